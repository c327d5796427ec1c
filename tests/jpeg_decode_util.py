"""Seeded JPEG files for the decoder's tests.  The golden set (tests/golden/jpeg_decode_pillow.npz, written with Pillow by
tests/golden/make_jpeg_decode_golden.py) holds Pillow's files and pixels; the GPU tests make their files with the package's own
encoder-side restatement and header patches, so they need no PIL."""
import ctypes as C

import numpy as np

import jpeg_util as J

SAMPLINGS = {"420": (2, 2), "422": (2, 1), "444": (1, 1)}
PIL_SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def golden_cases():
    """[(key, content, h, w, sampling, quality, save options)] of the golden file."""
    out = []
    for (h, w) in J.SIZES:
        for ss in SAMPLINGS:
            c = "noise" if h * w <= 17 * 33 else "checker"      # noise does not compress: the large frames are checkerboards
            out.append((f"{c}_{h}x{w}_{ss}_q95", c, h, w, ss, 95, {}))
    for (h, w) in ((3, 5), (9, 4), (2, 70)):        # narrow planes (replication instead of fancy upsampling), odd edges
        for ss in SAMPLINGS:
            out.append((f"ramp_{h}x{w}_{ss}_q95", "ramp", h, w, ss, 95, {}))
    for ss in SAMPLINGS:
        for q in (100, 50, 10, 1):
            for c in ("noise", "ramp"):
                out.append((f"{c}_17x33_{ss}_q{q}", c, 17, 33, ss, q, {}))
        for c in J.CONTENTS:
            h, w = (50, 70) if ss == "420" and c != "noise" else (17, 33)
            out.append((f"{c}_{h}x{w}_{ss}_q95_all", c, h, w, ss, 95, {}))
        h, w = (50, 70) if ss == "422" else (17, 33)
        out.append((f"ramp_{h}x{w}_{ss}_q95_opt", "ramp", h, w, ss, 95, dict(optimize=True)))
        out.append((f"noise_17x33_{ss}_q100_opt", "noise", 17, 33, ss, 100, dict(optimize=True)))
        out.append((f"noise_17x33_{ss}_q95_rb2", "noise", 17, 33, ss, 95, dict(restart_marker_blocks=2)))
        out.append((f"checker_135x241_{ss}_q50_rr1", "checker", 135, 241, ss, 50, dict(restart_marker_rows=1)))
        out.append((f"zrl_50x70_{ss}_q95_rb2", "zrl", 50, 70, ss, 95, dict(restart_marker_blocks=2)))
        h, w = (50, 70) if ss == "444" else (17, 33)
        out.append((f"ramp_{h}x{w}_{ss}_q95_nodht", "ramp", h, w, ss, 95, dict(strip_dht=True)))
    out.append(("checker_135x241_422_q100", "checker", 135, 241, "422", 100, {}))
    return out


def segments(data):
    """[(marker, start, end)] of the header's marker segments up to and including SOS (start at the 0xFF)."""
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m, L = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        out.append((m, p, p + 2 + L))
        if m == 0xDA:
            return out
        p += 2 + L


def strip_dht(data):
    """The file without its DHT segments, as a motion-JPEG camera sends it (valid only for files written with the Annex K tables)."""
    out, last = bytearray(data[:2]), 2
    for m, a, b in segments(data):
        if m != 0xC4:
            out += data[a:b]
        last = b
    return bytes(out + data[last:])


def set_sampling(data, sampling):
    """Patches the SOF0 luma sampling factors of a jpeg.header() (4:2:0) file header."""
    hs, vs = SAMPLINGS[sampling]
    d = bytearray(data)
    for m, a, b in segments(data):
        if m == 0xC0:
            d[a + 11] = (hs << 4) | vs
    return bytes(d)


def own_file(frame_bgr, quality, sampling="420", restart=0, with_dht=True):
    """A JPEG file of `frame_bgr` made without PIL from the package's encoder-side restatement (jpeg.py: colour conversion, FDCT,
    quantisation, Huffman coding with the Annex K tables); the chroma planes are plain box averages -- any valid file will do.
    restart > 0: a DRI segment and RSTn markers every `restart` MCUs."""
    from vti_amd import jpeg
    f = np.asarray(frame_bgr)
    H0, W0 = f.shape[:2]
    hs, vs = SAMPLINGS[sampling]
    qy, qc = jpeg.quant_tables(quality)
    x = f.astype(np.int64)
    R, G, B = x[..., 2], x[..., 1], x[..., 0]
    fix = lambda v: int(v * 65536 + 0.5)
    Y = (fix(.299) * R + fix(.587) * G + fix(.114) * B + 32768) >> 16
    Cb = (-fix(.16874) * R - fix(.33126) * G + fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (fix(.5) * R - fix(.41869) * G - fix(.08131) * B + (128 << 16) + 32767) >> 16
    mr, mc = -(-H0 // (8 * vs)), -(-W0 // (8 * hs))
    pad = lambda P, r, c: np.pad(P, ((0, r - P.shape[0]), (0, c - P.shape[1])), mode="edge")
    Yp = pad(Y, mr * 8 * vs, mc * 8 * hs)
    chroma = []
    for P in (Cb, Cr):
        P = pad(P, mr * 8 * vs, mc * 8 * hs)
        chroma.append(P.reshape(mr * 8, vs, mc * 8, hs).sum((1, 3)) // (hs * vs))      # a plain box average: any valid file will do
    cy, cb, cr = jpeg._blocks(Yp, qy), jpeg._blocks(chroma[0], qc), jpeg._blocks(chroma[1], qc)
    bpm = hs * vs + 2
    coef = np.zeros((mr, mc, bpm, 64), np.int64)
    for by in range(vs):
        for bx in range(hs):
            coef[:, :, by * hs + bx] = cy[by::vs, bx::hs]
    coef[:, :, bpm - 2], coef[:, :, bpm - 1] = cb, cr
    coef = coef.reshape(-1, bpm, 64)
    if not restart:             # the vectorised coder of jpeg.py
        comp = np.tile(np.array([0] * (bpm - 2) + [1, 2]), coef.shape[0])
        scan = jpeg._emission_bytes(*jpeg._emissions(coef.reshape(-1, 64), comp > 0, comp))
        data = set_sampling(jpeg.header(H0, W0, quality), sampling) + scan + b"\xff\xd9"
        return data if with_dht else strip_dht(data)
    codes = [jpeg.huffman_codes(jpeg.HUFFMAN[k]) for k in ("dc0", "ac0", "dc1", "ac1")]
    out = bytearray()
    acc, nacc = 0, 0
    pred = [0, 0, 0]

    def put(v, n):
        nonlocal acc, nacc
        acc, nacc = (acc << n) | v, nacc + n
        while nacc >= 8:
            byte = (acc >> (nacc - 8)) & 0xFF
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
            nacc -= 8
        acc &= (1 << nacc) - 1

    def amp(v):
        s = int(abs(v)).bit_length()
        return s, (v - 1 if v < 0 else v) & ((1 << s) - 1)
    nrst = 0
    for m in range(coef.shape[0]):
        if restart and m and m % restart == 0:
            if nacc:
                put((1 << (8 - nacc)) - 1, 8 - nacc)
            out += bytes([0xFF, 0xD0 + (nrst & 7)])
            nrst += 1
            pred = [0, 0, 0]
        for b in range(bpm):
            c = 0 if b < bpm - 2 else b - (bpm - 2) + 1
            t = 0 if c == 0 else 2
            blk = [int(v) for v in coef[m, b]]
            s, bits = amp(blk[0] - pred[c])
            pred[c] = blk[0]
            put(int(codes[t][0][s]), int(codes[t][1][s]))
            put(bits, s)
            run = 0
            last = max([k for k in range(1, 64) if blk[k]] or [0])
            for k in range(1, last + 1):
                if not blk[k]:
                    run += 1
                    continue
                while run > 15:
                    put(int(codes[t + 1][0][0xF0]), int(codes[t + 1][1][0xF0]))
                    run -= 16
                s, bits = amp(blk[k])
                put(int(codes[t + 1][0][(run << 4) | s]), int(codes[t + 1][1][(run << 4) | s]))
                put(bits, s)
                run = 0
            if last < 63:
                put(int(codes[t + 1][0][0]), int(codes[t + 1][1][0]))
    if nacc:
        put((1 << (8 - nacc)) - 1, 8 - nacc)
    head = set_sampling(jpeg.header(H0, W0, quality), sampling)
    if restart:
        sos = head.rindex(b"\xff\xda")
        head = head[:sos] + bytes([0xFF, 0xDD, 0, 4, restart >> 8, restart & 255]) + head[sos:]
    data = head + bytes(out) + b"\xff\xd9"
    return data if with_dht else strip_dht(data)


def plan(vti_amd, files, segment_bytes=0, layout=0, ctx=None):
    """vti_decode_jpeg_plan through the C ABI -> dict(blob, offs, table, H0, W0, out_off, scratch_bytes) (numpy arrays)."""
    L = vti_amd.lib()
    n = len(files)
    blob = np.frombuffer(b"".join(files) + b"\0", np.uint8).copy()
    offs = np.cumsum([0] + [len(f) for f in files]).astype(np.int64)
    nb = int(L.vti_decode_jpeg_table_bytes(n))
    table = np.zeros(nb, np.uint8)
    H0, W0, out_off, scratch = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n + 1, np.int64), C.c_int64(0)
    rc = L.vti_decode_jpeg_plan(ctx, blob.ctypes.data, offs.ctypes.data, n, segment_bytes, layout, table.ctypes.data, nb, H0.ctypes.data,
                                W0.ctypes.data, out_off.ctypes.data, C.byref(scratch))
    msg = L.vti_last_error(ctx)
    return rc, dict(blob=blob, offs=offs, table=table, H0=H0, W0=W0, out_off=out_off, scratch_bytes=int(scratch.value),
                    error=msg.decode() if msg else "")
