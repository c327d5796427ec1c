"""The saved JPEG (`cv2.imwrite(save_path, annotated)`, main.py:314, measurement.py:536) -- the host SPECIFICATION of vti_encode_jpeg.

The product encodes on the device (libvti.so `vti_encode_jpeg`, csrc/jpeg.hip, Engine.encode_jpeg), byte for byte what `encode`
below returns; the functions here stay as the statement of the rules and as the reference of tests/test_gpu_jpeg.py.  NumPy only.

The file is what libjpeg writes with its defaults at a given quality: baseline sequential, 8 bit, YCbCr 4:2:0, interleaved, one
scan, the Annex K quantisation tables scaled by jpeg_set_quality(q, force_baseline=TRUE), the Annex K Huffman tables, no restart
interval; SOI, APP0 (JFIF 1.01), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1, SOS, data, EOI.  All arithmetic is signed integer
(jccolor.c, jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c, jchuff.c).  PINNED against Pillow (libjpeg-turbo)
`Image.save(format="JPEG", quality=q, subsampling=2, optimize=False)` by tests/test_jpeg.py, whole file; cv2.imwrite uses libjpeg
with the same defaults, but OpenCV is not available here, so identity with cv2 itself is UNPINNED.
"""
import numpy as np

HEADER_BYTES = 623
MAX_BLOCK_BITS = 1658            # DC: 9 + 11; 63 AC coefficients of 16 + 10

# Annex K.1 quantisation tables, natural order
_QY = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
_QC = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, dtype=np.int64)
# zigzag position -> natural index
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)

# Annex K.3 Huffman tables: (bits[1..16], values)
DC0 = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC1 = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC0 = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
       [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
        0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
        0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
        0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
        0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
        0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
        0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
        0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa])
AC1 = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
       [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
        0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
        0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
        0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
        0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
        0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
        0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
        0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
        0xf9, 0xfa])
HUFFMAN = {"dc0": DC0, "ac0": AC0, "dc1": DC1, "ac1": AC1}


def quant_tables(quality):
    """jpeg_set_quality(q, TRUE): (luma, chroma) int64 [64] in natural order."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality must be in 1..100, got {quality!r}")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (_QY, _QC))


def huffman_codes(table):
    """The canonical codes of a (bits, values) list -> (code int64 [256], length int64 [256]); length 0: no such symbol."""
    bits, vals = table
    code = np.zeros(256, np.int64)
    size = np.zeros(256, np.int64)
    c, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code[vals[k]], size[vals[k]] = c, length
            c, k = c + 1, k + 1
        c <<= 1
    return code, size


def header(H0, W0, quality):
    """Everything before the entropy-coded data: SOI .. SOS, HEADER_BYTES long."""
    H0, W0 = int(H0), int(W0)
    if not (1 <= H0 <= 65535 and 1 <= W0 <= 65535):
        raise ValueError(f"frame size {H0}x{W0} outside 1..65535")
    qy, qc = quant_tables(quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for k, q in enumerate((qy, qc)):
        out += b"\xff\xdb\x00\x43" + bytes([k]) + bytes(q[ZIGZAG].astype(np.uint8))
    out += b"\xff\xc0\x00\x11\x08" + bytes([H0 >> 8, H0 & 255, W0 >> 8, W0 & 255]) + b"\x03\x01\x22\x00\x02\x11\x01\x03\x11\x01"
    for tc_th, name in ((0x00, "dc0"), (0x10, "ac0"), (0x01, "dc1"), (0x11, "ac1")):
        bits, vals = HUFFMAN[name]
        out += b"\xff\xc4" + bytes([0, 3 + 16 + len(vals), tc_th]) + bytes(bits) + bytes(vals)
    out += b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    assert len(out) == HEADER_BYTES
    return bytes(out)


def _fix(x):
    return int(x * 65536 + 0.5)


def _pad_edge(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def planes(frame, rgb=False):
    """jccolor.c + jcsample.c: (Y, Cb, Cr) int64 planes padded to their block extents (rules 1-4)."""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
        raise ValueError("frame must be uint8 [H0,W0,3]")
    f = f.astype(np.int64)
    R, G, B = (f[..., 0], f[..., 1], f[..., 2]) if rgb else (f[..., 2], f[..., 1], f[..., 0])
    Y = (_fix(.299) * R + _fix(.587) * G + _fix(.114) * B + 32768) >> 16
    Cb = (-_fix(.16874) * R - _fix(.33126) * G + _fix(.5) * B + (128 << 16) + 32767) >> 16
    Cr = (_fix(.5) * R - _fix(.41869) * G - _fix(.08131) * B + (128 << 16) + 32767) >> 16
    H0, W0 = Y.shape
    Y = _pad_edge(Y, 8 * -(-H0 // 8), 8 * -(-W0 // 8))
    ch, cw = -(-H0 // 2), -(-W0 // 2)
    cbr, cbc = -(-ch // 8), -(-cw // 8)
    bias = np.tile(np.array([1, 2], np.int64), 4 * cbc)
    chroma = []
    for P in (Cb, Cr):
        P = _pad_edge(P, 2 * ch, 16 * cbc)
        D = (P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + bias) >> 2
        chroma.append(_pad_edge(D, 8 * cbr, 8 * cbc))
    return Y, chroma[0], chroma[1]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One 1-D pass of jfdctint.c along the last axis of d [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        out[..., 0], out[..., 4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def _blocks(P, q):
    """Plane [8*br, 8*bc] -> quantised coefficients int64 [br, bc, 64] in zigzag order (rules 5-6)."""
    br, bc = P.shape[0] // 8, P.shape[1] // 8
    d = (P - 128).reshape(br, 8, bc, 8).transpose(0, 2, 1, 3)
    d = _fdct_pass(d, True)                                                 # rows
    d = _fdct_pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)    # columns
    c = d.reshape(br, bc, 64)
    q8 = 8 * q
    c = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    return c[..., ZIGZAG]


def scan_blocks(frame, quality=95, rgb=False):
    """-> (coef int64 [n_blocks, 64] zigzag, in scan order with the dummy blocks materialised; is_chroma bool [n_blocks])."""
    qy, qc = quant_tables(quality)
    Y, Cb, Cr = planes(frame, rgb)
    cy, cb, cr = _blocks(Y, qy), _blocks(Cb, qc), _blocks(Cr, qc)
    ybr, ybc = cy.shape[:2]
    H0, W0 = np.asarray(frame).shape[:2]
    mr, mc = -(-H0 // 16), -(-W0 // 16)
    assert cb.shape[:2] == (mr, mc)
    coef = np.zeros((mr, mc, 6, 64), np.int64)
    for k, (by, bx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        rows, cols = np.arange(mr) * 2 + by, np.arange(mc) * 2 + bx
        real = (rows < ybr)[:, None] & (cols < ybc)[None, :]
        src = cy[np.minimum(rows, ybr - 1)][:, np.minimum(cols, ybc - 1)]
        coef[:, :, k] = np.where(real[..., None], src, 0)
        if k:           # a dummy block: zero AC, the DC of the block before it in the MCU
            coef[:, :, k, 0] = np.where(real, coef[:, :, k, 0], coef[:, :, k - 1, 0])
    coef[:, :, 4], coef[:, :, 5] = cb, cr
    is_chroma = np.tile(np.array([0, 0, 0, 0, 1, 1], bool), mr * mc)
    return coef.reshape(-1, 64), is_chroma


def _bit_length(a):
    n = np.zeros(a.shape, np.int64)
    a = a.copy()
    while a.any():
        n += a > 0
        a >>= 1
    return n


def _emissions(coef, is_chroma, comp=None):
    """The scan as (table index 0..3 = dc0, ac0, dc1, ac1; symbol; extra-bit value; extra-bit count), in stream order.  comp: the
    component of every block (the 4:2:0 MCU's 0 0 0 0 1 2 unless given)."""
    nb = coef.shape[0]
    if comp is None:
        comp = np.tile(np.array([0, 0, 0, 0, 1, 2]), nb // 6)
    dc = coef[:, 0]
    diff = dc.copy()
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        diff[idx[1:]] = dc[idx[1:]] - dc[idx[:-1]]
    blk, pos = np.nonzero(coef[:, 1:])
    pos = pos + 1
    val = coef[blk, pos]
    first = np.ones(len(blk), bool)
    first[1:] = blk[1:] != blk[:-1]
    prev = np.where(first, 0, np.concatenate(([0], pos[:-1])))
    run = pos - prev - 1
    last = np.zeros(nb, np.int64)
    np.maximum.at(last, blk, pos)
    eob = np.nonzero(last < 63)[0]

    def amp(v):
        size = _bit_length(np.abs(v))
        return size, np.where(v < 0, v - 1, v) & ((1 << size) - 1)
    dsize, dbits = amp(diff)
    asize, abits = amp(val)
    nzrl = run >> 4
    zblk, zpos = np.repeat(blk, nzrl), np.repeat(pos, nzrl)
    # order: block, zigzag position, ZRLs before the coefficient's own symbol, EOB last
    b_all = np.concatenate((np.arange(nb), zblk, blk, eob))
    p_all = np.concatenate((np.zeros(nb, np.int64), zpos, pos, np.full(len(eob), 64)))
    s_all = np.concatenate((np.zeros(nb, np.int64), np.zeros(len(zblk), np.int64), np.ones(len(blk), np.int64), np.zeros(len(eob), np.int64)))
    sym = np.concatenate((dsize, np.full(len(zblk), 0xF0), ((run & 15) << 4) | asize, np.zeros(len(eob), np.int64)))
    ext = np.concatenate((dbits, np.zeros(len(zblk), np.int64), abits, np.zeros(len(eob), np.int64)))
    nex = np.concatenate((dsize, np.zeros(len(zblk), np.int64), asize, np.zeros(len(eob), np.int64)))
    is_ac = np.concatenate((np.zeros(nb, np.int64), np.ones(len(zblk) + len(blk) + len(eob), np.int64)))
    order = np.lexsort((s_all, p_all, b_all))
    tab = (2 * is_chroma[b_all].astype(np.int64) + is_ac)[order]
    return tab, sym[order], ext[order], nex[order]


def symbol_counts(frame, quality=95, rgb=False):
    """The Huffman symbol histogram per table: dict(dc0=int64 [12], ac0=int64 [256], dc1=..., ac1=...).  ac[0xF0] counts ZRL,
    ac[0x00] EOB, dc[11] the size-11 differences, ac[16 * run + 10] the size-10 coefficients."""
    tab, sym, _, _ = _emissions(*scan_blocks(frame, quality, rgb))
    return {name: np.bincount(sym[tab == k], minlength=n)[:n].astype(np.int64)
            for k, (name, n) in enumerate((("dc0", 12), ("ac0", 256), ("dc1", 12), ("ac1", 256)))}


def scan_bytes(frame, quality=95, rgb=False, stuffed=True):
    """The entropy-coded data: MSB first, the last byte padded with 1-bits, 0x00 after every 0xFF (rules 8-9)."""
    return _emission_bytes(*_emissions(*scan_blocks(frame, quality, rgb)), stuffed=stuffed)


def _emission_bytes(tab, sym, ext, nex, stuffed=True):
    """_emissions' stream coded with the Annex K tables -> bytes."""
    code, size = np.zeros((4, 256), np.int64), np.zeros((4, 256), np.int64)
    for k, name in enumerate(("dc0", "ac0", "dc1", "ac1")):
        code[k], size[k] = huffman_codes(HUFFMAN[name])
    clen = size[tab, sym]
    if not clen.all():
        raise ValueError("a symbol outside the Huffman table (coefficient out of the baseline range)")
    vals = (code[tab, sym] << nex) | ext
    lens = clen + nex
    total = int(lens.sum())
    idx = np.repeat(np.arange(len(lens)), lens)
    within = np.arange(total) - np.repeat(np.cumsum(lens) - lens, lens)
    bits = ((vals[idx] >> (lens[idx] - 1 - within)) & 1).astype(np.uint8)
    bits = np.concatenate((bits, np.ones(-total % 8, np.uint8)))
    data = np.packbits(bits)
    if not stuffed:
        return data.tobytes()
    ff = np.nonzero(data == 0xFF)[0]
    return np.insert(data, ff + 1, 0).tobytes()


def encode(frame, quality=95, rgb=False):
    """The JPEG file of a uint8 [H0,W0,3] frame (BGR as cv2's frames are, RGB with rgb=True) -> bytes."""
    H0, W0 = np.asarray(frame).shape[:2]
    return header(H0, W0, quality) + scan_bytes(frame, quality, rgb) + b"\xff\xd9"


# ---- decoding: the host SPECIFICATION of vti_decode_jpeg (csrc/jpeg_decode.hip, Engine.decode_jpeg) -------------------------------
# What cv2.imread / cap.read() of a motion-JPEG camera / PIL.Image.open do with libjpeg's defaults: jdhuff.c, jidctint.c (JDCT_ISLOW),
# jdsample.c fancy upsampling, jdcolor.c.  PINNED against Pillow (libjpeg-turbo) by tests/test_jpeg_decode.py, every pixel; identity
# with cv2.imread is expected (same library, same defaults) but OpenCV is not available here, so it is UNPINNED.
MAX_DECODE_SIDE = 8192


class UnsupportedJpeg(ValueError):
    """A well-formed file outside the supported class (the device call answers VTI_ERR_UNSUPPORTED)."""


def _derive_huffman(bits, vals):
    """jpeg_make_d_derived_tbl: -> (look uint16 [512] = length << 8 | symbol for codes of <= 9 bits, 0 otherwise; maxcode int [18];
    valoffset int [18]; huffval uint8 [256])."""
    if sum(bits) > 256 or sum(bits) != len(vals) or not vals:
        raise ValueError("bad Huffman table")
    look = np.zeros(512, np.uint16)
    maxcode = np.full(18, -1, np.int64)
    valoff = np.zeros(18, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        if bits[length - 1]:
            valoff[length] = k - code
            for _ in range(bits[length - 1]):
                if code >= 1 << length:
                    raise ValueError("bad Huffman table")
                if length <= 9:
                    look[code << (9 - length):(code + 1) << (9 - length)] = (length << 8) | vals[k]
                code, k = code + 1, k + 1
            maxcode[length] = code - 1
        code <<= 1
    maxcode[17] = 0xFFFFF
    hv = np.zeros(256, np.uint8)
    hv[:len(vals)] = vals
    return look, maxcode, valoff, hv


def parse(data):
    """The header of a supported file -> dict(H0, W0, hs, vs (luma sampling), quant int64 [3, 64] zigzag order per component,
    dc / ac: per component (bits, values), restart_interval, scan_start, scan_end (byte range of the entropy-coded data),
    mcu_rows, mcu_cols, blocks_per_mcu, n_blocks).  Raises UnsupportedJpeg for the refused classes, ValueError for malformed headers."""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise ValueError("not a JPEG file: no SOI marker")
    qt, dc_t, ac_t = {}, {}, {}
    sof = None
    ri = 0
    jfif, adobe = False, None
    p = 2
    while True:
        if p >= n:
            raise ValueError("truncated header: no SOS marker")
        if d[p] != 0xFF:
            raise ValueError(f"malformed header: byte {d[p]:#x} at {p} where a marker was expected")
        while p < n and d[p] == 0xFF:        # fill bytes
            p += 1
        if p >= n:
            raise ValueError("truncated header")
        m = d[p]
        p += 1
        if m == 0xD8 or 0xD0 <= m <= 0xD7 or m == 0x01:
            continue
        if m == 0xD9:
            raise ValueError("EOI before any scan")
        if p + 2 > n:
            raise ValueError("truncated header")
        L = (d[p] << 8) | d[p + 1]
        if L < 2 or p + L > n:
            raise ValueError("truncated header: a segment runs past the end of the file")
        body = d[p + 2:p + L]
        if m == 0xC0:
            if sof is not None:
                raise ValueError("two SOF markers")
            if len(body) < 6 or len(body) != 6 + 3 * body[5]:
                raise ValueError("bad SOF0 length")
            sof = body
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7):
            raise UnsupportedJpeg({0xC2: "progressive", 0xC1: "extended sequential"}.get(m, "lossless or differential")
                                  + " JPEG: only baseline sequential (SOF0) is decoded")
        elif m in (0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            raise UnsupportedJpeg("arithmetic coding is not decoded")
        elif m == 0xDB:
            q = 0
            while q < len(body):
                pq, tq = body[q] >> 4, body[q] & 15
                if pq == 1:
                    raise UnsupportedJpeg("16-bit quantisation table")
                if pq or tq > 3 or q + 65 > len(body):
                    raise ValueError("bad DQT segment")
                qt[tq] = np.frombuffer(body[q + 1:q + 65], np.uint8).astype(np.int64)
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                if q + 17 > len(body):
                    raise ValueError("bad DHT segment")
                tc, th = body[q] >> 4, body[q] & 15
                bits = list(body[q + 1:q + 17])
                cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or q + 17 + cnt > len(body):
                    raise ValueError("bad DHT segment")
                vals = list(body[q + 17:q + 17 + cnt])
                _derive_huffman(bits, vals)
                (ac_t if tc else dc_t)[th] = (bits, vals)
                q += 17 + cnt
        elif m == 0xDD:
            if len(body) != 2:
                raise ValueError("bad DRI segment")
            ri = (body[0] << 8) | body[1]
        elif m == 0xE0 and body[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDA:
            break
        p += L
    if sof is None:
        raise ValueError("SOS before SOF")
    prec, H0, W0, nc = sof[0], (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    if prec != 8:
        raise UnsupportedJpeg(f"{prec}-bit samples: only 8-bit is decoded")
    if nc == 1:
        raise UnsupportedJpeg("greyscale file: only three-component YCbCr is decoded")
    if nc != 3:
        raise UnsupportedJpeg(f"{nc} components: only three-component YCbCr is decoded")
    if not (1 <= H0 <= MAX_DECODE_SIDE and 1 <= W0 <= MAX_DECODE_SIDE):
        raise UnsupportedJpeg(f"frame size {H0}x{W0} outside 1..{MAX_DECODE_SIDE}")
    comps = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(3)]
    if adobe is not None and adobe != 1:
        raise UnsupportedJpeg(f"Adobe transform {adobe}: only YCbCr (transform 1) is decoded")
    if adobe is None and not jfif and [c[0] for c in comps] == [82, 71, 66]:
        raise UnsupportedJpeg("RGB components: only YCbCr is decoded")
    hs, vs = comps[0][1], comps[0][2]
    if (hs, vs) not in ((2, 2), (2, 1), (1, 1)) or any(c[1] != 1 or c[2] != 1 for c in comps[1:]):
        raise UnsupportedJpeg("sampling factors " + ",".join(f"{c[1]}x{c[2]}" for c in comps)
                              + ": only 2x2, 2x1 or 1x1 luma with 1x1 chroma is decoded")
    if len(body) < 1 or len(body) != 4 + 2 * body[0]:
        raise ValueError("bad SOS length")
    if body[0] != 3:
        raise UnsupportedJpeg("a scan that does not interleave all three components (multiple scans)")
    sel = []
    for i in range(3):
        if body[1 + 2 * i] != comps[i][0]:
            raise UnsupportedJpeg("scan components out of frame order")
        sel.append((body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15))
    if body[7] != 0 or body[8] != 63 or body[9] != 0:
        raise UnsupportedJpeg("spectral selection or successive approximation in a sequential scan")
    default_dc = {0: DC0, 1: DC1}
    default_ac = {0: AC0, 1: AC1}
    if not dc_t and not ac_t:                      # motion-JPEG: no DHT, the Annex K tables
        dc_t, ac_t = default_dc, default_ac
    quant, dcs, acs = [], [], []
    for i in range(3):
        if comps[i][3] not in qt:
            raise ValueError(f"component {i} uses quantisation table {comps[i][3]}, which the file does not define")
        if sel[i][0] not in dc_t or sel[i][1] not in ac_t:
            raise ValueError(f"component {i} uses a Huffman table the file does not define")
        quant.append(qt[comps[i][3]])
        dcs.append(dc_t[sel[i][0]])
        acs.append(ac_t[sel[i][1]])
    scan_start = p + L
    q = scan_start
    while True:                                    # the scan ends at the first marker that is not RSTn (or at the end of the file)
        q = d.find(b"\xff", q)
        if q < 0 or q + 1 >= n:
            scan_end = n
            break
        if d[q + 1] == 0 or 0xD0 <= d[q + 1] <= 0xD7 or d[q + 1] == 0xFF:
            q += 1 if d[q + 1] == 0xFF else 2
            continue
        scan_end = q
        break
    r = scan_end
    while r + 1 < n:                               # anything but EOI after the scan: another scan or tables for one
        if d[r] == 0xFF and d[r + 1] == 0xDA:
            raise UnsupportedJpeg("multiple scans")
        if d[r] == 0xFF and d[r + 1] == 0xD9:
            break
        r += 1
    mcu_rows, mcu_cols = -(-H0 // (8 * vs)), -(-W0 // (8 * hs))
    bpm = hs * vs + 2
    return dict(H0=H0, W0=W0, hs=hs, vs=vs, quant=np.stack(quant), dc=dcs, ac=acs, restart_interval=ri, scan_start=scan_start,
                scan_end=scan_end, mcu_rows=mcu_rows, mcu_cols=mcu_cols, blocks_per_mcu=bpm, n_blocks=mcu_rows * mcu_cols * bpm)


_LOOKUPS = {}


def _full_lookup(table):
    """(bits, values) -> lists [65536]: the code length (0: invalid) and the symbol of every 16-bit window."""
    key = (tuple(table[0]), tuple(table[1]))
    if key not in _LOOKUPS:
        if len(_LOOKUPS) > 64:
            _LOOKUPS.clear()
        _LOOKUPS[key] = _build_lookup(table)
    return _LOOKUPS[key]


def _build_lookup(table):
    bits, vals = table
    ln, sy = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            ln[code << (16 - length):(code + 1) << (16 - length)] = length
            sy[code << (16 - length):(code + 1) << (16 - length)] = vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return ln.tolist(), sy.tolist()


def decode_coefficients(data, hdr=None):
    """jdhuff.c: -> (coef int64 [n_blocks, 64] in zigzag order with the DC values summed, in scan order; ok bool).  ok is False for
    a damaged scan (an invalid code, data that ends early, a missing or misnumbered RSTn); the coefficients are then unspecified."""
    d = bytes(data)
    h = hdr or parse(d)
    nblk, bpm, ri = h["n_blocks"], h["blocks_per_mcu"], h["restart_interval"]
    comp_of = [0] * (bpm - 2) + [1, 2]
    dct = [_full_lookup(t) for t in h["dc"]]
    act = [_full_lookup(t) for t in h["ac"]]
    coef = np.zeros((nblk, 64), np.int64)
    raw = d[h["scan_start"]:h["scan_end"]]
    # the restart intervals: split at RSTn, unstuffed, each a list of 32-bit windows by byte
    parts, nums, s = [], [], 0
    while True:
        q = s
        while True:
            q = raw.find(b"\xff", q)
            if q < 0 or q + 1 >= len(raw):
                q = len(raw)
                break
            if 0xD0 <= raw[q + 1] <= 0xD7:
                break
            q += 2 if raw[q + 1] == 0 else 1
        parts.append(raw[s:q].replace(b"\xff\x00", b"\xff"))
        if q >= len(raw):
            break
        nums.append(raw[q + 1] & 7)
        s = q + 2
    ok = nums == [i & 7 for i in range(len(nums))]
    per = ri * bpm if ri else nblk
    blk = 0
    for pi, part in enumerate(parts):
        if blk >= nblk:
            ok = ok and pi == len(parts)       # data after the last block
            break
        if blk != pi * per:
            ok = False
            blk = pi * per
            if blk >= nblk:
                break
        a = np.frombuffer(part + b"\0\0\0\0", np.uint8).astype(np.int64)
        win = ((a[:-3] << 24) | (a[1:-2] << 16) | (a[2:-1] << 8) | a[3:]).tolist()
        nbits, pos = 8 * len(part), 0
        pred = [0, 0, 0]
        end = min(nblk, blk + per)
        flat = coef.reshape(-1)
        out = {}
        while blk < end:
            c = comp_of[blk % bpm]
            ln, sy = dct[c]
            w = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF if (pos >> 3) < len(win) else 0
            n_ = ln[w]
            if not n_ or pos + n_ > nbits:
                ok = False
                break
            pos += n_
            s_ = sy[w] & 15
            if s_:
                if pos + s_ > nbits:
                    ok = False
                    break
                v = (win[pos >> 3] >> (32 - s_ - (pos & 7))) & ((1 << s_) - 1)
                pos += s_
                if v < 1 << (s_ - 1):
                    v += 1 - (1 << s_)
                pred[c] += v
            base = blk * 64
            out[base] = pred[c]
            ln, sy = act[c]
            k = 1
            bad = False
            while k < 64:
                w = (win[pos >> 3] >> (16 - (pos & 7))) & 0xFFFF if (pos >> 3) < len(win) else 0
                n_ = ln[w]
                if not n_ or pos + n_ > nbits:
                    bad = True
                    break
                pos += n_
                rs = sy[w]
                s_ = rs & 15
                if s_:
                    k += rs >> 4
                    if pos + s_ > nbits:
                        bad = True
                        break
                    v = (win[pos >> 3] >> (32 - s_ - (pos & 7))) & ((1 << s_) - 1)
                    pos += s_
                    if k > 63:
                        bad = True
                        break
                    if v < 1 << (s_ - 1):
                        v += 1 - (1 << s_)
                    out[base + k] = v
                    k += 1
                elif rs == 0xF0:
                    k += 16
                else:
                    break
            if bad:
                ok = False
                break
            blk += 1
        if out:
            flat[np.fromiter(out.keys(), np.int64, len(out))] = np.fromiter(out.values(), np.int64, len(out))
        if blk < end:
            break
    if blk < nblk:
        ok = False
    return coef, ok


def _idct_pass(d, n):
    """One 1-D pass of jidctint.c along the last axis of d [..., 8], descaled by n bits."""
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * 4433
    t2, t3 = z1 - z3 * 15137, z1 + z2 * 6270
    t0, t1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    r = 1 << (n - 1)
    return np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], -1) + r >> n


def idct_blocks(coef, quant):
    """Dequantisation + jpeg_idct_islow: coef int64 [..., 64] zigzag, quant int64 [64] zigzag -> samples int64 [..., 8, 8] in 0..255."""
    nat = np.zeros(coef.shape, np.int64)
    nat[..., ZIGZAG] = coef * quant
    b = nat.reshape(coef.shape[:-1] + (8, 8))
    b = _idct_pass(b.swapaxes(-1, -2), 11).swapaxes(-1, -2)       # columns
    b = _idct_pass(b, 18)                                         # rows
    v = b & 1023                                                  # the range-limit table behind RANGE_MASK, centred on 128
    return np.where(v < 128, v + 128, np.where(v < 512, 255, np.where(v < 896, 0, v - 896)))


def _upsample_h(P, fancy):
    """jdsample.c along the rows: [h, cw] -> [h, 2 cw]."""
    out = np.empty((P.shape[0], 2 * P.shape[1]), np.int64)
    if not fancy:
        out[:, 0::2], out[:, 1::2] = P, P
        return out
    left, right = np.roll(P, 1, 1), np.roll(P, -1, 1)
    out[:, 0::2], out[:, 1::2] = (3 * P + left + 1) >> 2, (3 * P + right + 2) >> 2
    out[:, 0], out[:, -1] = P[:, 0], P[:, -1]
    return out


def upsample(P, hs, vs):
    """A chroma plane of the real downsampled size [ceil(H0/vs), ceil(W0/hs)] -> [vs * ., hs * .]: fancy upsampling when the plane
    is more than two samples wide (jinit_upsampler), sample replication otherwise."""
    if hs == 1:
        return P
    fancy = P.shape[1] > 2
    if vs == 1:
        return _upsample_h(P, fancy)
    if not fancy:
        return np.repeat(_upsample_h(P, False), 2, 0)
    up, down = np.vstack((P[:1], P[:-1])), np.vstack((P[1:], P[-1:]))
    out = np.empty((2 * P.shape[0], 2 * P.shape[1]), np.int64)
    for k, other in enumerate((up, down)):
        s = 3 * P + other
        left, right = np.roll(s, 1, 1), np.roll(s, -1, 1)
        even, odd = (3 * s + left + 8) >> 4, (3 * s + right + 7) >> 4
        even[:, 0], odd[:, -1] = (4 * s[:, 0] + 8) >> 4, (4 * s[:, -1] + 7) >> 4
        out[k::2, 0::2], out[k::2, 1::2] = even, odd
    return out


def pixels_from_coefficients(coef, hdr, rgb=True):
    """IDCT, upsampling and colour conversion of decode_coefficients' blocks -> uint8 [H0, W0, 3]."""
    H0, W0, hs, vs = hdr["H0"], hdr["W0"], hdr["hs"], hdr["vs"]
    mr, mc, bpm = hdr["mcu_rows"], hdr["mcu_cols"], hdr["blocks_per_mcu"]
    c = coef.reshape(mr, mc, bpm, 64)
    Y = idct_blocks(c[:, :, :hs * vs], hdr["quant"][0]).reshape(mr, mc, vs, hs, 8, 8).transpose(0, 2, 4, 1, 3, 5)
    Y = Y.reshape(mr * vs * 8, mc * hs * 8)[:H0, :W0]
    ch, cw = -(-H0 // vs), -(-W0 // hs)
    chroma = []
    for k in (1, 2):
        P = idct_blocks(c[:, :, hs * vs + k - 1], hdr["quant"][k]).transpose(0, 2, 1, 3).reshape(mr * 8, mc * 8)[:ch, :cw]
        chroma.append(upsample(P, hs, vs)[:H0, :W0] - 128)
    cb, cr = chroma
    R = Y + ((_fix(1.40200) * cr + 32768) >> 16)
    G = Y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    B = Y + ((_fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack((R, G, B) if rgb else (B, G, R), -1), 0, 255).astype(np.uint8)


def decode(data, rgb=True):
    """A supported JPEG file -> uint8 [H0, W0, 3], RGB as PIL.Image.open gives it (rgb=False: BGR, as cv2.imread / cap.read())."""
    hdr = parse(data)
    coef, _ = decode_coefficients(data, hdr)
    return pixels_from_coefficients(coef, hdr, rgb)
