"""Raw camera frames -> BGR on the host: the specification vti_convert_raw equals byte for byte (NumPy only).

What `cap.read()` returns for a V4L2 camera that delivers raw YUV is OpenCV's cvtColor(COLOR_YUV2BGR_*) of the buffer; with
`cap.set(cv2.CAP_PROP_CONVERT_RGB, 0)` it returns the buffer itself.  The rules below restate OpenCV 4.x's
imgproc/src/color_yuv.simd.hpp (BT.601, limited range, 20-bit fixed point):

    CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, SHIFT = 20
    u' = U - 128, v' = V - 128
    ruv = (1 << 19) + CVR*v'     guv = (1 << 19) + CVG*v' + CUG*u'     buv = (1 << 19) + CUB*u'
    y'  = max(0, Y - 16) * CY
    R = clamp((y' + ruv) >> 20)  G = clamp((y' + guv) >> 20)  B = clamp((y' + buv) >> 20)      (arithmetic shift, clamp to 0..255)

Chroma is replicated, never interpolated: one (U, V) serves a horizontal pixel pair in 4:2:2 and a 2x2 block in 4:2:0.  Frames
are tightly packed (no line padding):

    yuyv (0)  2*H0*W0 bytes    per pixel pair  Y0 U Y1 V                                  COLOR_YUV2BGR_YUYV
    uyvy (1)  2*H0*W0          U Y0 V Y1                                                  COLOR_YUV2BGR_UYVY
    nv12 (2)  H0*W0*3/2        Y plane, then interleaved U V (H0/2 x W0/2 pairs)          COLOR_YUV2BGR_NV12
    nv21 (3)  H0*W0*3/2        Y plane, then interleaved V U                              COLOR_YUV2BGR_NV21
    i420 (4)  H0*W0*3/2        Y plane, U plane, V plane                                  COLOR_YUV2BGR_I420
    yv12 (5)  H0*W0*3/2        Y plane, V plane, U plane                                  COLOR_YUV2BGR_YV12

W0 is even for 4:2:2, H0 and W0 are even for 4:2:0, 2 <= H0, W0 <= 8192.  Every byte string of the right length is a frame.
"""
import numpy as np

YUYV, UYVY, NV12, NV21, I420, YV12 = range(6)
FORMATS = {"yuyv": YUYV, "uyvy": UYVY, "nv12": NV12, "nv21": NV21, "i420": I420, "yv12": YV12}
NAMES = {v: k for k, v in FORMATS.items()}
MAX_SIDE = 8192

CY, CUB, CUG, CVG, CVR, SHIFT = 1220542, 2116026, -409993, -852492, 1673527, 20


def format_id(fmt):
    """A format's enum value from its name (any case) or the value itself; ValueError for anything else."""
    if isinstance(fmt, str):
        v = FORMATS.get(fmt.lower())
        if v is None:
            raise ValueError(f"unknown raw format {fmt!r}: one of {sorted(FORMATS)}")
        return v
    if isinstance(fmt, (bool, np.bool_)) or not isinstance(fmt, (int, np.integer)) or int(fmt) not in NAMES:
        raise ValueError(f"unknown raw format {fmt!r}: one of {sorted(FORMATS)} or 0..5")
    return int(fmt)


def frame_bytes(fmt, H0, W0):
    """Bytes of one H0 x W0 frame of `fmt`; ValueError for a size the format does not have."""
    f = format_id(fmt)
    for name, v in (("H0", H0), ("W0", W0)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} must be an integer, got {v!r}")
    H0, W0 = int(H0), int(W0)
    if not (2 <= H0 <= MAX_SIDE and 2 <= W0 <= MAX_SIDE):
        raise ValueError(f"a raw frame is 2..{MAX_SIDE} pixels high and wide, got {H0}x{W0}")
    if W0 & 1:
        raise ValueError(f"{NAMES[f]} needs an even W0, got {W0}")
    if f >= NV12 and H0 & 1:
        raise ValueError(f"{NAMES[f]} needs an even H0, got {H0}")
    return 2 * H0 * W0 if f < NV12 else H0 * W0 * 3 // 2


def as_bytes(raw, what="raw"):
    """Any uint8 array, bytes, bytearray or memoryview -> a flat uint8 ndarray (a view where the input allows it)."""
    if isinstance(raw, (bytes, bytearray, memoryview)):
        return np.frombuffer(raw, np.uint8)
    a = np.asarray(raw)
    if a.dtype != np.uint8:
        raise ValueError(f"{what} must be uint8, got {a.dtype}")
    return np.ascontiguousarray(a).reshape(-1)


def planes(raw, fmt, H0, W0):
    """-> (Y [n,H0,W0], U, V at the chroma resolution: [n,H0,W0/2] for 4:2:2, [n,H0/2,W0/2] for 4:2:0), uint8 views."""
    f = format_id(fmt)
    fb = frame_bytes(f, H0, W0)
    a = as_bytes(raw)
    if a.size == 0 or a.size % fb:
        raise ValueError(f"{NAMES[f]} {H0}x{W0}: expected a multiple of {fb} bytes, got {a.size}")
    n = a.size // fb
    a = a.reshape(n, fb)
    if f < NV12:
        q = a.reshape(n, H0, W0 // 2, 4)
        if f == YUYV:
            return q[..., 0::2].reshape(n, H0, W0), q[..., 1], q[..., 3]
        return q[..., 1::2].reshape(n, H0, W0), q[..., 0], q[..., 2]
    Y = a[:, :H0 * W0].reshape(n, H0, W0)
    c = a[:, H0 * W0:]
    if f in (NV12, NV21):
        c = c.reshape(n, H0 // 2, W0 // 2, 2)
        return (Y, c[..., 0], c[..., 1]) if f == NV12 else (Y, c[..., 1], c[..., 0])
    c = c.reshape(n, 2, H0 // 2, W0 // 2)
    return (Y, c[:, 0], c[:, 1]) if f == I420 else (Y, c[:, 1], c[:, 0])


def yuv_to_bgr(Y, U, V):
    """The pixel rule on arrays of equal shape -> uint8 [..., 3] in B, G, R order."""
    y = np.maximum(np.asarray(Y, np.int64) - 16, 0) * CY
    u = np.asarray(U, np.int64) - 128
    v = np.asarray(V, np.int64) - 128
    half = 1 << (SHIFT - 1)
    b = (y + half + CUB * u) >> SHIFT
    g = (y + half + CVG * v + CUG * u) >> SHIFT
    r = (y + half + CVR * v) >> SHIFT
    return np.clip(np.stack((b, g, r), -1), 0, 255).astype(np.uint8)


def to_bgr(raw, fmt, H0, W0, rgb=False):
    """n raw frames (any uint8 array or bytes of n * frame_bytes bytes) -> uint8 [n,H0,W0,3]: B, G, R as cap.read() gives them, or
    R, G, B with rgb=True."""
    f = format_id(fmt)
    Y, U, V = planes(raw, f, H0, W0)
    U, V = np.repeat(U, 2, axis=2), np.repeat(V, 2, axis=2)
    if f >= NV12:
        U, V = np.repeat(U, 2, axis=1), np.repeat(V, 2, axis=1)
    out = yuv_to_bgr(Y, U, V)
    return np.ascontiguousarray(out[..., ::-1]) if rgb else out


def from_planes(Y, U, V, fmt):
    """The inverse of planes(): Y [n,H0,W0] (or [H0,W0]) and U, V at the format's chroma resolution -> uint8 [n, frame_bytes]."""
    f = format_id(fmt)
    Y, U, V = (np.asarray(x, np.uint8) for x in (Y, U, V))
    if Y.ndim == 2:
        Y, U, V = Y[None], U[None], V[None]
    n, H0, W0 = Y.shape
    fb = frame_bytes(f, H0, W0)
    cs = (n, H0, W0 // 2) if f < NV12 else (n, H0 // 2, W0 // 2)
    if U.shape != cs or V.shape != cs:
        raise ValueError(f"{NAMES[f]}: U and V must have shape {cs}, got {U.shape} and {V.shape}")
    if f < NV12:
        q = np.empty((n, H0, W0 // 2, 4), np.uint8)
        yi, ui, vi = ((0, 1, 3) if f == YUYV else (1, 0, 2))
        q[..., yi], q[..., yi + 2] = Y[..., 0::2], Y[..., 1::2]
        q[..., ui], q[..., vi] = U, V
        return q.reshape(n, fb)
    out = np.empty((n, fb), np.uint8)
    out[:, :H0 * W0] = Y.reshape(n, -1)
    c = out[:, H0 * W0:]
    if f in (NV12, NV21):
        c = c.reshape(n, H0 // 2, W0 // 2, 2)
        c[..., 0], c[..., 1] = (U, V) if f == NV12 else (V, U)
    else:
        c = c.reshape(n, 2, H0 // 2, W0 // 2)
        c[:, 0], c[:, 1] = (U, V) if f == I420 else (V, U)
    return out
