"""Thin host wrapper around one libvti context: owns the torch-ROCm tensors the C ABI writes into.

PyTorch is plumbing here (device memory + the current HIP stream); all arithmetic runs in
libvti.so's HIP kernels.  Replaces the predictor object Ultralytics builds lazily on the first
`model.predict(...)` (reference: measurement.py:208-210).
"""
import contextlib
import ctypes as C
import dataclasses

import numpy as np
import torch

from . import _lib, rawframes
from . import overlay as _ov
from ._lib import VtiCheckerParams, VtiConvInfo, VtiDesc, VtiMeasureParams, VtiNmsParams, check, lib

# "h2": split-fp16 storage (every element an fp16 (hi, lo) pair, all products on the fp16 matrix pipe): the dtype whose results
# meet the reference tolerance (mask IoU >= 0.999, |d box| < 1e-3) at a multiple of the fp32 engine's rate -- include/vti.h
DTYPES = {"fp16": _lib.VTI_F16, "f16": _lib.VTI_F16, "half": _lib.VTI_F16,
          "fp32": _lib.VTI_F32, "f32": _lib.VTI_F32, "float": _lib.VTI_F32,
          "h2": _lib.VTI_H2, "fp16x2": _lib.VTI_H2, "split": _lib.VTI_H2}
_DTYPE_NAME = {_lib.VTI_F16: "fp16", _lib.VTI_F32: "fp32", _lib.VTI_H2: "h2"}
MASK_MODES = {"logit": _lib.VTI_MASK_LOGIT, "sigmoid": _lib.VTI_MASK_SIGMOID}
PACKINGS = {"u8": _lib.VTI_PACK_U8, "bits": _lib.VTI_PACK_BITS}
POLY_STRATEGIES = {"largest": _lib.VTI_POLY_LARGEST, "concat": _lib.VTI_POLY_CONCAT}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- argument checks shared by measure, measure_checker, annotate, annotate_checker and overlay (`who`: the method's name) ----------
def _select(who, select, B):
    """select -> the frame indices as a contiguous int32 array, each in [0, B)."""
    sel = np.asarray(select.cpu().numpy() if isinstance(select, torch.Tensor) else select)
    if sel.ndim != 1 or sel.size < 1 or sel.dtype.kind not in "iu":
        raise ValueError(f"{who}: select must be a non-empty sequence of frame indices")
    if sel.min() < 0 or sel.max() >= B:
        raise ValueError(f"{who}: frame index outside [0, {B})")
    return np.ascontiguousarray(sel, dtype=np.int32)


def _uniform_frames(who, frames):
    """A batch of frames of one size -> (B, H0, W0)."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"{who}: frames must be a uint8 [B,H0,W0,3] tensor")
    return frames.shape[:3]


def _measure_result(result, B, capacity, stitch_rows, dev):
    """The dict a measurement returns: `result`'s tensors, and a new one for each that it lacks."""
    r = dict(result or {})
    rows = [("frame_f64", (B, 2), torch.float64), ("frame_i32", (B, 6), torch.int32)]
    if stitch_rows:
        rows += [("stitch_f64", (capacity, 7), torch.float64), ("stitch_i32", (capacity, 2), torch.int32)]
    for key, shape, dtype in rows:
        if key not in r:
            r[key] = torch.empty(shape, dtype=dtype, device=dev)
    return r


def _camera_index(who, cameras, B, n_cams, dev, same_device=True):
    """The camera of every frame -> int32 [B] on dev.  A device tensor is checked on the device, a host sequence is range-checked here.
    same_device=False: a device tensor's own device is not compared with dev (annotate never did)."""
    if isinstance(cameras, torch.Tensor) and cameras.is_cuda:
        if cameras.dtype != torch.int32 or tuple(cameras.shape) != (B,) or not cameras.is_contiguous() or (same_device and cameras.device != dev):
            raise ValueError(f"{who}: cameras must be a contiguous int32 [{B}] tensor on the outputs' device")
        return cameras
    host = np.asarray(cameras.numpy() if isinstance(cameras, torch.Tensor) else cameras)
    if host.shape != (B,) or host.dtype.kind not in "iu":
        raise ValueError(f"{who}: cameras must be {B} integers, one per frame")
    if B and (host.min() < 0 or host.max() >= n_cams):
        raise ValueError(f"{who}: camera index outside [0, {n_cams})")
    return torch.from_numpy(host.astype(np.int32)).to(dev)


@dataclasses.dataclass(frozen=True)
class _Family:
    """What differs between process_frame's calls (measure, annotate) and the stitch-distance checker's (measure_checker,
    annotate_checker): the settings struct, the pack call and the entry points of libvti.so."""
    ctype: type             # the ctypes settings struct
    params: str             # the name of its dataclass, for messages
    pack: str               # the Engine method that packs a camera table, and the call behind it
    pack_fn: str
    measure_method: str
    measure: tuple          # one settings struct, a camera table, a frame table, a frame table with ragged native rows
    annotate: tuple         # one settings struct (None: no such call), a camera table, a frame table, a frame table with ragged rows


_PROCESS_FRAME = _Family(VtiMeasureParams, "MeasureParams", "pack_cameras", "vti_measure_pack_cameras", "measure",
                         ("vti_measure", "vti_measure_cameras", "vti_measure_frames", "vti_measure_frames_native"),
                         (None, "vti_annotate", "vti_annotate_frames", "vti_annotate_frames_native"))
_CHECKER = _Family(VtiCheckerParams, "CheckerParams", "pack_checker_cameras", "vti_checker_pack_cameras", "measure_checker",
                   ("vti_measure_checker", "vti_measure_checker_cameras", "vti_measure_checker_frames", "vti_measure_checker_frames_native"),
                   ("vti_annotate_checker", "vti_annotate_checker_cameras", "vti_annotate_checker_frames",
                    "vti_annotate_checker_frames_native"))


class _Table:
    """What the packed tables share: `host` (the packed bytes, a CPU u8 tensor) and `dev` (their device copy).  A FrameTable and a
    WindowTable also name the entry points of their kind, so that one call path serves both."""

    def _ptrs(self):
        return C.c_void_p(self.host.data_ptr()), C.c_void_p(self.dev.data_ptr())

    def _row(self, b, extra=()):
        """Row b through the kind's vti_*_table_info: the letterbox row, then the ints named by `extra`, then the doubles."""
        i32, f64 = (C.c_int32 * (8 + len(extra)))(), (C.c_double * 5)()
        check(None, getattr(lib(), self._info)(C.c_void_p(self.host.data_ptr()), int(b), i32, f64))
        d = dict(zip(("H0", "W0", "new_h", "new_w", "top", "left"), (int(v) for v in i32[:6])))
        d["offset"] = (i32[6] & 0xFFFFFFFF) | (i32[7] << 32)
        d.update(zip(extra, (int(v) for v in i32[8:])))
        d.update(zip(("scale_x", "scale_y", "gain", "padx", "pady"), (float(v) for v in f64)))
        return d


class FrameTable(_Table):
    """A packed frame table (vti_pack_frames) for a batch whose frames differ in size: `host` (the packed bytes, a CPU u8 tensor)
    and `dev` (their device copy), `shapes` [(H0, W0)] per frame, the frames' `byte_offsets` in the flat frame buffer and its
    `total_bytes`, the canvas `H`, `W` it was packed for and the largest `max_H0`, `max_W0`."""

    def __init__(self, host, dev, shapes, byte_offsets, total_bytes, H, W):
        self.host, self.dev, self.shapes, self.byte_offsets, self.total_bytes = host, dev, shapes, byte_offsets, total_bytes
        self.H, self.W, self.B = H, W, len(shapes)
        self.max_H0, self.max_W0 = max(h for h, _ in shapes), max(w for _, w in shapes)

    _info, _letterbox, _scale_boxes = "vti_frame_table_info", "vti_letterbox_frames", "vti_scale_boxes_frames"
    _native_bytes, _masks_native, _predict_native = "vti_mask_native_frames_bytes", "vti_masks_native_frames", "vti_predict_frames_native"

    def row(self, b):
        """Host only: what row b holds -> dict(H0, W0, new_h, new_w, top, left, offset, scale_x, scale_y, gain, padx, pady)."""
        return self._row(b)


class WindowTable(_Table):
    """A packed window table (vti_pack_windows): one window (x0, y0, w, h) of each frame of a batch.  `host` / `dev` as a FrameTable's;
    `frames` is the FrameTable of the FULL frames on the same canvas (the frame buffer's layout, and what every consumer of the
    windowed outputs takes), `windows` [(x0, y0, w, h)] per frame."""

    def __init__(self, host, dev, frames, windows):
        self.host, self.dev, self.frames, self.windows = host, dev, frames, windows
        self.H, self.W, self.B = frames.H, frames.W, frames.B
        self.shapes, self.total_bytes = frames.shapes, frames.total_bytes

    _info, _letterbox, _scale_boxes = "vti_window_table_info", "vti_letterbox_windows", "vti_scale_boxes_windows"
    _native_bytes, _masks_native, _predict_native = "vti_mask_native_windows_bytes", "vti_masks_native_windows", "vti_predict_windows"

    def row(self, b):
        """Host only: what row b holds -> FrameTable.row's dict for the contiguous crop (H0, W0 are the window's h, w; offset is the
        byte of its first pixel), plus x0, y0 and the frame's frame_H0, frame_W0."""
        return self._row(b, ("x0", "y0", "frame_H0", "frame_W0"))


def check_window(window, H0, W0, who="window"):
    """(x0, y0, x1, y1), x1 and y1 exclusive, or None for the whole frame -> (x0, y0, w, h); a ValueError unless it is four integers
    with 0 <= x0 < x1 <= W0 and 0 <= y0 < y1 <= H0."""
    if window is None:
        return 0, 0, int(W0), int(H0)
    try:
        vals = list(window)
    except TypeError:
        vals = None
    if vals is None or len(vals) != 4 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) for v in vals):
        raise ValueError(f"{who} must be None or four integers (x0, y0, x1, y1), got {window!r}")
    x0, y0, x1, y1 = (int(v) for v in vals)
    if not (0 <= x0 < x1 <= W0 and 0 <= y0 < y1 <= H0):
        raise ValueError(f"{who} (x0, y0, x1, y1) = {(x0, y0, x1, y1)} does not lie inside its {H0}x{W0} frame with x0 < x1 and y0 < y1")
    return x0, y0, x1 - x0, y1 - y0


class RawTable(_Table):
    """A packed raw table (vti_pack_raw_frames) for raw camera frames that differ in size and / or format: `host` (the packed bytes,
    a CPU u8 tensor) and `dev` (their device copy), `shapes` [(H0, W0)] and `fmts` [VTI_RAW_*] per frame, the frames' `raw_offsets`
    in the flat raw buffer (multiples of 16), their `frame_bytes` and the buffer's `raw_bytes`."""

    def __init__(self, host, dev, shapes, fmts, raw_offsets, raw_bytes):
        self.host, self.dev, self.shapes, self.fmts, self.raw_offsets, self.raw_bytes = host, dev, shapes, fmts, raw_offsets, raw_bytes
        self.n = len(shapes)
        self.frame_bytes = [rawframes.frame_bytes(f, h, w) for f, (h, w) in zip(fmts, shapes)]


class StampTable:
    """A packed stamp table (vti_pack_stamps): `host` (the packed bytes, a CPU u8 tensor), `dev` (their device copy), `bits` (the
    device bit buffer, u32 as int32 [n_words]), the pictures' `shapes` [(H0, W0)] and the number of stamps `n_stamps`."""

    def __init__(self, host, dev, bits, n_words, shapes, n_stamps):
        self.host, self.dev, self.bits, self.n_words, self.shapes, self.n_stamps = host, dev, bits, n_words, shapes, n_stamps
        self.n = len(shapes)
        self.up_bytes = host.numel() + 4 * n_words      # what crossed to the device


@dataclasses.dataclass(frozen=True)
class NmsParams:
    """One row of an NMS table (include/vti.h vti_nms_params): the settings of Ultralytics' non_max_suppression for the frames that
    name the row.  classes: None for every class, or the class ids to keep (Ultralytics' `classes=`)."""
    conf: float = 0.25
    iou: float = 0.7
    max_det: int = 300
    agnostic: bool = False
    classes: tuple = None


class NmsTable:
    """A packed NMS table (vti_pack_nms_table): `host` (the packed bytes, a CPU u8 tensor), `dev` (their device copy), `n_rows`."""

    def __init__(self, host, dev, n_rows):
        self.host, self.dev, self.n_rows = host, dev, n_rows


class Engine:
    """One (model description, input size, max batch, dtype) context."""

    def __init__(self, scale="n", nc=80, nm=32, reg_max=16, H=640, W=640, max_batch=1, dtype="fp16"):
        self.scale, self.nc, self.nm, self.reg_max = scale, nc, nm, reg_max
        self.H, self.W, self.max_batch = H, W, max_batch
        self.dtype = _DTYPE_NAME[DTYPES[dtype]]
        self._ctx = C.c_void_p(0)
        desc = VtiDesc(scale.encode()[:1], nc, nm, reg_max, H, W, max_batch, DTYPES[dtype])
        rc = lib().vti_create(C.byref(desc), C.byref(self._ctx))
        if rc != 0:
            raise _lib.VtiError(rc, lib().vti_last_error(None).decode())
        self.device = None
        self._ws = None

    def __del__(self):
        try:
            if getattr(self, "_ctx", None) and self._ctx.value:
                lib().vti_destroy(self._ctx)
                self._ctx = C.c_void_p(0)
        except Exception:
            pass

    # ---- host-only plan introspection ------------------------------------------------
    def conv_table(self):
        out = []
        info = VtiConvInfo()
        for i in range(lib().vti_num_convs(self._ctx)):
            check(self._ctx, lib().vti_conv_at(self._ctx, i, C.byref(info)))
            out.append(dict(name=info.name.decode(), c1=info.c1, c2=info.c2, k=info.k, s=info.s, kind=info.kind,
                            h_in=info.h_in, w_in=info.w_in, h_out=info.h_out, w_out=info.w_out, macs=info.macs,
                            tile=(info.tile_h, info.tile_w), waves_n=info.waves_n, nrep=info.nrep, lds=info.lds_bytes,
                            fused=bool(info.fused), persistent=bool(info.persistent)))
        return out

    @property
    def num_anchors(self):
        return lib().vti_num_anchors(self._ctx)

    @property
    def fused_params(self):
        return lib().vti_fused_params(self._ctx)

    @property
    def macs_per_frame(self):
        return lib().vti_macs_per_frame(self._ctx)

    @property
    def workspace_bytes(self):
        return lib().vti_workspace_bytes(self._ctx)

    @property
    def num_launches(self):
        return lib().vti_num_launches(self._ctx)

    @property
    def no(self):
        return 4 + self.nc + self.nm

    @property
    def torch_dtype(self):
        return torch.float16 if self.dtype == "fp16" else torch.float32

    # ---- device setup ------------------------------------------------------------------
    def load_weights(self, blob, device=0):
        """blob: bytes of a VTIW1 container.  Uploads to `device` and allocates the workspace."""
        if not torch.cuda.is_available():
            raise RuntimeError("vti_amd needs a ROCm GPU: torch.cuda.is_available() is False (no CPU fallback)")
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        torch.cuda.set_device(dev)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        check(self._ctx, lib().vti_load_weights(self._ctx, buf, len(blob), dev.index or 0))
        self.device = dev
        self._ws = torch.empty(self.workspace_bytes + 256, dtype=torch.uint8, device=dev)
        base = self._ws.data_ptr()
        aligned = (base + 255) & ~255
        check(self._ctx, lib().vti_set_workspace(self._ctx, C.c_void_p(aligned), self.workspace_bytes))
        return self

    # ---- stages ------------------------------------------------------------------------
    def letterbox(self, frames, out=None):
        """frames: u8 [B,H0,W0,3] on device -> u8 [B,H,W,3]."""
        B, H0, W0, _ = frames.shape
        if out is None:
            out = torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device=frames.device)
        check(self._ctx, lib().vti_letterbox(self._ctx, _ptr(frames), B, H0, W0, _ptr(out), _stream()))
        return out

    # ---- batches whose frames differ in size (vti_pack_frames and the *_frames entry points) --------------------------------
    def pack_frames(self, shapes, device=None):
        """shapes: one (H0, W0) per frame.  Lays the frames out back to back, each at a multiple of 16 bytes, validates and packs the
        frame table for this engine's canvas and uploads it once.  -> (FrameTable, byte_offsets, total_bytes); a VtiError names the
        failing frame."""
        shapes = [(int(h), int(w)) for h, w in (tuple(x)[:2] for x in shapes)]
        B = len(shapes)
        if B < 1:
            raise ValueError("pack_frames: at least one frame")
        byte_offsets, total_bytes = [], 0
        for h, w in shapes:
            byte_offsets.append(total_bytes)
            total_bytes = (total_bytes + 3 * max(h, 0) * max(w, 0) + 15) & ~15
        total_bytes = max(total_bytes, 16)
        H0 = (C.c_int32 * B)(*[h for h, _ in shapes])
        W0 = (C.c_int32 * B)(*[w for _, w in shapes])
        off = (C.c_int64 * B)(*byte_offsets)
        nbytes = int(lib().vti_frame_table_bytes(B))
        host = torch.zeros(nbytes, dtype=torch.uint8)
        check(self._ctx, lib().vti_pack_frames(self._ctx, self.H, self.W, H0, W0, off, B, int(total_bytes),
                                               C.c_void_p(host.data_ptr()), nbytes))
        dev = host.to(device or self.device or "cuda")
        return FrameTable(host, dev, shapes, byte_offsets, int(total_bytes), self.H, self.W), byte_offsets, int(total_bytes)

    def _check_frames(self, table, B=None, buf=None):
        if not isinstance(table, FrameTable):
            raise ValueError("frames must be the FrameTable of Engine.pack_frames()")
        if (table.H, table.W) != (self.H, self.W):
            raise ValueError(f"the frame table was packed for a {table.H}x{table.W} canvas, this engine's is {self.H}x{self.W}")
        if B is not None and table.B != B:
            raise ValueError(f"the frame table describes {table.B} frames, the batch has {B}")
        if buf is not None:
            if buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() < table.total_bytes:
                raise ValueError(f"the frame buffer must be a flat contiguous uint8 tensor of >= {table.total_bytes} bytes")
            if buf.device != table.dev.device:
                raise ValueError("the frame buffer and the frame table must be on one device")

    def letterbox_frames(self, buf, table, out=None):
        """buf: flat u8 device buffer holding the frames of `table` (pack_frames) -> u8 [B,H,W,3]: vti_letterbox_frames."""
        self._check_frames(table, buf=buf)
        return self._letterbox_table(buf, table, out)

    def _letterbox_table(self, buf, table, out):
        """vti_letterbox_frames or vti_letterbox_windows, by the kind of `table` (checked by the caller)."""
        if out is None:
            out = torch.empty((table.B, self.H, self.W, 3), dtype=torch.uint8, device=buf.device)
        check(self._ctx, getattr(lib(), table._letterbox)(self._ctx, _ptr(buf), *table._ptrs(), table.B, _ptr(out), _stream()))
        return out

    # ---- predict on a window of each frame (vti_pack_windows and the *_windows entry points) ----------------------------------
    def pack_windows(self, shapes, windows, device=None):
        """shapes: one (H0, W0) per frame; windows: one (x0, y0, w, h) per frame.  Packs the FrameTable of the full frames
        (pack_frames: it fixes the frame buffer's layout) and the window table beside it, and uploads both.  -> WindowTable; a
        VtiError names the failing frame."""
        frames, byte_offsets, total_bytes = self.pack_frames(shapes, device)
        B = frames.B
        windows = [tuple(int(v) for v in w) for w in windows]
        if len(windows) != B or any(len(w) != 4 for w in windows):
            raise ValueError(f"pack_windows: one (x0, y0, w, h) per frame: {B} frames, got {windows!r}")
        H0 = (C.c_int32 * B)(*[h for h, _ in frames.shapes])
        W0 = (C.c_int32 * B)(*[w for _, w in frames.shapes])
        off = (C.c_int64 * B)(*byte_offsets)
        win = (C.c_int32 * (4 * B))(*[v for w in windows for v in w])
        nbytes = int(lib().vti_window_table_bytes(B))
        host = torch.zeros(nbytes, dtype=torch.uint8)
        check(self._ctx, lib().vti_pack_windows(self._ctx, self.H, self.W, H0, W0, off, win, B, int(total_bytes),
                                                C.c_void_p(host.data_ptr()), nbytes))
        return WindowTable(host, host.to(frames.dev.device), frames, windows)

    def _check_windows(self, table, B=None, buf=None):
        if not isinstance(table, WindowTable):
            raise ValueError("windows must be the WindowTable of Engine.pack_windows()")
        self._check_frames(table.frames, B=B, buf=buf)

    def letterbox_windows(self, buf, table, out=None):
        """buf: the flat u8 device buffer of the frames of `table` (pack_windows) -> u8 [B,H,W,3], the canvas of the contiguous crops
        read in place: vti_letterbox_windows."""
        self._check_windows(table, buf=buf)
        return self._letterbox_table(buf, table, out)

    def scale_boxes_windows(self, dets, counts, table, xyxy=None):
        """The boxes in FRAME px: scale_boxes(frames=the crops' table) plus the window's origin (vti_scale_boxes_windows)."""
        self._check_windows(table, B=dets.shape[0])
        return self._scale_boxes_table(dets, counts, table, xyxy)

    def mask_native_windows_bytes(self, table, max_det):
        """Host only: mask_native_frames_bytes of the full frames of `table`."""
        self._check_windows(table)
        return self._mask_native_table_bytes(table, max_det)

    def masks_native_windows(self, dets, counts, proto, table, mode="logit", masks=None, capacity_bytes=None, offsets=None,
                             mask_bases=None):
        """masks_native_frames' ragged buffer for the FULL frames of `table` (pack_windows), every instance's crop mask placed at its
        window's origin and zeros elsewhere (vti_masks_native_windows; the boxes are recomputed in window px from dets).  `masks`:
        a flat u8 buffer, by default mask_native_windows_bytes(table, max_det) bytes.  -> (masks, offsets, mask_bases)."""
        self._check_windows(table, B=dets.shape[0])
        return self._masks_native_table("masks_native_windows", table, dets, (counts, proto), mode, masks, capacity_bytes, offsets,
                                        mask_bases, lambda: self.mask_native_windows_bytes(table, dets.shape[1]))

    def predict_windows_into(self, buf, table, out, conf=0.25, iou=0.7, max_det=300, agnostic=False, swap_rb=True, mask_mode="logit",
                             nms=None):
        """predict_frames_into(native=True) on one window of each frame (vti_predict_windows): `buf` holds the full frames in the layout
        of table.frames, `out` comes from alloc_outputs(table.B, ..., native_frames=table.frames).  out["xyxy"] is in frame px and the
        ragged masks are frame-resolution rows with the window's mask at its place, so measure(frames=table.frames, native=True),
        annotate, overlay and mask_polygons_frames take `out` as they take predict_frames_into's.  nms: as predict_frames_into."""
        self._check_windows(table, B=out["counts"].shape[0] if isinstance(out, dict) and "counts" in out else None, buf=buf)
        self._check_ragged(out, table.frames, max_det, "predict_windows_into")
        if nms is not None:
            with self._nms_scope(nms):
                return self.predict_windows_into(buf, table, out, conf, iou, max_det, agnostic, swap_rb, mask_mode)
        return self._predict_table_native(buf, table, out, conf, iou, max_det, agnostic, swap_rb, mask_mode, "bits")

    def _predict_table_native(self, buf, table, out, conf, iou, max_det, agnostic, swap_rb, mask_mode, packing):
        """vti_predict_frames_native or vti_predict_windows, by the kind of `table`, into a ragged output set; the caller has checked
        both."""
        check(self._ctx, getattr(lib(), table._predict_native)(
            self._ctx, _ptr(buf), *table._ptrs(), table.B, int(bool(swap_rb)), float(conf), float(iou), int(max_det),
            int(bool(agnostic)), MASK_MODES[mask_mode], PACKINGS[packing], _ptr(out["input"]), _ptr(out["pred"]), _ptr(out["proto"]),
            _ptr(out["dets"]), _ptr(out["counts"]), _ptr(out["masks"]), out["masks"].numel(), _ptr(out["offsets"]),
            _ptr(out["mask_bases"]), _ptr(out["xyxy"]), _stream()))
        return out

    def predict_frames_into(self, buf, table, out, conf=0.25, iou=0.7, max_det=300, agnostic=False, swap_rb=True,
                            mask_mode="logit", packing="bits", native=False, nms=None):
        """predict_into for a batch whose frames differ in size: `buf` / `table` as letterbox_frames, `out` from
        alloc_outputs(table.B, ...).  Masks stay at the canvas size; out["xyxy"] is in each frame's own pixels.
        native=True (vti_predict_frames_native): frame-resolution masks in the ragged buffer of a set from
        alloc_outputs(..., native_frames=table) -- any other set is a ValueError before any call.
        nms=(NmsTable, rows): the call runs inside nms_table(table, rows)."""
        if native:
            self._check_ragged(out, table, max_det, "predict_frames_into")
        self._check_frames(table, B=out["counts"].shape[0], buf=buf)
        if nms is not None:
            with self._nms_scope(nms):
                return self.predict_frames_into(buf, table, out, conf, iou, max_det, agnostic, swap_rb, mask_mode, packing, native)
        if native:
            return self._predict_table_native(buf, table, out, conf, iou, max_det, agnostic, swap_rb, mask_mode, packing)
        check(self._ctx, lib().vti_predict_frames(
            self._ctx, _ptr(buf), *table._ptrs(), table.B, int(bool(swap_rb)), float(conf), float(iou), int(max_det),
            int(bool(agnostic)), MASK_MODES[mask_mode], PACKINGS[packing], _ptr(out["input"]), _ptr(out["pred"]), _ptr(out["proto"]),
            _ptr(out["dets"]), _ptr(out["counts"]), _ptr(out["masks"]), out["masks"].shape[0], _ptr(out["offsets"]), _ptr(out["xyxy"]),
            _stream()))
        return out

    def alloc_pred(self, B, device):
        """pred in Ultralytics' logical shape [B, 4+nc+nm, A] over the library's ANCHOR-MAJOR memory [B, A, 4+nc+nm]
        (each anchor's box, scores and coefficients are one contiguous row: that is how the head towers and NMS touch it)."""
        return torch.empty((B, self.num_anchors, self.no), dtype=torch.float32, device=device).transpose(1, 2)

    @staticmethod
    def _anchor_major(pred):
        """-> a tensor with pred's values whose memory is [B, A, no] contiguous (no copy for tensors from alloc_pred)."""
        pa = pred.transpose(1, 2)
        return pa if pa.is_contiguous() else pa.contiguous()

    def forward(self, inp, swap_rb=True, pred=None, proto=None, best=None):
        """inp: u8 [B,H,W,3] letterboxed -> pred f32 [B,4+nc+nm,A] (a view of anchor-major memory, see alloc_pred),
        proto T [B,H/4,W/4,nm] (NHWC).  best: optional f32 [B,A,2] that receives (best class score, its class) per anchor
        for nms(best=...) -- vti_forward_scored."""
        self._check_input(inp, (self.H, self.W))
        B = inp.shape[0]
        if pred is None:
            pred = self.alloc_pred(B, inp.device)
        elif not pred.transpose(1, 2).is_contiguous():
            raise ValueError("pred must come from Engine.alloc_pred / alloc_outputs (anchor-major memory)")
        if proto is None:
            proto = torch.empty((B, self.H // 4, self.W // 4, self.nm), dtype=self.torch_dtype, device=inp.device)
        if best is None:
            check(self._ctx, lib().vti_forward(self._ctx, _ptr(inp), B, int(bool(swap_rb)), _ptr(pred), _ptr(proto), _stream()))
        else:
            self._check_best(best, B)
            check(self._ctx, lib().vti_forward_scored(self._ctx, _ptr(inp), B, int(bool(swap_rb)), _ptr(pred), _ptr(proto), _ptr(best), _stream()))
        return pred, proto

    def alloc_best(self, B, device=None):
        return torch.empty((B, self.num_anchors, 2), dtype=torch.float32, device=device or self.device)

    def _check_best(self, best, B):
        if best.dtype != torch.float32 or tuple(best.shape) != (B, self.num_anchors, 2) or not best.is_contiguous():
            raise ValueError("best must be a contiguous f32 [B, A, 2] tensor (Engine.alloc_best)")

    def nms(self, pred, conf=0.25, iou=0.7, max_det=300, agnostic=False, dets=None, counts=None, best=None):
        """pred: [B, 4+nc+nm, A] (any layout; tensors from forward()/alloc_pred are used in place).  best: the pairs forward(best=...)
        wrote for THIS pred (vti_nms_scored: the candidate filter reads them instead of the class scores).  Inside nms_table() the
        settings of every frame come from its row of the table; conf, iou and agnostic are then ignored and max_det is the row
        stride of dets and the upper bound of the rows' limits."""
        pred = self._anchor_major(pred)
        B = pred.shape[0]
        if dets is None:
            dets = torch.empty((B, max_det, 6 + self.nm), dtype=torch.float32, device=pred.device)
        if counts is None:
            counts = torch.empty((B,), dtype=torch.int32, device=pred.device)
        if best is None:
            check(self._ctx, lib().vti_nms(self._ctx, _ptr(pred), B, float(conf), float(iou), int(max_det), int(bool(agnostic)),
                                           _ptr(dets), _ptr(counts), _stream()))
        else:
            self._check_best(best, B)
            check(self._ctx, lib().vti_nms_scored(self._ctx, _ptr(pred), _ptr(best), B, float(conf), float(iou), int(max_det),
                                                  int(bool(agnostic)), _ptr(dets), _ptr(counts), _stream()))
        return dets, counts

    # ---- NMS settings per frame and the `classes` filter (vti_pack_nms_table, vti_set_nms_table) --------------------------------
    def pack_nms_table(self, params_list, device=None):
        """One row per NmsParams of `params_list`, validated and packed by vti_pack_nms_table (a VtiError names the failing row and
        field) and uploaded once -> NmsTable for nms_table() and the nms= argument of predict_into / predict_frames_into."""
        rows = list(params_list)
        n = len(rows)
        if n < 1:
            raise ValueError("pack_nms_table: at least one row")
        keep = []           # the class lists stay alive until the call returns
        arr = (VtiNmsParams * n)()
        for k, p in enumerate(rows):
            cls = None if p.classes is None else [int(c) for c in p.classes]
            if cls is not None and not cls:
                raise ValueError(f"pack_nms_table: row {k}: an empty class set keeps nothing; pass classes=None for every class")
            ids = (C.c_int32 * len(cls))(*cls) if cls else None
            keep.append(ids)
            arr[k] = VtiNmsParams(float(p.conf), int(p.max_det), float(p.iou), int(bool(p.agnostic)), len(cls) if cls else 0,
                                  C.cast(ids, C.POINTER(C.c_int32)) if cls else None)
        nbytes = int(lib().vti_nms_table_bytes(n))
        if nbytes <= 0:
            raise ValueError(f"pack_nms_table: {n} rows are more than a table holds ({_lib.VTI_NMS_TABLE_MAX_ROWS})")
        host = torch.zeros(nbytes, dtype=torch.uint8)
        check(self._ctx, lib().vti_pack_nms_table(self._ctx, arr, n, C.c_void_p(host.data_ptr()), nbytes))
        return NmsTable(host, host.to(device or self.device or "cuda"), n)

    @contextlib.contextmanager
    def nms_table(self, table, rows=None):
        """While the block runs, every NMS of this engine (nms, predict_into, predict_frames_into) takes frame b's conf, iou,
        max_det, agnostic and class set from row rows[b] of `table` (pack_nms_table); rows=None: row 0 for every frame.  rows: host
        integers (range-checked here) or an int32 device tensor (checked by the kernel: a frame whose index is outside the table
        comes back with count 0), one per frame.  The calls' own conf, iou and agnostic are ignored meanwhile and their max_det is
        the row stride and the upper bound.  The table and the index stay referenced until the block ends, where the table is
        cleared (vti_set_nms_table)."""
        if not isinstance(table, NmsTable):
            raise ValueError("nms_table: table must be the NmsTable of Engine.pack_nms_table()")
        dev_rows = None
        if rows is not None:
            if isinstance(rows, torch.Tensor) and rows.is_cuda:
                if rows.dtype != torch.int32 or rows.dim() != 1 or not rows.is_contiguous() or rows.device != table.dev.device:
                    raise ValueError("nms_table: rows must be a contiguous int32 [B] tensor on the table's device")
                dev_rows = rows
            else:
                host = np.asarray(rows.numpy() if isinstance(rows, torch.Tensor) else rows)
                if host.ndim != 1 or host.dtype.kind not in "iu" or host.size > self.max_batch:
                    raise ValueError(f"nms_table: rows must be at most {self.max_batch} integers, one per frame")
                if host.size and (host.min() < 0 or host.max() >= table.n_rows):
                    raise ValueError(f"nms_table: row index outside [0, {table.n_rows})")
                dev_rows = torch.from_numpy(host.astype(np.int32)).to(table.dev.device)
            if dev_rows.numel() < self.max_batch:       # the library may be asked for any B up to max_batch
                dev_rows = torch.cat((dev_rows, dev_rows.new_zeros(self.max_batch - dev_rows.numel())))
        check(self._ctx, lib().vti_set_nms_table(self._ctx, C.c_void_p(table.host.data_ptr()), _ptr(table.dev), table.n_rows,
                                                 _ptr(dev_rows)))
        try:
            yield table
        finally:
            check(self._ctx, lib().vti_set_nms_table(self._ctx, None, None, 0, None))

    def _nms_scope(self, nms):
        """nms=(table, rows) of the predict forms -> the context that holds the table for the call; None: nothing to hold."""
        if nms is None:
            return contextlib.nullcontext()
        table, rows = nms
        return self.nms_table(table, rows)

    def masks(self, dets, counts, proto, mode="logit", packing="u8", capacity=None, masks=None, offsets=None):
        """-> (masks u8 [capacity,H,W] or [capacity,H,W/8], offsets i32 [B+1]).  With capacity=None the
        detection counts are read back first (one small D2H sync) to size the output exactly."""
        B, max_det = dets.shape[0], dets.shape[1]
        if capacity is None:
            capacity = int(counts.clamp(0, max_det).sum().item())
        wb = self.W if packing == "u8" else self.W // 8
        if masks is None:
            masks = torch.empty((capacity, self.H, wb), dtype=torch.uint8, device=dets.device)
        if offsets is None:
            offsets = torch.empty((B + 1,), dtype=torch.int32, device=dets.device)
        check(self._ctx, lib().vti_masks(self._ctx, _ptr(dets), _ptr(counts), _ptr(proto), B, max_det, MASK_MODES[mode],
                                         PACKINGS[packing], _ptr(masks) if capacity else C.c_void_p(0), capacity,
                                         _ptr(offsets), _stream()))
        return masks, offsets

    # ---- retina_masks: frame-resolution masks (process_mask_native) -------------------------
    def mask_native_layout(self, H0, W0, packing="bits"):
        """Host only: how masks_native lays out an H0 x W0 frame's masks -> dict(top, bottom, left, right, row_bytes,
        slot_bytes): the kept rows / columns of the prototype grid and the bytes per mask row and per slot."""
        out = (C.c_int32 * 6)()
        check(self._ctx, lib().vti_mask_native_layout(self._ctx, int(H0), int(W0), PACKINGS[packing], out))
        return dict(zip(("top", "bottom", "left", "right", "row_bytes", "slot_bytes"), (int(v) for v in out)))

    def masks_native(self, dets, counts, xyxy, proto, H0, W0, mode="logit", packing="bits", capacity=None, masks=None,
                     offsets=None):
        """Ultralytics process_mask_native (predict(retina_masks=True)): masks at the FRAME size from the frame-px boxes of
        scale_boxes() -> (masks u8 [capacity,H0,row_bytes] (bits: row_bytes = 8*ceil(W0/64); u8: W0), offsets i32 [B+1]).
        capacity=None reads the counts back first, as masks()."""
        B, max_det = dets.shape[0], dets.shape[1]
        if capacity is None:
            capacity = int(counts.clamp(0, max_det).sum().item())
        if masks is None:
            rb = self.mask_native_layout(H0, W0, packing)["row_bytes"]
            masks = torch.empty((capacity, H0, rb), dtype=torch.uint8, device=dets.device)
        if offsets is None:
            offsets = torch.empty((B + 1,), dtype=torch.int32, device=dets.device)
        check(self._ctx, lib().vti_masks_native(self._ctx, _ptr(dets), _ptr(xyxy), _ptr(counts), _ptr(proto), B, max_det, int(H0),
                                                int(W0), MASK_MODES[mode], PACKINGS[packing],
                                                _ptr(masks) if capacity else C.c_void_p(0), capacity, _ptr(offsets), _stream()))
        return masks, offsets

    # ---- retina_masks for frames of differing sizes: the ragged mask buffer (vti_masks_native_frames) ----------------------
    def mask_native_frames_bytes(self, table, max_det):
        """Host only: the bytes of max_det frame-resolution slots for every frame of `table` (the worst case of the ragged buffer)."""
        self._check_frames(table)
        return self._mask_native_table_bytes(table, max_det)

    def _mask_native_table_bytes(self, table, max_det):
        return int(getattr(lib(), table._native_bytes)(self._ctx, C.c_void_p(table.host.data_ptr()), int(max_det)))

    def _check_ragged(self, out, table, max_det, who):
        """`out` is a ragged output set (alloc_outputs(native_frames=)) made for the shapes of `table`."""
        if not isinstance(out, dict) or "mask_bases" not in out or out["masks"].dim() != 1:
            raise ValueError(f"{who}: native masks for frames of differing sizes need alloc_outputs(..., native_frames=table)")
        if isinstance(table, FrameTable) and out.get("native_shapes") != tuple(table.shapes):
            raise ValueError(f"{who}: the output set was allocated for other frame shapes than the table's")

    def masks_native_frames(self, dets, counts, xyxy, proto, table, mode="logit", masks=None, capacity_bytes=None, offsets=None,
                            mask_bases=None):
        """masks_native for a batch whose frames differ in size (xyxy from scale_boxes(frames=table)) -> (masks flat u8,
        offsets i32 [B+1], mask_bases i64 [B+1]): instance i of frame b is H0[b] rows of 8*ceil(W0[b]/64) bytes from byte
        mask_bases[b] + i * slot_bytes[b] on (frame_masks() cuts the views).  capacity_bytes=None: all of `masks`, or, when that is
        None too, the counts are read back first to size the buffer exactly."""
        self._check_frames(table, B=dets.shape[0])

        def exact_bytes():
            cnt = counts.clamp(0, dets.shape[1]).cpu().tolist()
            return sum(n * self.mask_native_layout(h, w)["slot_bytes"] for n, (h, w) in zip(cnt, table.shapes))
        return self._masks_native_table("masks_native_frames", table, dets, (xyxy, counts, proto), mode, masks, capacity_bytes, offsets,
                                        mask_bases, exact_bytes)

    def _masks_native_table(self, who, table, dets, inputs, mode, masks, capacity_bytes, offsets, mask_bases, default_bytes):
        """vti_masks_native_frames or vti_masks_native_windows, by the kind of `table` (checked by the caller).  inputs: the device
        tensors between dets and the table in the call; default_bytes(): the buffer's size when neither masks nor capacity_bytes says."""
        B, max_det = dets.shape[0], dets.shape[1]
        if masks is None:
            masks = torch.empty(int(default_bytes() if capacity_bytes is None else capacity_bytes), dtype=torch.uint8, device=dets.device)
        elif masks.dtype != torch.uint8 or masks.dim() != 1 or not masks.is_contiguous():
            raise ValueError(f"{who}: masks must be a flat contiguous uint8 tensor")
        if capacity_bytes is None:
            capacity_bytes = masks.numel()
        if not 0 <= int(capacity_bytes) <= masks.numel():
            raise ValueError(f"{who}: capacity_bytes must be in [0, {masks.numel()}]")
        if offsets is None:
            offsets = torch.empty((B + 1,), dtype=torch.int32, device=dets.device)
        if mask_bases is None:
            mask_bases = torch.empty((B + 1,), dtype=torch.int64, device=dets.device)
        check(self._ctx, getattr(lib(), table._masks_native)(
            self._ctx, _ptr(dets), *[_ptr(t) for t in inputs], *table._ptrs(), B, max_det, MASK_MODES[mode], PACKINGS["bits"],
            _ptr(masks) if int(capacity_bytes) else C.c_void_p(0), int(capacity_bytes), _ptr(offsets), _ptr(mask_bases), _stream()))
        return masks, offsets, mask_bases

    def frame_masks(self, masks, table, b, base, n):
        """The view u8 [n, H0[b], row_bytes[b]] of frame b's first n slots in a ragged buffer; `base` = mask_bases[b] (host int).
        n is cut to the slots that end inside the buffer."""
        H0, W0 = table.shapes[b]
        lay = self.mask_native_layout(H0, W0)
        n = max(0, min(int(n), (masks.numel() - int(base)) // lay["slot_bytes"]))
        return masks[int(base):int(base) + n * lay["slot_bytes"]].view(n, H0, lay["row_bytes"])

    def scale_boxes(self, dets, counts, H0=None, W0=None, xyxy=None, frames=None):
        """frames: a FrameTable (pack_frames) -- every frame is mapped back with its own gain, pads and bounds; else one H0 x W0."""
        B, max_det = dets.shape[0], dets.shape[1]
        if frames is not None:
            self._check_frames(frames, B=B)
            return self._scale_boxes_table(dets, counts, frames, xyxy)
        if xyxy is None:
            xyxy = torch.empty((B, max_det, 4), dtype=torch.float32, device=dets.device)
        check(self._ctx, lib().vti_scale_boxes(self._ctx, _ptr(dets), _ptr(counts), B, max_det, H0, W0, _ptr(xyxy), _stream()))
        return xyxy

    def _scale_boxes_table(self, dets, counts, table, xyxy):
        """vti_scale_boxes_frames or vti_scale_boxes_windows, by the kind of `table` (checked by the caller)."""
        B, max_det = dets.shape[0], dets.shape[1]
        if xyxy is None:
            xyxy = torch.empty((B, max_det, 4), dtype=torch.float32, device=dets.device)
        check(self._ctx, getattr(lib(), table._scale_boxes)(self._ctx, _ptr(dets), _ptr(counts), *table._ptrs(), B, max_det, _ptr(xyxy),
                                                            _stream()))
        return xyxy

    def alloc_outputs(self, B, max_det, capacity, packing="bits", device=None, native_hw=None, native_frames=None):
        """Preallocated output set for predict_into (the no-sync, graph-friendly form).  native_hw=(H0, W0): the masks are
        frame-resolution ones for predict_into(native=True) (mask_native_layout).  native_frames=FrameTable: the ragged set of
        predict_frames_into(native=True) -- `masks` is the flat u8 buffer of mask_native_frames_bytes(table, max_det) bytes and
        `mask_bases` i64 [B+1] comes with it; `capacity` is not used (the per-slot rows of measure() are B * max_det)."""
        dev = device or self.device
        if native_frames is not None:
            if native_hw is not None or packing != "bits":
                raise ValueError("alloc_outputs: native_frames excludes native_hw and is bit-packed only")
            self._check_frames(native_frames, B=B)
            nbytes = self.mask_native_frames_bytes(native_frames, max_det)
            if nbytes <= 0:
                raise ValueError("alloc_outputs: the frame table has no native mask layout for this engine")
            o = self.alloc_outputs(B, max_det, 0, "bits", dev)
            o["masks"] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            o["mask_bases"] = torch.empty((B + 1,), dtype=torch.int64, device=dev)
            o["native_shapes"] = tuple(native_frames.shapes)
            return o
        if native_hw is None:
            mh, wb = self.H, (self.W if packing == "u8" else self.W // 8)
        else:
            mh, wb = native_hw[0], self.mask_native_layout(native_hw[0], native_hw[1], packing)["row_bytes"]
        return dict(
            pred=self.alloc_pred(B, dev),
            proto=torch.empty((B, self.H // 4, self.W // 4, self.nm), dtype=self.torch_dtype, device=dev),
            dets=torch.empty((B, max_det, 6 + self.nm), dtype=torch.float32, device=dev),
            counts=torch.empty((B,), dtype=torch.int32, device=dev),
            masks=torch.empty((capacity, mh, wb), dtype=torch.uint8, device=dev),
            offsets=torch.empty((B + 1,), dtype=torch.int32, device=dev),
            xyxy=torch.empty((B, max_det, 4), dtype=torch.float32, device=dev),
            input=torch.empty((B, self.H, self.W, 3), dtype=torch.uint8, device=dev),
            best=self.alloc_best(B, dev),
        )

    def predict_into(self, frames, out, conf=0.25, iou=0.7, max_det=300, agnostic=False, swap_rb=True,
                     mask_mode="logit", packing="bits", native=False, nms=None):
        """Whole pipeline (letterbox -> net -> NMS -> masks -> scale_boxes) on the current stream with
        no host synchronisation; `out` from alloc_outputs().  native=True: scale_boxes -> frame-resolution masks
        (retina_masks; `out` from alloc_outputs(native_hw=(H0, W0))).  nms=(NmsTable, rows): the call runs inside
        nms_table(table, rows) -- per-frame NMS settings and the class filter."""
        if nms is not None:
            with self._nms_scope(nms):
                return self.predict_into(frames, out, conf, iou, max_det, agnostic, swap_rb, mask_mode, packing, native)
        B, H0, W0, _ = frames.shape
        capacity = out["masks"].shape[0]
        if native:
            rb = self.mask_native_layout(H0, W0, packing)["row_bytes"]
            if tuple(out["masks"].shape[1:]) != (H0, rb):
                raise ValueError(f"native masks for {H0}x{W0} frames need alloc_outputs(native_hw=({H0}, {W0}), packing={packing!r})")
        check(self._ctx, lib().vti_predict(
            self._ctx, _ptr(frames), B, H0, W0, int(bool(swap_rb)), float(conf), float(iou), int(max_det),
            int(bool(agnostic)), MASK_MODES[mask_mode] | (_lib.VTI_MASK_NATIVE if native else 0), PACKINGS[packing], _ptr(out["input"]), _ptr(out["pred"]),
            _ptr(out["proto"]), _ptr(out["dets"]), _ptr(out["counts"]), _ptr(out["masks"]), capacity,
            _ptr(out["offsets"]), _ptr(out["xyxy"]), _stream()))
        return out

    # ---- consumer-side reductions (measurement.py:70-86,160-185,300-330) ----------------
    def mask_to_frame(self, masks_u8, H0, W0):
        n, H, W = masks_u8.shape
        bitmaps = torch.empty((n, H0, W0), dtype=torch.uint8, device=masks_u8.device)
        nonzero = torch.empty((n,), dtype=torch.int32, device=masks_u8.device)
        check(self._ctx, lib().vti_mask_to_frame(self._ctx, _ptr(masks_u8), n, H, W, H0, W0, _ptr(bitmaps), _ptr(nonzero), _stream()))
        return bitmaps, nonzero

    def union_envelope(self, bitmaps, select):
        n, H0, W0 = bitmaps.shape
        sel = torch.as_tensor(select, dtype=torch.int32, device=bitmaps.device)
        uni = torch.empty((H0, W0), dtype=torch.uint8, device=bitmaps.device)
        env = torch.empty((W0,), dtype=torch.int32, device=bitmaps.device)
        check(self._ctx, lib().vti_union_envelope(self._ctx, _ptr(bitmaps), _ptr(sel), sel.numel(), H0, W0, _ptr(uni), _ptr(env), _stream()))
        return uni, env

    def mask_stats(self, bitmaps):
        n, H0, W0 = bitmaps.shape
        stats = torch.empty((n, 5), dtype=torch.int64, device=bitmaps.device)
        check(self._ctx, lib().vti_mask_stats(self._ctx, _ptr(bitmaps), n, H0, W0, _ptr(stats), _stream()))
        return stats

    # ---- the same reductions straight from bit-packed masks (no frame-sized bitmaps) ------
    def mask_stats_bits(self, masks_bits, H0, W0, stats=None, offsets=None):
        """masks_bits u8 [n,H,W/8] (VTI_PACK_BITS) -> i64 [n,5] = m00, m10, m01, min_col, max_col of each instance's
        H0 x W0 nearest-resized bitmap (measurement.py:70-86,302-318).  `offsets` (i32 [B+1] from masks()): slots at and
        beyond offsets[B] of a fixed-capacity buffer are skipped and report the empty mask."""
        n, H, wb = masks_bits.shape
        if stats is None:
            stats = torch.empty((n, 5), dtype=torch.int64, device=masks_bits.device)
        n_live = C.c_void_p(offsets.data_ptr() + 4 * (offsets.numel() - 1)) if offsets is not None else C.c_void_p(0)
        check(self._ctx, lib().vti_mask_stats_bits(self._ctx, _ptr(masks_bits), n, n_live, H, wb * 8, H0, W0, _ptr(stats), _stream()))
        return stats

    def envelope_bits(self, masks_bits, offsets, dets, cls, H0, W0, envelope=None):
        """Per frame: lower envelope i32 [B,W0] of the union of its instances of class `cls` (< 0: all)
        (measurement.py:160-185 on the bitmaps of measurement.py:70-86)."""
        B, max_det = dets.shape[0], dets.shape[1]
        if envelope is None:
            envelope = torch.empty((B, W0), dtype=torch.int32, device=dets.device)
        check(self._ctx, lib().vti_envelope_bits(self._ctx, _ptr(masks_bits), _ptr(offsets), _ptr(dets), B, max_det,
                                                 masks_bits.shape[0], int(cls), H0, W0, _ptr(envelope), _stream()))
        return envelope

    # ---- process_frame's measurement record (measurement.py:240-510) -------------------------------
    def measure_scratch_bytes(self, B, capacity, W0):
        return int(lib().vti_measure_scratch_bytes(self._ctx, int(B), int(capacity), int(W0)))

    def pack_cameras(self, params_list, device=None):
        """The camera table of vti_measure_cameras: one row per measure.MeasureParams (or VtiMeasureParams) of `params_list`, validated
        and packed by vti_measure_pack_cameras (a VtiError names the failing index) and uploaded once.  -> u8 device tensor to pass as
        measure(..., params=table, cameras=...); row k is camera k."""
        return self._pack_cameras(_PROCESS_FRAME, params_list, device)

    def pack_checker_cameras(self, params_list, device=None):
        """The camera table of the checker's rig calls: one row per measure.CheckerParams (or VtiCheckerParams) of `params_list`,
        validated and packed by vti_checker_pack_cameras (a VtiError names the failing index) and uploaded once.  -> u8 device tensor
        to pass as measure_checker(..., params=table, cameras=...) and annotate_checker(...); row k is camera k.  Its rows are not
        pack_cameras()' rows."""
        return self._pack_cameras(_CHECKER, params_list, device)

    def _pack_cameras(self, fam, params_list, device):
        cps = [p.to_c() if hasattr(p, "to_c") else p for p in params_list]
        n = len(cps)
        if n < 1:
            raise ValueError(f"{fam.pack}: at least one camera")
        arr = (fam.ctype * n)(*cps)
        nbytes = int(lib().vti_measure_cameras_bytes(n))
        host = torch.empty(nbytes, dtype=torch.uint8)
        check(self._ctx, getattr(lib(), fam.pack_fn)(self._ctx, arr, n, C.c_void_p(host.data_ptr()), nbytes))
        return host.to(device or self.device or "cuda")

    def _camera_table(self, fam, who, params, dev):
        """One settings object of the family, a list of them or the table of its pack call -> (table, n_cams)."""
        if not isinstance(params, (list, tuple, torch.Tensor)):
            params = [params]
        table = params if isinstance(params, torch.Tensor) else self._pack_cameras(fam, params, dev)
        row = int(lib().vti_measure_cameras_bytes(1))
        if table.dtype != torch.uint8 or table.dim() != 1 or table.numel() < row or table.numel() % row or table.device != dev:
            raise ValueError(f"{who}: params must be {fam.params} or the u8 table of {fam.pack}() on the outputs' device")
        return table, table.numel() // row

    def _scratch(self, attr, need, dev):
        """The scratch kept as self.<attr>: at least `need` bytes on dev, reallocated only when it is too small or elsewhere."""
        ws = getattr(self, attr, None)
        if ws is None or ws.numel() < need or ws.device != dev:
            setattr(self, attr, None)
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            setattr(self, attr, ws)
        return ws

    def measure(self, out, params, H0=None, W0=None, native=False, stitch_rows=True, result=None, cameras=None, frames=None):
        """The per-frame measurement of measurement.py's process_frame for every frame of an alloc_outputs() set that predict_into()
        (or nms/masks/scale_boxes) filled: vti_measure.  params: a measure.MeasureParams (or a VtiMeasureParams).  native=True: the
        masks are frame-size rows (predict_into(native=True)).  Returns device tensors, no host synchronisation:
        dict(frame_f64 [B,2] avg_dist_mm, avg_width_mm (NaN = None), frame_i32 [B,6] status, n_stitch, n_fabric, n_selected, n_dist,
        n_width, and with stitch_rows the per-slot stitch_f64 [capacity,7], stitch_i32 [capacity,2]).  `result`: the same dict
        preallocated (any of its tensors reused).
        cameras (vti_measure_cameras): the camera of every frame, an int32 device tensor [B] (checked on the device: a frame whose
        index is outside the table reports status VTI_MEASURE_BAD_CAMERA) or a host sequence (range-checked here, ValueError); then
        `params` is the table of pack_cameras() or a list of MeasureParams (packed and uploaded on every call: pack once instead).
        frames (vti_measure_frames): a FrameTable (pack_frames) in place of H0, W0 -- frame b is measured at its own size; letterbox
        bit masks, or with native=True the ragged frame-size rows of a set from alloc_outputs(native_frames=) that
        predict_frames_into(native=True) filled (vti_measure_frames_native; native=True with any other set is a ValueError).
        Without `cameras` the one `params` serves every frame."""
        return self._measure(_PROCESS_FRAME, "measure", out, params, H0, W0, native, stitch_rows, result, cameras, frames)

    def measure_checker(self, out, params, H0=None, W0=None, native=False, stitch_rows=True, result=None, cameras=None, frames=None):
        """The stitch-distance checker's per-frame measurement (Utils/check_stitch_distance.py:281-553) for every frame of an output
        set, as measure() does process_frame's: vti_measure_checker.  params: a measure.CheckerParams (or a VtiCheckerParams);
        native, stitch_rows, result and the returned dict of device tensors are measure()'s, with the checker's meanings
        (include/vti.h): the upper fabric edge, the signed proximity test, widths for the final set only.
        cameras (vti_measure_checker_cameras): the camera of every frame, an int32 device tensor [B] (checked on the device: a frame
        whose index is outside the table reports VTI_MEASURE_BAD_CAMERA) or a host sequence (range-checked here, ValueError); then
        `params` is the table of pack_checker_cameras() or a list of CheckerParams (packed and uploaded on every call: pack once
        instead).  frames (vti_measure_checker_frames): a FrameTable in place of H0, W0 -- frame b is measured at its own size;
        letterbox bit masks, or with native=True the ragged rows of a set from alloc_outputs(native_frames=)
        (vti_measure_checker_frames_native; the set needs mask_bases).  Without `cameras` the one `params` serves every frame."""
        return self._measure(_CHECKER, "measure_checker", out, params, H0, W0, native, stitch_rows, result, cameras, frames)

    def _measure(self, fam, who, out, params, H0, W0, native, stitch_rows, result, cameras, frames):
        """measure() and measure_checker(): fam's four calls on the arguments both take."""
        one, with_cameras, with_frames, with_ragged = (getattr(lib(), name) for name in fam.measure)
        dets, masks = out["dets"], out["masks"]
        B, max_det, capacity = out["counts"].shape[0], dets.shape[1], masks.shape[0]
        dev = dets.device
        ragged = frames is not None and native and "mask_bases" in out
        if frames is not None:
            self._check_frames(frames, B=B)
            if native and not ragged:
                raise ValueError(f"{who}: frames of differing sizes have letterbox masks only (native=True needs one frame size, "
                                 "or the ragged set of alloc_outputs(native_frames=) with its mask_bases)")
            if ragged:
                self._check_ragged(out, frames, max_det, who)
                if not (dets.is_cuda and masks.is_cuda and out["mask_bases"].is_cuda):
                    raise ValueError(f"{who}: the output set must be in device memory")
                capacity = B * max_det
            if H0 is not None or W0 is not None:
                raise ValueError(f"{who}: give H0, W0 or frames, not both")
            H0, W0 = frames.max_H0, frames.max_W0
            if cameras is None:
                cameras = [0] * B
        elif H0 is None or W0 is None:
            raise ValueError(f"{who}: H0 and W0 (or frames=) are required")
        if cameras is not None:
            if isinstance(params, (list, tuple)) and not isinstance(cameras, torch.Tensor):
                cameras = _camera_index(who, cameras, B, len(params), "cpu")       # before anything is packed
            table, n_cams = self._camera_table(fam, who, params, dev)
            cameras = _camera_index(who, cameras, B, n_cams, dev)
        else:
            cp = params.to_c() if hasattr(params, "to_c") else params
        r = _measure_result(result, B, capacity, stitch_rows, dev)
        ws = self._scratch("_measure_ws", max(self.measure_scratch_bytes(B, capacity, W0), 256), dev)
        head = (_ptr(masks) if capacity else C.c_void_p(0), int(bool(native)), _ptr(dets), _ptr(out["xyxy"]), _ptr(out["counts"]),
                _ptr(out["offsets"]))
        tail = (_ptr(ws), ws.numel(), _ptr(r["frame_f64"]), _ptr(r["frame_i32"]), _ptr(r.get("stitch_f64")), _ptr(r.get("stitch_i32")),
                _stream())
        rest = head + (B, max_det, capacity, int(H0), int(W0)) + tail
        if ragged:
            check(self._ctx, with_ragged(self._ctx, _ptr(table), n_cams, _ptr(cameras), _ptr(masks), _ptr(out["mask_bases"]), masks.numel(),
                                         *head[2:], *frames._ptrs(), B, max_det, capacity, *tail))
        elif frames is not None:
            check(self._ctx, with_frames(self._ctx, _ptr(table), n_cams, _ptr(cameras), *head, *frames._ptrs(), B, max_det, capacity, *tail))
        elif cameras is not None:
            check(self._ctx, with_cameras(self._ctx, _ptr(table), n_cams, _ptr(cameras), *rest))
        else:
            check(self._ctx, one(self._ctx, C.byref(cp), *rest))
        return r

    # ---- process_frame's annotated frame (measurement.py:219-504): the overlay on a selection of the batch ------------------
    def annotate_scratch_bytes(self, n_sel, max_det, H0, W0, max_points):
        return int(lib().vti_annotate_scratch_bytes(self._ctx, int(n_sel), int(max_det), int(H0), int(W0), int(max_points)))

    def annotate(self, frames, out, meas, params_or_table, select, cameras=None, native=False, result=None, max_points=16384,
                 table=None, capacity_bytes=None):
        """The frames `select` of the batch with the reference's overlay drawn on them: vti_annotate, byte for byte
        annotate.rasterise(frame, annotate.display_list(...)).  frames: the contiguous uint8 [B,H0,W0,3] BGR device batch predict
        consumed; out: its output set; meas: measure(..., stitch_rows=True)'s dict on the same set; params_or_table: the
        MeasureParams of that measure call, a list of them, or the table of pack_cameras(); cameras: as measure() took them (None:
        the first row serves every frame); select: host integers in [0, B), any order, duplicates allowed (ValueError otherwise).
        max_points: room for the fabric outline's vertices per frame.  Returns device tensors, no host synchronisation:
        dict(frames=u8 [n_sel,H0,W0,3], status=i32 [n_sel]: VTI_ANNOTATE_OUTLINE_SKIPPED where the outline did not fit).  `result`: the
        same dict preallocated.  Text is the host's: annotate.text_items / put_text.
        table (vti_annotate_frames): the FrameTable of a batch whose frames differ in size; `frames` is then the flat u8 device buffer
        the table describes (what predict consumed, or DecodedFrames.buf) and frame select[k] is drawn at its own size.  Returns
        dict(buf=u8 flat, table=the FrameTable of the selection (pack_frames of its shapes; the 16 latest tuples of shapes are kept), shapes,
        byte_offsets, status): picture k is buf[byte_offsets[k]:][:3 * H0 * W0].view(H0, W0, 3), and (buf, table) is what
        encode_jpeg(..., table=) and predict_frames_into take.  `result` may preallocate buf and status.  Letterbox masks, or with
        native=True (vti_annotate_frames_native) the ragged frame-size rows of a set from alloc_outputs(native_frames=) that
        predict_frames_into(native=True) or predict_windows_into filled and measure(frames=table, native=True) measured; native=True
        with any other set is a ValueError.  capacity_bytes (ragged sets only; default: all of out["masks"]): a slot that ends beyond
        it is an empty mask, as measure() saw it; the slot indices are cut by the rows of meas["stitch_i32"]."""
        return self._annotate(_PROCESS_FRAME, "annotate", frames, out, meas, params_or_table, select, cameras, native, result, max_points, table,
                              capacity_bytes)

    # ---- the stitch-distance checker's picture (Utils/check_stitch_distance.py:293-545): vti_annotate_checker ------------------
    def annotate_checker(self, frames, out, meas, params, select, native=False, result=None, max_points=16384, cameras=None,
                         table=None, capacity_bytes=None):
        """The frames `select` of the batch with the stitch-distance checker's picture drawn on them: vti_annotate_checker, byte for
        byte annotate.rasterise(frame, annotate.checker_display_list(...)).  frames, out, select, native, result, max_points and the
        returned dict(frames=u8 [n_sel,H0,W0,3], status=i32 [n_sel]) of device tensors are annotate()'s uniform form (the frames feed
        encode_jpeg as they are); meas: measure_checker(..., stitch_rows=True)'s dict on the same set; params: the CheckerParams (or
        VtiCheckerParams) of that call.  Text is the host's: measure.checker_text_items / put_text.
        cameras (vti_annotate_checker_cameras): as measure_checker() took them; params is then a list of CheckerParams or the table
        of pack_checker_cameras().  table (vti_annotate_checker_frames): the FrameTable of a batch whose frames differ in size;
        `frames` is then the flat u8 device buffer it describes, and the call returns dict(buf, table, shapes, byte_offsets, status)
        as annotate(table=) does: it feeds encode_jpeg(table=) and stamp(table=) unchanged.  With table=: letterbox masks, or with
        native=True (vti_annotate_checker_frames_native) the ragged rows of a set from alloc_outputs(native_frames=) that
        measure_checker(frames=table, native=True) measured; capacity_bytes as annotate() takes it."""
        return self._annotate(_CHECKER, "annotate_checker", frames, out, meas, params, select, cameras, native, result, max_points, table,
                              capacity_bytes)

    def _annotate(self, fam, who, frames, out, meas, params, select, cameras, native, result, max_points, table, capacity_bytes=None):
        """annotate() and annotate_checker(): fam's calls on the arguments both take.  Only the checker has a call that takes one
        settings struct; process_frame's picture always goes through a camera table."""
        one, with_cameras, with_frames, with_ragged = (name and getattr(lib(), name) for name in fam.annotate)
        ragged = table is not None and bool(native)
        if table is not None:
            self._check_frames(table)
            if ragged and not (isinstance(out, dict) and "mask_bases" in out and out["masks"].dim() == 1):
                raise ValueError(f"{who}: frames of differing sizes have letterbox masks only (native=True needs one frame size, "
                                 "or the ragged set of alloc_outputs(native_frames=) with its mask_bases)")
            if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 1:
                raise ValueError(f"{who}: with table=, frames must be the flat uint8 frame buffer")
            B, H0, W0 = table.B, None, None
        else:
            B, H0, W0 = _uniform_frames(who, frames)
        dets, masks = out["dets"], out["masks"]
        dev = dets.device
        if out["counts"].shape[0] != B:
            raise ValueError(f"{who}: {B} frames but an output set of {out['counts'].shape[0]}")
        max_det, capacity = dets.shape[1], masks.shape[0]
        sel = _select(who, select, B)
        n_sel = int(sel.size)
        for key in ("frame_i32", "stitch_f64", "stitch_i32"):
            if meas.get(key) is None:
                raise ValueError(f"{who}: meas needs {key} ({fam.measure_method}(..., stitch_rows=True))")
        if ragged:
            self._check_ragged(out, table, max_det, who)
            bases = out["mask_bases"]
            if masks.dtype != torch.uint8 or not masks.is_contiguous() or bases.dtype != torch.int64 or tuple(bases.shape) != (B + 1,) \
                    or not bases.is_contiguous():
                raise ValueError(f"{who}: the ragged set is the flat uint8 buffer of masks_native_frames with its int64 [{B + 1}] mask_bases")
            if capacity_bytes is None:
                capacity_bytes = masks.numel()
            if isinstance(capacity_bytes, bool) or not isinstance(capacity_bytes, (int, np.integer)) \
                    or not 0 <= int(capacity_bytes) <= masks.numel():
                raise ValueError(f"{who}: capacity_bytes must be an integer in [0, {masks.numel()}]")
            capacity = int(meas["stitch_i32"].shape[0])                 # slot indices: the per-slot rows measure() wrote, not bytes
            if meas["stitch_f64"].shape[0] < capacity:
                raise ValueError(f"{who}: meas has {capacity} rows of stitch_i32 but fewer of stitch_f64")
        elif capacity_bytes is not None:
            raise ValueError(f"{who}: capacity_bytes belongs to table= with native=True (the ragged frame-size rows)")
        rig = one is None or cameras is not None or table is not None or isinstance(params, (list, tuple, torch.Tensor))
        if rig and isinstance(params, (list, tuple)) and cameras is not None and not isinstance(cameras, torch.Tensor):
            cameras = _camera_index(who, cameras, B, len(params), "cpu")
        # everything above is about shapes and values; what needs a device comes from here on
        if not frames.is_cuda or not frames.is_contiguous():
            raise ValueError(f"{who}: frames must be the contiguous device batch predict consumed")
        if rig:
            table_c, n_cams = self._camera_table(fam, who, params, dev)
            if cameras is not None:
                cameras = _camera_index(who, cameras, B, n_cams, dev, same_device=False)
        else:
            cp = params.to_c() if hasattr(params, "to_c") else params
        r = dict(result or {})
        if "status" not in r:
            r["status"] = torch.empty((n_sel,), dtype=torch.int32, device=dev)
        if table is not None:
            self._check_frames(table, buf=frames)
            if ragged and not (masks.is_cuda and out["mask_bases"].device == dev):
                raise ValueError(f"{who}: the output set must be in device memory")
            shapes = tuple(table.shapes[int(b)] for b in sel)
            out_table = self._out_table(shapes, dev)                     # the 16 latest selections are kept
            self._selection_out(r, out_table, shapes, dev)
            need = int(lib().vti_annotate_frames_scratch_bytes(self._ctx, C.c_void_p(out_table.host.data_ptr()), max_det, int(max_points)))
            if need <= 0:
                raise ValueError(f"{who}: unsupported geometry (n_sel={n_sel}, max_det={max_det}, frames up to "
                                 f"{out_table.max_H0}x{out_table.max_W0}, max_points={max_points}; a drawn frame is at most 8192 x 8192)")
        else:
            if "frames" not in r:
                r["frames"] = torch.empty((n_sel, H0, W0, 3), dtype=torch.uint8, device=dev)
            need = self.annotate_scratch_bytes(n_sel, max_det, H0, W0, max_points)
            if need <= 0:
                raise ValueError(f"{who}: unsupported geometry (n_sel={n_sel}, max_det={max_det}, {H0}x{W0}, max_points={max_points})")
        ws = self._scratch("_annotate_ws", need, dev)
        dev_sel = torch.from_numpy(sel).to(dev)
        mid = (_ptr(dets), _ptr(out["xyxy"]), _ptr(out["counts"]), _ptr(out["offsets"]), max_det, capacity, _ptr(meas["frame_i32"]),
               _ptr(meas["stitch_f64"]), _ptr(meas["stitch_i32"]), C.c_void_p(sel.ctypes.data), _ptr(dev_sel), n_sel, int(max_points))
        pm = _ptr(masks) if capacity else C.c_void_p(0)
        if ragged:
            check(self._ctx, with_ragged(self._ctx, _ptr(frames), *table._ptrs(), B, _ptr(table_c), n_cams, _ptr(cameras),
                                         _ptr(masks) if int(capacity_bytes) else C.c_void_p(0), _ptr(out["mask_bases"]), int(capacity_bytes),
                                         *mid, *out_table._ptrs(), _ptr(r["buf"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
        elif table is not None:
            check(self._ctx, with_frames(self._ctx, _ptr(frames), *table._ptrs(), B, _ptr(table_c), n_cams, _ptr(cameras), pm, 0, *mid,
                                         *out_table._ptrs(), _ptr(r["buf"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
        elif rig:
            check(self._ctx, with_cameras(self._ctx, _ptr(frames), B, H0, W0, _ptr(table_c), n_cams, _ptr(cameras), pm, int(bool(native)),
                                          *mid, _ptr(r["frames"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
        else:
            check(self._ctx, one(self._ctx, _ptr(frames), B, H0, W0, C.byref(cp), pm, int(bool(native)), *mid,
                                 _ptr(r["frames"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
        return r

    # ---- the model-check viewer's picture (Utils/check_model.py:155-256): vti_overlay ------------------------------------------
    def overlay_scratch_bytes(self, n_sel, max_det, H0, W0, max_points):
        return int(lib().vti_overlay_scratch_bytes(self._ctx, int(n_sel), int(max_det), int(H0), int(W0), int(max_points)))

    def _out_table(self, shapes, dev):
        """The FrameTable of a selection's pictures (pack_frames of its shapes): the 16 latest tuples of shapes are kept, per device."""
        cache = self.__dict__.setdefault("_out_tables", {})              # (shapes, device) -> FrameTable
        out_table = cache.pop((shapes, str(dev)), None)
        if out_table is None:
            out_table = self.pack_frames(shapes, dev)[0]
            while len(cache) >= 16:
                del cache[next(iter(cache))]
        cache[(shapes, str(dev))] = out_table                           # (re)inserted last: the oldest entry is the first
        return out_table

    def _selection_out(self, r, out_table, shapes, dev):
        """What a drawing call with table= returns besides status, put into r: the selection's out table, `buf` for its pictures (r's
        own if it has one), shapes and byte_offsets."""
        if "buf" not in r:
            r["buf"] = torch.empty(out_table.total_bytes, dtype=torch.uint8, device=dev)
        self._check_frames(out_table, buf=r["buf"])
        r.update(table=out_table, shapes=list(shapes), byte_offsets=list(out_table.byte_offsets))

    def overlay(self, frames, out, select, native=False, plates=None, mode="both", annotated=None, alpha=0.30, beta=0.70,
                palette=_ov.PALETTE, max_points=16384, result=None, table=None, mask_bases=None, capacity_bytes=None):
        """The frames `select` of the batch as check_model.py's annotate_result shows them (without the label text): vti_overlay,
        byte for byte overlay.render(...).  frames: the contiguous uint8 [B,H0,W0,3] BGR device batch predict consumed; out: its
        output set; select: host integers in [0, B), any order, duplicates allowed (ValueError otherwise); native: the masks are
        frame-size rows (retina_masks).  plates: None, or a contiguous int32 [capacity,4] device tensor (xa, ya, xb, yb) per mask slot
        (overlay.plates).  mode: "draw" (contours, boxes, plates), "blend" (the tinted frame blended with `annotated`, a contiguous
        uint8 [n_sel,H0,W0,3] device tensor, which may be result["frames"] itself) or "both" ("blend" applied to "draw"'s picture).
        palette: BGR triplets, 1..16 (overlay.PALETTE).  max_points: room for the contour vertices of one frame.  Returns device
        tensors, no host synchronisation: dict(frames=u8 [n_sel,H0,W0,3], status=i32 [n_sel]: VTI_OVERLAY_OUTLINE_SKIPPED where the
        contours did not fit); "frames" feeds encode_jpeg unchanged.  `result`: the same dict preallocated.  The scratch is kept per
        (n_sel, H0, W0).
        table (vti_overlay_frames): the FrameTable of a batch whose frames differ in size; `frames` is then the flat u8 device buffer
        the table describes (what predict_frames_into consumed) and frame select[k] is drawn at its own size.  Returns dict(buf=u8
        flat, table=the FrameTable of the selection (the 16 latest are kept), shapes, byte_offsets, status) as annotate(table=) does:
        picture k is buf[byte_offsets[k]:][:3 * H0 * W0].view(H0, W0, 3), and (buf, table) is what encode_jpeg(..., table=) takes.
        annotated: a flat u8 buffer of the out table's size (e.g. "draw"'s buf with text put on it; it may be result["buf"] itself).
        native=True: the masks are the ragged rows of a set from alloc_outputs(native_frames=) (masks_native_frames); mask_bases and
        capacity_bytes default to out["mask_bases"] and the whole of out["masks"], and plates are then int32 [B * max_det, 4] per
        slot index.  `result` may preallocate buf and status."""
        if table is not None:
            self._check_frames(table)
            if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 1:
                raise ValueError("overlay: with table=, frames must be the flat uint8 frame buffer")
            B, H0, W0 = table.B, None, None
        else:
            if mask_bases is not None or capacity_bytes is not None:
                raise ValueError("overlay: mask_bases and capacity_bytes belong to table= (frames of differing sizes)")
            B, H0, W0 = _uniform_frames("overlay", frames)
        dets, masks = out["dets"], out["masks"]
        dev = dets.device
        if out["counts"].shape[0] != B:
            raise ValueError(f"overlay: {B} frames but an output set of {out['counts'].shape[0]}")
        max_det, capacity = dets.shape[1], masks.shape[0]
        ragged = table is not None and bool(native)
        sel = _select("overlay", select, B)
        n_sel = int(sel.size)
        mode_i = _ov.MODES.get(mode, mode) if isinstance(mode, str) else mode
        if mode_i not in (_ov.DRAW, _ov.BLEND, _ov.BOTH):
            raise ValueError(f"overlay: mode must be 'draw', 'blend' or 'both', got {mode!r}")
        if (annotated is not None) != (mode_i == _ov.BLEND):
            raise ValueError("overlay: annotated is the picture mode='blend' blends with (and only that mode takes one)")
        pal = np.ascontiguousarray(palette, dtype=np.uint8)
        if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 16:
            raise ValueError("overlay: palette must be 1 .. 16 BGR triplets")
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError("overlay: alpha and beta must be finite")
        if ragged:
            if mask_bases is None:
                mask_bases = out.get("mask_bases")
            if masks.dtype != torch.uint8 or masks.dim() != 1 or not masks.is_contiguous() or not isinstance(mask_bases, torch.Tensor) \
                    or mask_bases.dtype != torch.int64 or tuple(mask_bases.shape) != (B + 1,) or not mask_bases.is_contiguous():
                raise ValueError("overlay: native masks for frames of differing sizes are the flat uint8 buffer of masks_native_frames "
                                 f"with its int64 [{B + 1}] mask_bases (alloc_outputs(..., native_frames=table))")
            if capacity_bytes is None:
                capacity_bytes = masks.numel()
            if not 0 <= int(capacity_bytes) <= masks.numel():
                raise ValueError(f"overlay: capacity_bytes must be in [0, {masks.numel()}]")
            capacity = B * max_det                                      # slot indices: the per-slot rows (plates) are B * max_det
        else:
            if mask_bases is not None or capacity_bytes is not None:
                raise ValueError("overlay: mask_bases and capacity_bytes belong to native=True (the ragged frame-size rows)")
            if capacity:
                want = (H0, 8 * -(-W0 // 64)) if native else (self.H, self.W // 8)
                if masks.dtype != torch.uint8 or masks.dim() != 3 or tuple(masks.shape[1:]) != want:
                    raise ValueError(f"overlay: masks must be uint8 [capacity, {want[0]}, {want[1]}] ({'frame-size rows' if native else 'letterbox bits'})")
        if table is not None:
            shapes = tuple(table.shapes[int(b)] for b in sel)
            out_bytes = sum(-(-3 * h * w // 16) * 16 for h, w in shapes)     # pack_frames: every picture starts at a multiple of 16
            if annotated is not None and not (isinstance(annotated, torch.Tensor) and annotated.dtype == torch.uint8 and annotated.dim() == 1
                                              and annotated.numel() == out_bytes):
                raise ValueError(f"overlay: with table=, annotated must be a flat uint8 buffer of the out table's {out_bytes} bytes")
        # everything above is about shapes and values; what needs a device comes from here on
        if not frames.is_cuda or not frames.is_contiguous():
            raise ValueError("overlay: frames must be the contiguous device batch predict consumed")
        if plates is not None and not (isinstance(plates, torch.Tensor) and plates.dtype == torch.int32 and plates.is_contiguous()
                                       and tuple(plates.shape) == (capacity, 4) and plates.device == dev):
            raise ValueError(f"overlay: plates must be a contiguous int32 [{capacity},4] tensor on the outputs' device")
        r = dict(result or {})
        if "status" not in r:
            r["status"] = torch.empty((n_sel,), dtype=torch.int32, device=dev)
        if table is not None:
            self._check_frames(table, buf=frames)
            if ragged and not (masks.is_cuda and mask_bases.device == dev):
                raise ValueError("overlay: the output set must be in device memory")
            out_table = self._out_table(shapes, dev)
            if out_table.total_bytes != out_bytes:
                raise ValueError(f"overlay: the out table holds {out_table.total_bytes} bytes, {out_bytes} expected")
            if annotated is not None and not (annotated.is_contiguous() and annotated.device == dev):
                raise ValueError("overlay: annotated must be a contiguous buffer on the outputs' device")
            self._selection_out(r, out_table, shapes, dev)
            need = int(lib().vti_overlay_frames_scratch_bytes(self._ctx, C.c_void_p(out_table.host.data_ptr()), max_det, int(max_points)))
            if need <= 0:
                raise ValueError(f"overlay: unsupported geometry (n_sel={n_sel}, max_det={max_det}, frames up to "
                                 f"{out_table.max_H0}x{out_table.max_W0}, max_points={max_points}; a drawn frame is at most 8192 x 8192)")
        else:
            if annotated is not None and not (isinstance(annotated, torch.Tensor) and annotated.dtype == torch.uint8 and annotated.is_contiguous()
                                              and tuple(annotated.shape) == (n_sel, H0, W0, 3) and annotated.device == dev):
                raise ValueError(f"overlay: annotated must be a contiguous uint8 [{n_sel},{H0},{W0},3] tensor on the outputs' device")
            if "frames" not in r:
                r["frames"] = torch.empty((n_sel, H0, W0, 3), dtype=torch.uint8, device=dev)
            need = self.overlay_scratch_bytes(n_sel, max_det, H0, W0, max_points)
            if need <= 0:
                raise ValueError(f"overlay: unsupported geometry (n_sel={n_sel}, max_det={max_det}, {H0}x{W0}, max_points={max_points})")
        ws = self._scratch("_overlay_ws", need, dev)
        dev_sel = torch.from_numpy(sel).to(dev)
        have_masks = capacity and (not ragged or int(capacity_bytes))
        tail = (_ptr(dets), _ptr(out["xyxy"]), _ptr(out["counts"]), _ptr(out["offsets"]), max_det, capacity,
                _ptr(plates) if plates is not None and capacity else C.c_void_p(0), C.c_void_p(pal.ctypes.data), int(pal.shape[0]),
                float(alpha), float(beta), C.c_void_p(sel.ctypes.data), _ptr(dev_sel), n_sel, int(mode_i), _ptr(annotated),
                int(max_points))
        if table is not None:
            check(self._ctx, lib().vti_overlay_frames(
                self._ctx, _ptr(frames), *table._ptrs(), B, _ptr(masks) if have_masks else C.c_void_p(0), int(ragged),
                _ptr(mask_bases) if ragged else C.c_void_p(0), int(capacity_bytes) if ragged else 0, *tail, *out_table._ptrs(),
                _ptr(r["buf"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
            return r
        check(self._ctx, lib().vti_overlay(
            self._ctx, _ptr(frames), B, H0, W0, _ptr(masks) if capacity else C.c_void_p(0), int(bool(native)), *tail,
            _ptr(r["frames"]), _ptr(r["status"]), _ptr(ws), ws.numel(), _stream()))
        return r

    # ---- the saved JPEG (cv2.imwrite(save_path, annotated), main.py:314): vti_encode_jpeg ----------------------------------
    def encode_jpeg_scratch_bytes(self, n, H0, W0):
        return int(lib().vti_encode_jpeg_scratch_bytes(self._ctx, int(n), int(H0), int(W0)))

    def encode_jpeg(self, frames, quality=95, rgb=False, max_bytes=None, table=None):
        """The frames as JPEG files, byte for byte jpeg.encode(frame, quality, rgb) (libjpeg's baseline 4:2:0 file): vti_encode_jpeg.
        frames: a contiguous uint8 [n,H0,W0,3] device tensor, BGR unless rgb (annotate()'s "frames", or a raw batch); never written.
        -> (out u8 [max_bytes], offsets i64 [n+1]) on the device: file k is out[offsets[k]:offsets[k+1]].  max_bytes: the room for
        the n files, 3 * n * H0 * W0 + 1024 * n by default; when offsets[n] exceeds it (one host read of that value) the call runs
        again with exactly offsets[n].  The scratch is kept per (n, H0, W0).
        table (vti_encode_jpeg_frames): a FrameTable; `frames` is then the flat u8 device buffer it describes (annotate(..., table=)'s
        buf with its table, a decoded batch, ...) and file k is frame k at its own size.  max_bytes defaults to the sum of 3 * H0 * W0
        + 1024 over the frames; the scratch is kept per tuple of shapes."""
        if table is not None:
            self._check_frames(table)
            if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 1:
                raise ValueError("encode_jpeg: with table=, frames must be the flat uint8 frame buffer")
            n = table.B
        else:
            if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3:
                raise ValueError("encode_jpeg: frames must be a uint8 [n,H0,W0,3] tensor")
            n, H0, W0, _ = frames.shape
        quality = int(quality)
        if not 1 <= quality <= 100:
            raise ValueError(f"encode_jpeg: quality must be in 1..100, got {quality}")
        if max_bytes is None:
            max_bytes = sum(3 * h * w + 1024 for h, w in table.shapes) if table is not None else 3 * n * H0 * W0 + 1024 * n
        max_bytes = int(max_bytes)
        if max_bytes < 0:
            raise ValueError("encode_jpeg: max_bytes must be >= 0")
        if table is not None:
            need = int(lib().vti_encode_jpeg_frames_scratch_bytes(self._ctx, C.c_void_p(table.host.data_ptr())))
            if need <= 0:
                raise ValueError(f"encode_jpeg: unsupported geometry ({n} frames up to {table.max_H0}x{table.max_W0}; 1 <= H0, W0 <= 8192)")
            self._check_frames(table, buf=frames)
        else:
            need = self.encode_jpeg_scratch_bytes(n, H0, W0)
            if need <= 0:
                raise ValueError(f"encode_jpeg: unsupported geometry (n={n}, {H0}x{W0}; 1 <= H0, W0 <= 8192)")
        if not frames.is_cuda or not frames.is_contiguous():
            raise ValueError("encode_jpeg: frames must be a contiguous device tensor")
        dev = frames.device
        key = (tuple(table.shapes), str(dev)) if table is not None else (n, H0, W0, str(dev))
        ws = getattr(self, "_jpeg_ws", None)
        if ws is None or ws[0] != key:
            self._jpeg_ws = None                        # free the old scratch before the new one is allocated
            ws = self._jpeg_ws = (key, torch.empty(need, dtype=torch.uint8, device=dev))
        ws = ws[1]
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)

        def launch(room):
            out = torch.empty((room,), dtype=torch.uint8, device=dev)
            if table is not None:
                check(self._ctx, lib().vti_encode_jpeg_frames(self._ctx, _ptr(frames), *table._ptrs(), n, int(bool(rgb)), quality, _ptr(ws),
                                                              ws.numel(), _ptr(offsets), _ptr(out) if room else C.c_void_p(0), room,
                                                              _stream()))
                return out
            check(self._ctx, lib().vti_encode_jpeg(self._ctx, _ptr(frames), n, H0, W0, int(bool(rgb)), quality, _ptr(ws), ws.numel(),
                                                   _ptr(offsets), _ptr(out) if room else C.c_void_p(0), room, _stream()))
            return out
        out = launch(max_bytes)
        total = int(offsets[n])
        if total > max_bytes:                           # nothing was written: run again with exactly the room the files need
            out = launch(total)
        return out, offsets

    # ---- the text of the annotated pictures (cv2.putText): vti_pack_stamps, vti_stamp, vti_stamp_frames -------------------------
    def pack_stamps(self, stamps_per_picture, shapes, device=None, pitch_extra=0, pad_fill=0):
        """stamps_per_picture: per picture the list of stamps (x, y, bits bool [h, w], BGR colour) of annotate.text_stamps, in painting
        order; shapes: the pictures' (H0, W0).  Packs the rows of every stamp into 32-bit words (bit j of word q of a row: column
        32 q + j), validates and packs the stamp table (vti_pack_stamps: a VtiError names the failing stamp) and uploads both, one
        copy each.  -> StampTable (host, dev, bits).  pitch_extra: words added to every row's pitch; pad_fill: the 32-bit pattern the
        bits at columns >= w are filled with (they are ignored)."""
        shapes = [(int(h), int(w)) for h, w in (tuple(x)[:2] for x in shapes)]
        if len(stamps_per_picture) != len(shapes) or not shapes:
            raise ValueError(f"pack_stamps: {len(stamps_per_picture)} lists of stamps for {len(shapes)} pictures (at least one)")
        descs, words, at = [], [], 0
        for k, stamps in enumerate(stamps_per_picture):
            for x, y, bits, colour in stamps:
                bits = np.asarray(bits, dtype=bool)
                if bits.ndim != 2 or bits.size == 0:
                    raise ValueError(f"pack_stamps: picture {k}: a stamp's bits must be a non-empty 2-D array")
                h, w = bits.shape
                pitch = (w + 31) // 32 + int(pitch_extra)
                row = np.zeros((h, pitch * 32), dtype=bool)
                if pad_fill:
                    row[:] = np.tile(np.unpackbits(np.array([pad_fill], dtype="<u4").view(np.uint8), bitorder="little"), pitch)[None]
                row[:, :w] = bits
                words.append(np.packbits(row, axis=1, bitorder="little").view("<u4").reshape(-1))
                b, g, r = (int(v) for v in colour[:3])
                descs.append(_lib.VtiStampDesc(k, int(x), int(y), w, h, pitch, (C.c_uint8 * 4)(b, g, r, 0), 0, at))
                at += h * pitch
        n, ns = len(shapes), len(descs)
        nbytes = int(lib().vti_stamp_table_bytes(n, ns))
        if nbytes <= 0:
            raise ValueError(f"pack_stamps: {n} pictures and {ns} stamps are outside the limits of vti_stamp_table_bytes()")
        host = torch.zeros(nbytes, dtype=torch.uint8)
        H0 = (C.c_int32 * n)(*[h for h, _ in shapes])
        W0 = (C.c_int32 * n)(*[w for _, w in shapes])
        arr = (_lib.VtiStampDesc * ns)(*descs) if ns else None
        check(self._ctx, lib().vti_pack_stamps(self._ctx, H0, W0, n, arr, ns, at, C.c_void_p(host.data_ptr()), nbytes))
        dev = device or self.device or "cuda"
        flat = np.concatenate(words).astype("<u4") if words else np.zeros(0, "<u4")
        bits_dev = torch.from_numpy(flat.view(np.int32)).to(dev) if at else None
        return StampTable(host, host.to(dev), bits_dev, at, shapes, ns)

    def stamp(self, frames_or_buf, packed, table=None):
        """Paints the stamps of `packed` (pack_stamps) onto the pictures, in place, byte for byte annotate.stamp per picture:
        vti_stamp on a contiguous uint8 [n,H0,W0,3] device tensor (annotate()'s "frames"), or with table= (the FrameTable of
        annotate(..., table=)) vti_stamp_frames on its flat buffer.  One launch on the current stream, no host synchronisation;
        a byte that no stamp covers is not touched.  -> frames_or_buf."""
        if not isinstance(packed, StampTable):
            raise ValueError("stamp: packed must be the StampTable of Engine.pack_stamps()")
        t = frames_or_buf
        if table is not None:
            self._check_frames(table, B=packed.n)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 1:
                raise ValueError("stamp: with table=, the pictures must be the flat uint8 buffer")
            shapes = [tuple(x) for x in table.shapes]
        else:
            n, H0, W0 = _uniform_frames("stamp", t)
            shapes = [(int(H0), int(W0))] * int(n)
        if shapes != [tuple(x) for x in packed.shapes]:
            raise ValueError("stamp: the stamps were packed for pictures of other sizes (or another number of them)")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("stamp: the pictures must be a contiguous device tensor")
        if table is not None:
            self._check_frames(table, buf=t)
            check(self._ctx, lib().vti_stamp_frames(self._ctx, _ptr(t), *table._ptrs(), packed.n, C.c_void_p(packed.host.data_ptr()),
                                                    _ptr(packed.dev), _ptr(packed.bits), packed.n_words, _stream()))
        else:
            check(self._ctx, lib().vti_stamp(self._ctx, _ptr(t), packed.n, shapes[0][0], shapes[0][1], C.c_void_p(packed.host.data_ptr()),
                                             _ptr(packed.dev), _ptr(packed.bits), packed.n_words, _stream()))
        return t

    # ---- JPEG files -> frames (cap.read() of a motion-JPEG camera, cv2.imread): vti_decode_jpeg ------------------------------
    def decode_jpeg_plan(self, files, dense=None, segment_bytes=0, stage=None):
        """Host only: parses and validates the files (vti_decode_jpeg_plan; a VtiError names the first refused file and why) ->
        dict(n, table_bytes, files_at, used, shapes, byte_offsets, out_bytes, scratch_bytes, dense, stage): `stage` is a u8 host
        tensor that holds the descriptor table at 0 and the concatenated files at files_at (a multiple of 256)."""
        files = list(files)
        n = len(files)
        if n < 1:
            raise ValueError("decode_jpeg: at least one file")
        for k, f in enumerate(files):
            if not isinstance(f, (bytes, bytearray, memoryview)):
                raise ValueError(f"decode_jpeg: file {k} must be bytes, got {type(f).__name__}")
        tb = int(lib().vti_decode_jpeg_table_bytes(n))
        if tb <= 0:
            raise ValueError(f"decode_jpeg: 1 <= n <= 4096 files, got {n}")
        files_at = (tb + 255) & ~255
        offs = np.zeros(n + 1, np.int64)
        np.cumsum([len(f) for f in files], out=offs[1:])
        used = files_at + int(offs[n])
        if stage is None or stage.numel() < used:
            stage = torch.empty(max(used, 1 << 16), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        flat = stage.numpy()
        for k, f in enumerate(files):
            flat[files_at + offs[k]:files_at + offs[k + 1]] = np.frombuffer(f, np.uint8)
        H0, W0 = (C.c_int32 * n)(), (C.c_int32 * n)()
        out_off, scratch = (C.c_int64 * (n + 1))(), C.c_int64(0)

        def plan(layout):
            check(self._ctx, lib().vti_decode_jpeg_plan(self._ctx, C.c_void_p(stage.data_ptr() + files_at), C.c_void_p(offs.ctypes.data), n,
                                                        int(segment_bytes), layout, C.c_void_p(stage.data_ptr()), tb, H0, W0, out_off,
                                                        C.byref(scratch)))
        plan(1 if dense else 0)
        shapes = [(int(h), int(w)) for h, w in zip(H0, W0)]
        if dense is None:
            dense = all(x == shapes[0] for x in shapes)
            if dense:
                plan(1)
        return dict(n=n, table_bytes=tb, files_at=files_at, used=used, shapes=shapes, byte_offsets=[int(v) for v in out_off[:n]],
                    out_bytes=int(out_off[n]), scratch_bytes=int(scratch.value), dense=bool(dense), stage=stage)

    def decode_jpeg(self, files, rgb=True, dense=None, segment_bytes=0, device=None):
        """JPEG files (a list of bytes) -> frames on the device, byte for byte jpeg.decode(file, rgb): vti_decode_jpeg.  One pinned
        staging copy and one asynchronous H2D of the descriptor table and the concatenated files; nothing is read back.
        dense (None: when all files have one size) -> (frames u8 [n,H0,W0,3], info); otherwise -> (buf u8 flat, shapes [(H0, W0)],
        byte_offsets, info) with the frames laid out as pack_frames lays them, so `buf` is a frame-table buffer.  info i32 [n,4] =
        {status (0 or VTI_JPEG_CORRUPT), segments, rounds, blocks}.  The staging buffer, its device twin and the scratch are kept and
        grown; a refused file raises before anything is launched."""
        st = getattr(self, "_jd", None) or {}
        ev = st.get("event")
        if ev is not None:
            ev.synchronize()                # the staging buffer is free once the previous copy has left it
        p = self.decode_jpeg_plan(files, dense, segment_bytes, st.get("stage"))
        if not torch.cuda.is_available():
            raise ValueError("decode_jpeg: needs a ROCm device (no CPU fallback; jpeg.decode is the host specification)")
        dev = torch.device(device) if device is not None else (self.device or torch.device("cuda", torch.cuda.current_device()))
        if st.get("dev") is None or st["dev"].numel() < p["used"] or st["dev"].device != dev:
            st["dev"] = torch.empty(p["stage"].numel(), dtype=torch.uint8, device=dev)
        if st.get("ws") is None or st["ws"].numel() < p["scratch_bytes"] or st["ws"].device != dev:
            st["ws"] = None
            st["ws"] = torch.empty(max(p["scratch_bytes"], 256), dtype=torch.uint8, device=dev)
        st["stage"] = p["stage"]
        dbuf, ws = st["dev"], st["ws"]
        dbuf[:p["used"]].copy_(p["stage"][:p["used"]], non_blocking=True)
        st["event"] = torch.cuda.Event()
        st["event"].record()
        self._jd = st
        n = p["n"]
        out = torch.empty(p["out_bytes"], dtype=torch.uint8, device=dev)
        info = torch.empty((n, 4), dtype=torch.int32, device=dev)
        check(self._ctx, lib().vti_decode_jpeg(self._ctx, C.c_void_p(dbuf.data_ptr() + p["files_at"]), C.c_void_p(p["stage"].data_ptr()),
                                               _ptr(dbuf), n, int(bool(rgb)), _ptr(out), out.numel(), _ptr(info), _ptr(ws), ws.numel(),
                                               _stream()))
        if p["dense"]:
            h, w = p["shapes"][0]
            return out.view(n, h, w, 3), info
        return out, p["shapes"], p["byte_offsets"], info

    # ---- raw camera frames -> BGR frames (cap.read() with CAP_PROP_CONVERT_RGB = 0): vti_convert_raw -------------------------------
    def convert_raw(self, raw, fmt, H0, W0, rgb=False, out=None):
        """n raw frames of one size and format -> u8 [n,H0,W0,3] on the device, byte for byte rawframes.to_bgr(raw, fmt, H0, W0, rgb):
        vti_convert_raw.  raw: a uint8 tensor of any shape with n * rawframes.frame_bytes(fmt, H0, W0) bytes -- a device tensor is
        used in place (any byte address), a CPU tensor, ndarray or bytes is copied to the device first.  fmt: a name ("yuyv", "uyvy",
        "nv12", "nv21", "i420", "yv12") or its VTI_RAW_* value.  out: the u8 [n,H0,W0,3] device tensor to write (any byte address)."""
        f = rawframes.format_id(fmt)
        fb = rawframes.frame_bytes(f, H0, W0)
        if not isinstance(raw, torch.Tensor):
            raw = torch.from_numpy(np.array(rawframes.as_bytes(raw)))
        if raw.dtype != torch.uint8:
            raise ValueError(f"convert_raw: raw must be uint8, got {raw.dtype}")
        if raw.numel() == 0 or raw.numel() % fb:
            raise ValueError(f"convert_raw: {rawframes.NAMES[f]} {H0}x{W0} frames are {fb} bytes each, got {raw.numel()} bytes")
        n = raw.numel() // fb
        if n > 4096:
            raise ValueError(f"convert_raw: at most 4096 frames per call, got {n}")
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != (n, H0, W0, 3)
                                or not out.is_contiguous()):
            raise ValueError(f"convert_raw: out must be a contiguous uint8 [{n},{H0},{W0},3] tensor")
        if not torch.cuda.is_available():
            raise ValueError("convert_raw: needs a ROCm device (no CPU fallback; rawframes.to_bgr is the host specification)")
        if not raw.is_cuda:
            dev = out.device if out is not None else (self.device or torch.device("cuda", torch.cuda.current_device()))
            raw = raw.to(dev, non_blocking=True)
        raw = raw.contiguous()
        if out is None:
            out = torch.empty((n, H0, W0, 3), dtype=torch.uint8, device=raw.device)
        elif out.device != raw.device:
            raise ValueError("convert_raw: raw and out must be on one device")
        check(self._ctx, lib().vti_convert_raw(self._ctx, _ptr(raw), f, n, int(H0), int(W0), int(bool(rgb)), _ptr(out), _stream()))
        return out

    def pack_raw_frames(self, shapes, fmts, device=None):
        """shapes: one (H0, W0) per raw frame, fmts: one format (name or VTI_RAW_* value) per frame, or one for all.  Validates the
        frames, places them back to back at multiples of 16 bytes, packs the raw table and uploads it once -> RawTable (its
        raw_offsets / raw_bytes say where the frames go in the flat raw buffer); a VtiError names the failing frame."""
        shapes = [(int(h), int(w)) for h, w in (tuple(x)[:2] for x in shapes)]
        n = len(shapes)
        if isinstance(fmts, (str, int, np.integer)):
            fmts = [fmts] * n
        fmts = [rawframes.format_id(f) for f in fmts]
        if len(fmts) != n:
            raise ValueError(f"pack_raw_frames: {n} shapes but {len(fmts)} formats")
        nbytes = int(lib().vti_raw_table_bytes(n))
        if nbytes <= 0:
            raise ValueError(f"pack_raw_frames: 1 <= n <= 4096 frames, got {n}")
        host = torch.zeros(nbytes, dtype=torch.uint8)
        off = (C.c_int64 * (n + 1))()
        check(self._ctx, lib().vti_pack_raw_frames(self._ctx, (C.c_int32 * n)(*[h for h, _ in shapes]), (C.c_int32 * n)(*[w for _, w in shapes]),
                                                   (C.c_int32 * n)(*fmts), n, C.c_void_p(host.data_ptr()), nbytes, off))
        dev = host.to(device or self.device or "cuda")
        return RawTable(host, dev, shapes, fmts, [int(v) for v in off[:n]], int(off[n]))

    def convert_raw_frames(self, buf, raw_table, table, rgb=False, out=None):
        """Raw frames that differ in size and / or format -> the frame-table buffer of `table` (pack_frames of the same shapes):
        vti_convert_raw_frames.  buf: flat u8 device tensor of >= raw_table.raw_bytes bytes with frame k at raw_table.raw_offsets[k];
        out: flat u8 device tensor of >= table.total_bytes bytes (allocated when None).  Frame k lands at table.byte_offsets[k], byte
        for byte rawframes.to_bgr of it; the gaps between frames are not written.  (out, table) is what predict_frames_into,
        annotate(table=) and encode_jpeg(table=) take."""
        if not isinstance(raw_table, RawTable):
            raise ValueError("convert_raw_frames: raw_table must be the RawTable of Engine.pack_raw_frames()")
        self._check_frames(table, B=raw_table.n)
        if list(raw_table.shapes) != list(table.shapes):
            raise ValueError("convert_raw_frames: the raw table and the frame table describe frames of other shapes")
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.uint8 or buf.dim() != 1 or not buf.is_contiguous() \
                or buf.numel() < raw_table.raw_bytes:
            raise ValueError(f"convert_raw_frames: buf must be a flat contiguous uint8 tensor of >= {raw_table.raw_bytes} bytes")
        if buf.device != table.dev.device or raw_table.dev.device != table.dev.device:
            raise ValueError("convert_raw_frames: the raw buffer, the raw table and the frame table must be on one device")
        if out is None:
            out = torch.empty(table.total_bytes, dtype=torch.uint8, device=buf.device)
        self._check_frames(table, buf=out)
        check(self._ctx, lib().vti_convert_raw_frames(self._ctx, _ptr(buf), buf.numel(), *raw_table._ptrs(), *table._ptrs(), table.B,
                                                      int(bool(rgb)), _ptr(out), out.numel(), _stream()))
        return out

    # ---- Results.masks.xy: instance polygons in frame pixels (vti_mask_polygons) -------------------------------------------
    def mask_polygons_scratch_bytes(self, H, W, row_bytes):
        return int(lib().vti_mask_polygons_scratch_bytes(self._ctx, int(H), int(W), int(row_bytes)))

    def mask_polygons(self, masks_bits, W, H0, W0, strategy="largest", offsets=None):
        """Ultralytics masks2segments + scale_coords (polygons.py, bit for bit) on the device.  masks_bits: u8 [n,H,row_bytes] LSB-first
        with W real columns (masks()' bits: row_bytes = W/8; masks_native()'s rows: W = W0).  strategy "largest" (the outer contour with
        the most vertices) or "concat" (every outer contour).  `offsets` (i32 [B+1] from masks()): slots at and beyond offsets[B] are not
        read and have empty polygons.  -> (points f32 [P,2] (x, y) in H0 x W0 frame pixels, point_offsets i32 [n+1]): slot i's polygon
        is points[point_offsets[i]:point_offsets[i+1]].  `points` is a view of a buffer the engine keeps and reuses: valid until the next
        call.  One host read (the vertex total and the status word); a second launch only when the kept buffer was too small."""
        if strategy not in POLY_STRATEGIES:
            raise ValueError(f"strategy must be one of {sorted(POLY_STRATEGIES)}, got {strategy!r}")
        masks_bits = masks_bits.contiguous()
        n, H, rb = masks_bits.shape
        dev = masks_bits.device
        need = self.mask_polygons_scratch_bytes(H, W, rb)
        if need <= 0:
            raise ValueError(f"mask_polygons: bad mask geometry H={H} W={W} row_bytes={rb}")
        ws = getattr(self, "_poly_ws", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            self._poly_ws = None                       # free the old scratch before the new one is allocated
            ws = self._poly_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        pts = getattr(self, "_poly_points", None)
        if pts is None or pts.device != dev:
            pts = self._poly_points = torch.empty((1 << 16, 2), dtype=torch.float32, device=dev)
        point_offsets = torch.empty((n + 1,), dtype=torch.int32, device=dev)
        n_live = C.c_void_p(offsets.data_ptr() + 4 * (offsets.numel() - 1)) if offsets is not None else C.c_void_p(0)

        def launch(buf):
            check(self._ctx, lib().vti_mask_polygons(self._ctx, _ptr(masks_bits) if n else C.c_void_p(0), n, n_live, H, int(W), rb,
                                                     int(H0), int(W0), POLY_STRATEGIES[strategy], _ptr(ws), ws.numel(),
                                                     _ptr(point_offsets), _ptr(buf), buf.shape[0], _stream()))
        launch(pts)
        total, status = torch.cat((point_offsets[n:], ws[:4].view(torch.int32))).tolist()
        if status != _lib.VTI_POLY_OK:
            raise _lib.VtiError(-4, f"vti_mask_polygons: status word {status} (1: a loop reached its bound, "
                                    f"2: more than 2^31-1 vertices)")     # -4: VTI_ERR_HIP, an error found on the device
        if total > pts.shape[0]:                       # the kept buffer was too small: grow it and run again
            self._poly_points = None
            pts = self._poly_points = torch.empty((max(total, 2 * pts.shape[0]), 2), dtype=torch.float32, device=dev)
            launch(pts)
        return pts[:total], point_offsets

    # ---- the polygons of a batch whose frames differ in size (vti_mask_polygons_frames) ---------------------------------------
    def mask_polygons_frames_scratch_bytes(self, table, native):
        self._check_frames(table)
        return int(lib().vti_mask_polygons_frames_scratch_bytes(self._ctx, C.c_void_p(table.host.data_ptr()), int(bool(native))))

    def mask_polygons_frames(self, out, table, native=False, strategy="largest"):
        """mask_polygons for every slot of an output set that predict_frames_into() filled, in one call: slot s of frame b
        (offsets[b] <= s < offsets[b+1]) gets the polygon mask_polygons gives it with that frame's (H0, W0) -- letterbox bit masks,
        or with native=True the ragged frame-size rows of a set from alloc_outputs(native_frames=table) (any other set is a
        ValueError).  -> (points f32 [P,2], point_offsets i32 [capacity+1]) as mask_polygons: slots beyond the live ones have empty
        polygons, `points` is a view of the kept buffer, one host read, a second launch only when that buffer was too small."""
        if strategy not in POLY_STRATEGIES:
            raise ValueError(f"strategy must be one of {sorted(POLY_STRATEGIES)}, got {strategy!r}")
        if native:
            self._check_ragged(out, table, out["dets"].shape[1], "mask_polygons_frames")
        masks = out["masks"]
        B = out["counts"].shape[0]
        self._check_frames(table, B=B)
        if not native and (masks.dim() != 3 or tuple(masks.shape[1:]) != (self.H, self.W // 8) or not masks.is_contiguous()):
            raise ValueError(f"mask_polygons_frames: the masks must be contiguous letterbox bit masks u8 [capacity, {self.H}, {self.W // 8}]")
        capacity = (B * out["dets"].shape[1] if native else masks.shape[0]) if masks.numel() else 0
        dev = masks.device
        need = self.mask_polygons_frames_scratch_bytes(table, native)
        if need <= 0:
            raise ValueError("mask_polygons_frames: a frame of the table is above mask_polygons' size limit (H0 * W0 <= 2^26)")
        ws = self._scratch("_poly_ws", need, dev)
        pts = getattr(self, "_poly_points", None)
        if pts is None or pts.device != dev:
            pts = self._poly_points = torch.empty((1 << 16, 2), dtype=torch.float32, device=dev)
        point_offsets = torch.empty((capacity + 1,), dtype=torch.int32, device=dev)
        bases = _ptr(out["mask_bases"]) if native else C.c_void_p(0)

        def launch(buf):
            check(self._ctx, lib().vti_mask_polygons_frames(
                self._ctx, _ptr(masks) if capacity else C.c_void_p(0), int(bool(native)), bases, masks.numel() if native else 0,
                _ptr(out["offsets"]), *table._ptrs(), B, capacity, POLY_STRATEGIES[strategy], _ptr(ws), ws.numel(),
                _ptr(point_offsets), _ptr(buf), buf.shape[0], _stream()))
        launch(pts)
        total, status = torch.cat((point_offsets[capacity:], ws[:4].view(torch.int32))).tolist()
        if status != _lib.VTI_POLY_OK:
            raise _lib.VtiError(-4, f"vti_mask_polygons_frames: status word {status} (1: a loop reached its bound, "
                                    f"2: more than 2^31-1 vertices)")     # -4: VTI_ERR_HIP, an error found on the device
        if total > pts.shape[0]:                       # the kept buffer was too small: grow it and run again
            self._poly_points = None
            pts = self._poly_points = torch.empty((max(total, 2 * pts.shape[0]), 2), dtype=torch.float32, device=dev)
            launch(pts)
        return pts[:total], point_offsets

    # ---- test hook ---------------------------------------------------------------------
    def debug_conv_output(self, i, B):
        t = self.conv_table()[i]
        out = torch.empty((B, t["c2"], t["h_out"], t["w_out"]), dtype=torch.float32, device=self.device)
        check(self._ctx, lib().vti_debug_conv_output(self._ctx, i, B, _ptr(out), _stream()))
        return out

    def debug_set_conv_output(self, i, values):
        """The inverse of debug_conv_output (vti_debug_set_conv_output): values, f32 [B,c2,h_out,w_out] on the device, into conv
        i's output view, encoded as the engine's storage encodes (fp16 rounding, the saturating h2 pair, or f32)."""
        t = self.conv_table()[i]
        if values.dtype != torch.float32 or not values.is_cuda or not values.is_contiguous() or \
                tuple(values.shape[1:]) != (t["c2"], t["h_out"], t["w_out"]):
            raise ValueError(f"debug_set_conv_output: expected contiguous float32 [B,{t['c2']},{t['h_out']},{t['w_out']}] on the device, "
                             f"got {values.dtype} {tuple(values.shape)}")
        check(self._ctx, lib().vti_debug_set_conv_output(self._ctx, i, values.shape[0], _ptr(values), _stream()))

    def debug_run_op(self, i, B, x=None, swap_rb=False, pred=None, proto=None, best=None):
        """Launch the ONE op of the plan that computes conv i (vti_debug_run_op), once, on the current stream: it reads what its
        input views hold (debug_set_conv_output; x, u8 [B,H,W,3], for the stem) and writes its outputs (debug_conv_output reads
        them; pred f32 [B,A,4+nc+nm], best f32 [B,A,2] and proto for the ops that write those).  -> the conv indices the op
        computes, in execution order."""
        convs = (C.c_int32 * 4)()
        check(self._ctx, lib().vti_debug_run_op(self._ctx, i, _ptr(x), B, int(bool(swap_rb)), _ptr(pred), _ptr(proto), _ptr(best),
                                                convs, _stream()))
        return [v for v in convs if v >= 0]

    def _check_input(self, t, hw):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3 or tuple(t.shape[1:3]) != tuple(hw):
            raise ValueError(f"expected uint8 [B,{hw[0]},{hw[1]},3], got {t.dtype} {tuple(t.shape)}")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError("input must be a contiguous device tensor")
        if t.shape[0] > self.max_batch:
            raise ValueError(f"batch {t.shape[0]} exceeds max_batch {self.max_batch}")


def _f64(a, n):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64).ravel())
    if a.size != n:
        raise ValueError(f"expected {n} float64 values, got {a.size}")
    return a


def pixels_to_world(uv, K, dist, R, t):
    """measurement.py:50-65 for n points at once.  uv f64 [n,2] device tensor; K (3x3), dist (5), R (3x3), t (3) host arrays.
    -> (xyz f64 [n,3] device, valid i32 [n])."""
    uv = uv.to(torch.float64).contiguous()
    n = uv.shape[0]
    xyz = torch.empty((n, 3), dtype=torch.float64, device=uv.device)
    valid = torch.empty((n,), dtype=torch.int32, device=uv.device)
    Kh, dh, Rh, th = _f64(K, 9), _f64(dist, 5), _f64(R, 9), _f64(t, 3)
    rc = lib().vti_pixels_to_world(None, _ptr(uv), n, Kh.ctypes.data_as(C.c_void_p), dh.ctypes.data_as(C.c_void_p),
                                   Rh.ctypes.data_as(C.c_void_p), th.ctypes.data_as(C.c_void_p), _ptr(xyz), _ptr(valid), _stream())
    check(None, rc)
    return xyz, valid


def kmeans1d2(values, counts, max_iters=10):
    """measurement.py:88-113 batched.  values f64 [B,max_n] device, counts i32 [B] -> (labels i32 [B,max_n], centers f64 [B,2])."""
    values = values.to(torch.float64).contiguous()
    B, max_n = values.shape
    labels = torch.empty((B, max_n), dtype=torch.int32, device=values.device)
    centers = torch.empty((B, 2), dtype=torch.float64, device=values.device)
    check(None, lib().vti_kmeans1d2(None, _ptr(values), _ptr(counts), B, max_n, int(max_iters), _ptr(labels), _ptr(centers), _stream()))
    return labels, centers


H2_SCALE = 16.0     # conv_dev.h: H2_SX
H2_MAX = 4094.0     # conv_dev.h: H2_MAX (4094 * 16 = 65504, the largest fp16)


def h2_encode(t):
    """float tensor -> the h2 engine's storage: per element the fp16 pair (hi | lo << 16) of value * 16, returned as float32-typed
    bits (same shape).  Saturating at +-4094 as the kernels' h2_enc is; -0 encodes as +0 (the device's fma(v, 16, +0)).
    Host-side helper for tests and the single-conv debug entry point; the engine itself never needs it."""
    s = t.float().clamp(-H2_MAX, H2_MAX) * H2_SCALE + 0.0
    hi = s.half()
    lo = (s - hi.float()).half()
    bits = hi.view(torch.int16).to(torch.int32) & 0xFFFF | (lo.view(torch.int16).to(torch.int32) << 16)
    return bits.view(torch.float32)


def h2_decode(t):
    """inverse of h2_encode (exact: hi + lo has at most 24 significant bits)."""
    bits = t.view(torch.int32)
    hi = (bits & 0xFFFF).to(torch.int16).view(torch.float16).float()
    lo = (bits >> 16).to(torch.int16).view(torch.float16).float()
    return (hi + lo) / H2_SCALE


def unpack_bits(bits, W):
    """u8 [...,R] LSB-first -> u8 [...,W] of 0/1 (host-side convenience for bit-packed masks).  R may be padded past W/8
    (masks_native rows are 8*ceil(W/64) bytes): the columns from W on are dropped."""
    b = bits.unsqueeze(-1)
    sh = torch.arange(8, device=bits.device, dtype=torch.uint8)
    full = ((b >> sh) & 1).reshape(*bits.shape[:-1], bits.shape[-1] * 8)
    return full if full.shape[-1] == W else full[..., :W]


def to_numpy(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def debug_conv2d(x, w, b, k, s, kind=0, dtype="fp16", res=None, out=None, in_coff=0, c1=None, out_coff=0, out_ld=None,
                 out_f32=False, swap_rb=False, tile=(0, 0), waves_n=0, nrep=0, iters=1):
    """Run ONE conv of the engine's conv family (vti_debug_conv2d): unit tests / micro-benchmarks.
    x: device tensor NHWC [B,H,W,ld] of the engine dtype (or uint8 [B,H,W,3] for the stem);
    w: f32 OIHW (kind 2: IOHW) numpy/torch on host; returns (out NHWC, ms_per_launch, cfg)."""
    B, H, W, ld = x.shape
    w = np.ascontiguousarray(to_numpy(w), dtype=np.float32)
    b = np.ascontiguousarray(to_numpy(b), dtype=np.float32)
    c2 = w.shape[1] if kind == 2 else w.shape[0]
    if c1 is None:
        c1 = w.shape[0] if kind == 2 else w.shape[1]
    Ho, Wo = (2 * H, 2 * W) if kind == 2 else ((H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1)
    tdt = torch.float32 if (out_f32 or DTYPES[dtype] != _lib.VTI_F16) else torch.float16      # h2: 4-byte pairs, carried as f32 bits
    if out is None:
        out_ld = out_ld or (out_coff + c2)
        out = torch.zeros((B, Ho, Wo, out_ld), dtype=tdt, device=x.device)
    else:
        out_ld = out.shape[3]
    ms = C.c_float(0)
    cfg = (C.c_int32 * 5)()
    rc = lib().vti_debug_conv2d(DTYPES[dtype], _ptr(x), B, H, W, ld, in_coff, c1, w.ctypes.data_as(C.c_void_p),
                                b.ctypes.data_as(C.c_void_p), c2, k, s, kind, _ptr(res), res.shape[3] if res is not None else 0,
                                0, _ptr(out), out_ld, out_coff, int(out_f32), int(swap_rb), tile[0], tile[1], waves_n, nrep,
                                iters, C.byref(ms), cfg, _stream())
    if rc != 0:
        raise _lib.VtiError(rc, lib().vti_last_error(None).decode())
    return out, ms.value, dict(tile=(cfg[0], cfg[1]), waves_n=cfg[2], nrep=cfg[3], lds=abs(cfg[4]), pk=cfg[4] < 0)


def _nhwc(who, t, dtype):
    """The checks of one NHWC tensor of a single-kernel hook; -> (B, H, W, ld)."""
    want = torch.float16 if DTYPES[dtype] == _lib.VTI_F16 else torch.float32        # h2: 4-byte pairs, carried as f32 bits
    if t.dim() != 4 or t.dtype != want or not t.is_contiguous():
        raise ValueError(f"{who}: expected a contiguous {want} NHWC tensor, got {t.dtype} {tuple(t.shape)}")
    return tuple(t.shape)


def _check_debug(rc):
    if rc != 0:
        raise _lib.VtiError(rc, lib().vti_last_error(None).decode())


def debug_sppf_pool(x, c, dtype="fp16", in_coff=0, out=None, out_coff=None):
    """Run the SPPF's three chained 5x5 max-pools alone (vti_debug_sppf_pool): channels [in_coff, in_coff + c) of x (NHWC
    [B,H,W,ld] of the engine dtype; h2 as float32-typed bits) -> channels [out_coff, out_coff + 3 c) of `out` (default: x itself at
    out_coff = in_coff + c, the engine's layout).  Enqueued on the current stream.  -> (out, path): path 0 = the global-memory
    kernel, 1 / 4 = the LDS kernel with one / four 16-byte pieces per lane group."""
    B, H, W, ld = _nhwc("debug_sppf_pool", x, dtype)
    if out is None:
        out = x
    if tuple(out.shape) != (B, H, W, ld) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("debug_sppf_pool: out must have x's shape, dtype and layout")
    if out_coff is None:
        out_coff = in_coff + c
    path = C.c_int32(-1)
    _check_debug(lib().vti_debug_sppf_pool(DTYPES[dtype], _ptr(x), _ptr(out), B, H, W, c, ld, in_coff, out_coff, C.byref(path), _stream()))
    return out, path.value


def debug_upsample2x(x, c, out, dtype="fp16", in_coff=0, out_coff=0):
    """Run the nearest 2x upsample alone (vti_debug_upsample2x): channels [in_coff, in_coff + c) of x (NHWC [B,H,W,in_ld]) ->
    channels [out_coff, out_coff + c) of out (NHWC [B,2H,2W,out_ld], same dtype).  Enqueued on the current stream.  -> out."""
    B, H, W, in_ld = _nhwc("debug_upsample2x", x, dtype)
    Bo, Ho, Wo, out_ld = _nhwc("debug_upsample2x", out, dtype)
    if (Bo, Ho, Wo) != (B, 2 * H, 2 * W):
        raise ValueError(f"debug_upsample2x: out must be [{B},{2 * H},{2 * W},out_ld], got {tuple(out.shape)}")
    _check_debug(lib().vti_debug_upsample2x(DTYPES[dtype], _ptr(x), _ptr(out), B, H, W, c, in_ld, in_coff, out_ld, out_coff, _stream()))
    return out


def debug_decode(box, cls, mc, levels, strides, nc, nm, pred, box_only=False):
    """Run the Detect/Segment decode alone (vti_debug_decode).  box / cls / mc: three contiguous f32 device tensors each, level l
    of shape [B, H_l * W_l, 64 | nc | nm]; levels: three (H_l, W_l); pred: f32 [B, A, 4 + nc + nm], A = sum H_l W_l.  box_only: the
    box-only kernel, which writes pred[..., :4] and nothing else (cls and mc may be None).  Enqueued on the current stream.  -> pred."""
    def table(ts, width):
        if ts is None:
            return None
        for t, (h, w) in zip(ts, levels):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, h * w, width):
                raise ValueError(f"debug_decode: expected contiguous float32 [{B},{h * w},{width}], got {t.dtype} {tuple(t.shape)}")
        return (C.c_void_p * 3)(*[t.data_ptr() for t in ts])
    B = pred.shape[0]
    A = sum(h * w for h, w in levels)
    if len(levels) != 3 or pred.dtype != torch.float32 or not pred.is_contiguous() or tuple(pred.shape) != (B, A, 4 + nc + nm):
        raise ValueError(f"debug_decode: pred must be contiguous float32 [B,{A},{4 + nc + nm}], got {pred.dtype} {tuple(pred.shape)}")
    hs, ws, st = ((C.c_int32 * 3)(*v) for v in ([h for h, _ in levels], [w for _, w in levels], list(strides)))
    _check_debug(lib().vti_debug_decode(int(bool(box_only)), table(box, 64), table(cls, nc), table(mc, nm), hs, ws, st, B, nc, nm, _ptr(pred), _stream()))
    return pred
