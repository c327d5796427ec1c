"""Drop-in mirror of the `ultralytics.YOLO` protocol as the reference consumes it.

    model = YOLO(path)                                         measurement.py:145
    results = model.predict(rgb, verbose=False, conf=..., iou=..., max_det=..., imgsz=960)
                                                               measurement.py:208-210
    r = results[0]; r.boxes.cls / .xyxy / .conf; len(r.boxes); r.masks.data[idx]; model.names
                                   measurement.py:74-75,242-245; Utils/check_model.py:170-209,341

Same names, argument meaning and error behaviour (any failure raises; the caller's try/except
at measurement.py:207-216 turns it into an error dict).  Everything numeric runs in libvti.so.
"""
import math
import os

import numpy as np
import torch

from . import rawframes
from .engine import check_window, Engine, NmsParams, unpack_bits
from .weights import random_weights, unpack_container


def letterbox_shape(H0, W0, imgsz, auto=True, stride=32):
    """Ultralytics LetterBox output size."""
    new_shape = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
    new_shape = tuple(max(math.ceil(x / stride) * stride, stride) for x in new_shape)   # Ultralytics check_imgsz: round up to the stride
    r = min(new_shape[0] / H0, new_shape[1] / W0)
    new_w, new_h = int(round(W0 * r)), int(round(H0 * r))
    dw, dh = new_shape[1] - new_w, new_shape[0] - new_h
    if auto:
        dw, dh = dw % stride, dh % stride
    dw, dh = dw / 2, dh / 2
    top, bottom = int(round(dh - 0.1)), int(round(dh + 0.1))
    left, right = int(round(dw - 0.1)), int(round(dw + 0.1))
    return new_h + top + bottom, new_w + left + right


class Boxes:
    """Results.boxes: xyxy in ORIGINAL frame pixels, conf-descending."""

    def __init__(self, data, orig_shape):
        self.data = data                 # f32 [N,6]: x1,y1,x2,y2,conf,cls
        self.orig_shape = orig_shape

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, 4]

    @property
    def cls(self):
        return self.data[:, 5]

    def __len__(self):
        return self.data.shape[0]


class Masks:
    """Results.masks: `.data` is f32 0/1 [N,H,W] at the LETTERBOXED size, as Ultralytics returns it, or [N,H0,W0] at the frame
    size with predict(retina_masks=True).  The engine writes bit-packed masks (u8 [N,H,W/8]; retina: u8 [N,H0,8*ceil(W0/64)]);
    they are expanded on the device the first time `.data` / `.data_u8` is read."""

    def __init__(self, bits, W, orig_shape, engine=None):
        self.bits = bits                 # u8 [N,H,R] device tensor, LSB-first; W columns of the R*8 are real
        self._W = W
        self.orig_shape = orig_shape
        self._engine = engine            # the Engine that made the masks: .xy runs its vti_mask_polygons
        self._u8 = None
        self._f = None
        self._xy = None
        self._xyn = None

    @property
    def data_u8(self):
        if self._u8 is None:
            self._u8 = unpack_bits(self.bits, self._W)
        return self._u8

    @property
    def data(self):
        if self._f is None:
            self._f = self.data_u8.float()
        return self._f

    @property
    def xy(self):
        """One float32 [n,2] (x, y) polygon per instance in ORIGINAL frame pixels: the largest outer contour of the mask
        (Ultralytics masks2segments + scale_coords; Utils/check_model.py:185-188 fills it).  Computed on the device on first use
        (Engine.mask_polygons, bit-identical to polygons.py), then one copy to the host."""
        if self._xy is None:
            if self._engine is None:
                raise RuntimeError("Masks.xy needs the Engine that made the masks (Masks(..., engine=)); there is no host path")
            n = self.bits.shape[0]
            pts, off = self._engine.mask_polygons(self.bits, self._W, *self.orig_shape)
            host = torch.cat((pts.reshape(-1).view(torch.int32), off)).cpu().numpy()     # one device -> host copy, bits as int32
            p = host[:pts.numel()].view(np.float32).reshape(-1, 2)
            o = host[pts.numel():]
            self._xy = [p[o[i]:o[i + 1]] for i in range(n)]
        return self._xy

    @property
    def xyn(self):
        """Ultralytics' normalised segments: xy divided by (W0, H0) in float32 (scale_coords(..., normalize=True))."""
        if self._xyn is None:
            wh = np.array((self.orig_shape[1], self.orig_shape[0]), dtype=np.float32)
            self._xyn = [s / wh for s in self.xy]
        return self._xyn

    def __len__(self):
        return self.bits.shape[0]


class Results:
    def __init__(self, orig_shape, names, boxes, masks, dets=None):
        self.orig_shape = orig_shape
        self.names = names
        self.boxes = boxes
        self.masks = masks               # None when there are no detections (as Ultralytics)
        self.dets = dets                 # raw rows incl. mask coefficients, letterboxed px

    def __len__(self):
        return len(self.boxes)


class DecodedFrames:
    """Frames of differing sizes that Engine.decode_jpeg left on the device: `buf` is a frame-table buffer (pack_frames' layout)."""

    def __init__(self, buf, shapes, byte_offsets):
        self.buf, self.shapes, self.byte_offsets = buf, shapes, byte_offsets


class RawFrames:
    """n raw camera frames of one size and format, as cap.read() returns them with CAP_PROP_CONVERT_RGB = 0: a source of
    YOLO.predict and the measurers' process_frames, converted on the device (vti_convert_raw) to the BGR frames cap.read() would
    otherwise have delivered (rawframes.to_bgr).  data: a uint8 ndarray, a CPU or device tensor, or bytes, of any shape with
    n * rawframes.frame_bytes(fmt, H0, W0) bytes ([H0,W0,2] and [H0*3/2,W0] as OpenCV shapes them, [n,...] stacks, flat buffers);
    fmt: "yuyv", "uyvy", "nv12", "nv21", "i420", "yv12" or the VTI_RAW_* value."""

    def __init__(self, data, fmt, H0, W0):
        self.fmt = rawframes.format_id(fmt)
        self.frame_bytes = rawframes.frame_bytes(self.fmt, H0, W0)
        self.H0, self.W0 = int(H0), int(W0)
        if isinstance(data, torch.Tensor):
            if data.dtype != torch.uint8:
                raise ValueError(f"RawFrames: data must be uint8, got {data.dtype}")
            flat = data.contiguous().reshape(-1)
            count = flat.numel()
        else:
            flat = rawframes.as_bytes(data, "RawFrames: data")
            count = flat.size
        if count == 0 or count % self.frame_bytes:
            raise ValueError(f"RawFrames: {rawframes.NAMES[self.fmt]} {self.H0}x{self.W0} frames are {self.frame_bytes} bytes each; "
                             f"expected a multiple of {self.frame_bytes} bytes, got {count}")
        self.data = flat                 # flat uint8: an ndarray, or the tensor (CPU or device) as it was given
        self.n = count // self.frame_bytes

    def __len__(self):
        return self.n

    def frame(self, k):
        """Frame k's bytes (a flat view)."""
        return self.data[k * self.frame_bytes:(k + 1) * self.frame_bytes]

    def to_bgr(self, rgb=False):
        """The host specification of what the device makes of these frames: uint8 [n,H0,W0,3]."""
        d = self.data.cpu().numpy() if isinstance(self.data, torch.Tensor) else self.data
        return rawframes.to_bgr(d, self.fmt, self.H0, self.W0, rgb)


class RawBatch:
    """Raw frames of differing sizes and / or formats on their way to one vti_convert_raw_frames: one (fmt, flat bytes) per frame."""

    def __init__(self, members):
        self.frames = [(m.fmt, m.frame(k)) for m in members for k in range(m.n)]
        self.shapes = [(m.H0, m.W0) for m in members for _ in range(m.n)]
        self.fmts = [f for f, _ in self.frames]


class YOLO:
    """`YOLO(path)` takes a VTIW1 container; `YOLO(None, scale=, nc=, seed=)` makes seeded random weights."""

    def __init__(self, model=None, *, scale="n", nc=80, seed=1, cls_bias=None, dtype="h2", device=0,
                 names=None, mask_mode="logit", max_batch=64, drop_empty_masks=False):
        """dtype: "h2" (default; split-fp16 storage on the fp16 matrix pipe -- results within the reference tolerance of the fp32 CPU
        path: mask IoU >= 0.999, |d box| < 1e-3), "fp32" (exact-f32 MFMA, slower) or "fp16" (fastest; boxes drift ~1 px and masks to
        IoU ~0.92-0.99 on untrained margins).  drop_empty_masks: newer Ultralytics releases drop instances whose thresholded mask is
        empty (`keep = masks.sum((-2, -1)) > 0`); older ones (and the default here) return them."""
        self._blob = None
        if isinstance(model, (bytes, bytearray, memoryview)):
            self._blob = bytes(model)
        elif isinstance(model, (str, os.PathLike)):
            with open(model, "rb") as f:
                self._blob = f.read()
        elif model is not None:
            raise TypeError("model must be a path, bytes or None")
        if self._blob is not None:
            meta, _, _ = unpack_container(self._blob)
            scale, nc = meta["scale"], meta["nc"]
            self._nm, self._reg_max = meta["nm"], meta["reg_max"]
        else:
            self._nm, self._reg_max = 32, 16
        self.scale, self.nc, self.dtype, self.device = scale, nc, dtype, device
        self._seed, self._cls_bias = seed, cls_bias
        self.mask_mode = mask_mode
        self.drop_empty_masks = drop_empty_masks
        self.max_batch = max_batch
        self._outs = {}
        self._frame_tables = {}
        self._window_tables = {}
        self._nms_tables = {}
        self.names = names if names is not None else {i: f"class{i}" for i in range(nc)}
        self._engines = {}

    def _engine(self, H, W, B, max_det=300):
        key = (H, W)
        eng = self._engines.get(key)
        # one vti_masks call handles max_batch * 512 instances (VTI_MASK_SLOTS_PER_FRAME): a predict() with a larger max_det
        # gets an engine with proportionally more batch slots, so every detection still gets its mask
        need = max(B, -(-B * max_det // 512), 1)
        if eng is None or eng.max_batch < need:
            eng = Engine(self.scale, self.nc, self._nm, self._reg_max, H, W, need, self.dtype)
            if self._blob is None:
                self._blob = random_weights(eng, self._seed, self._cls_bias)
            eng.load_weights(self._blob, self.device)
            self._engines[key] = eng
        return eng

    def _to_device_batch(self, source):
        if isinstance(source, torch.Tensor):
            t = source
        elif isinstance(source, (list, tuple)):
            t = torch.from_numpy(np.stack([np.asarray(s) for s in source]))
        else:
            t = torch.from_numpy(np.ascontiguousarray(source))
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4 or t.shape[-1] != 3 or t.dtype != torch.uint8:
            raise ValueError(f"source must be uint8 HxWx3 or BxHxWx3, got {t.dtype} {tuple(t.shape)}")
        dev = torch.device("cuda", self.device) if isinstance(self.device, int) else torch.device(self.device)
        return t.to(dev, non_blocking=True).contiguous()

    @staticmethod
    def _jpeg_files(source):
        """The files' bytes when `source` is JPEG data (bytes), a path to a JPEG file (str / os.PathLike), or a list / tuple of
        these, as Ultralytics' file sources are; None for array sources."""
        is_file = lambda s: isinstance(s, (bytes, bytearray, memoryview, str, os.PathLike))
        if is_file(source):
            source = [source]
        elif not (isinstance(source, (list, tuple)) and len(source) and any(is_file(s) for s in source)):
            return None
        files = []
        for k, s in enumerate(source):
            if not is_file(s):
                raise ValueError(f"a list source is either all frames or all JPEG files (bytes or paths); item {k} is {type(s).__name__}")
            if isinstance(s, (str, os.PathLike)):
                with open(s, "rb") as f:
                    s = f.read()
            files.append(bytes(s))
        return files

    def _decode_jpeg(self, files, rgb):
        """JPEG files -> (a device batch u8 [n,H0,W0,3], or DecodedFrames when the sizes differ; info i32 [n,4] on the device).
        A refused file raises here, before anything is launched."""
        dec = self._aux_engine()
        dev = torch.device("cuda", self.device) if isinstance(self.device, int) else torch.device(self.device)
        if dev.type == "cuda" and torch.cuda.is_available():
            torch.cuda.set_device(dev)
        got = dec.decode_jpeg(files, rgb=rgb, device=dev)
        if len(got) == 2:
            return got
        return DecodedFrames(got[0], got[1], got[2]), got[3]

    def _aux_engine(self):
        """The context of the calls that need no weights (vti_decode_jpeg, vti_convert_raw): the smallest plan serves every size."""
        dec = getattr(self, "_decoder", None)
        if dec is None:
            dec = self._decoder = Engine(self.scale, self.nc, self._nm, self._reg_max, 32, 32, 1, self.dtype)
        return dec

    @staticmethod
    def _raw_source(source):
        """The members when `source` is a RawFrames or a list / tuple of them; None for every other source."""
        if isinstance(source, RawFrames):
            return [source]
        if not (isinstance(source, (list, tuple)) and len(source) and any(isinstance(s, RawFrames) for s in source)):
            return None
        for k, s in enumerate(source):
            if not isinstance(s, RawFrames):
                raise ValueError(f"a list source is either all RawFrames or none; item {k} is {type(s).__name__}")
        return list(source)

    def _convert_raw(self, members):
        """RawFrames members -> the BGR device batch u8 [N,H0,W0,3] cap.read() would have delivered (vti_convert_raw per member,
        into one batch) when all have one size; a RawBatch for _predict_outputs_frames otherwise."""
        if any((m.H0, m.W0) != (members[0].H0, members[0].W0) for m in members):
            return RawBatch(members)
        dev = torch.device("cuda", self.device) if isinstance(self.device, int) else torch.device(self.device)
        if not torch.cuda.is_available():
            raise RuntimeError("RawFrames sources need a ROCm GPU (no CPU fallback; rawframes.to_bgr is the host specification)")
        torch.cuda.set_device(dev)
        eng = self._aux_engine()
        H0, W0 = members[0].H0, members[0].W0
        out = torch.empty((sum(m.n for m in members), H0, W0, 3), dtype=torch.uint8, device=dev)
        at = 0
        for m in members:
            d = m.data if isinstance(m.data, torch.Tensor) else torch.from_numpy(np.array(m.data))
            eng.convert_raw(d.to(dev, non_blocking=True), m.fmt, H0, W0, rgb=False, out=out[at:at + m.n])
            at += m.n
        return out

    def _raw_to_frame_buffer(self, eng, batch, table, buf, dev):
        """The RawBatch's bytes through one flat pinned staging buffer and one asynchronous H2D, then vti_convert_raw_frames into
        the frame-table buffer `buf`.  The raw table, the staging buffer and its device twin are cached per (engine, shapes, fmts)."""
        key = (id(eng), tuple(batch.shapes), tuple(batch.fmts))
        ent = getattr(self, "_raw_tables", {}).get(key)
        if ent is None:
            rt = eng.pack_raw_frames(batch.shapes, batch.fmts, dev)
            ent = (rt, torch.empty(max(rt.raw_bytes, 16), dtype=torch.uint8, pin_memory=True),
                   torch.empty(max(rt.raw_bytes, 16), dtype=torch.uint8, device=dev))
            self._raw_tables = {key: ent}      # one rig at a time, as the frame table
        rt, stage, rawbuf = ent
        flat = stage.numpy()
        for (_, data), off, fb in zip(batch.frames, rt.raw_offsets, rt.frame_bytes):
            flat[off:off + fb] = data.cpu().numpy() if isinstance(data, torch.Tensor) else data
        rawbuf.copy_(stage, non_blocking=True)
        eng.convert_raw_frames(rawbuf, rt, table, rgb=False, out=buf)

    @staticmethod
    def _raise_if_corrupt(info):
        """After the call: one read of the decoder's status words; a damaged scan is an error that names its file."""
        if info is None:
            return
        bad = torch.nonzero(info[:, 0]).flatten().cpu().tolist()
        if bad:
            raise ValueError(f"JPEG file {bad[0]} is damaged (its scan holds an invalid code, ends early or misses a restart marker)"
                             + (f"; so are files {bad[1:]}" if len(bad) > 1 else ""))

    @staticmethod
    def _differing_shapes(source):
        """[(H0, W0)] when `source` is a list / tuple of frames whose shapes are not all equal (Ultralytics then letterboxes every
        frame onto one imgsz canvas, LetterBox(auto=False)); None for everything that keeps the stacked path."""
        if isinstance(source, (DecodedFrames, RawBatch)):
            return list(source.shapes)
        if not isinstance(source, (list, tuple)) or len(source) < 2:
            return None
        shapes = [tuple(s.shape) if hasattr(s, "shape") else np.shape(s) for s in source]
        if all(x == shapes[0] for x in shapes):
            return None
        for x in shapes:
            if len(x) != 3 or x[2] != 3:
                raise ValueError(f"every frame of a list source must be uint8 HxWx3, got shape {x}")
        return [x[:2] for x in shapes]

    @staticmethod
    def _classes_arg(classes, nc):
        """Ultralytics' `classes=` -> None (every class) or the sorted tuple of distinct class ids; anything else is a ValueError."""
        if classes is None:
            return None
        if isinstance(classes, torch.Tensor):
            classes = classes.detach().cpu().numpy()
        arr = np.asarray(classes)
        if arr.size == 0:
            raise ValueError("predict: classes is empty (it would keep nothing); pass None for every class")
        if arr.dtype.kind not in "iu" or arr.ndim > 1:
            raise ValueError(f"predict: classes must be None, an int or a sequence of ints, got {classes!r}")
        ids = sorted({int(c) for c in arr.reshape(-1)})
        if ids[0] < 0 or ids[-1] >= nc:
            raise ValueError(f"predict: classes must lie in [0, {nc}), got {classes!r}")
        return tuple(ids)

    def _nms_table(self, eng, dev, rows):
        """The NMS table of `rows` (a tuple of NmsParams) on `eng`, packed and uploaded once per (engine, device, settings)."""
        key = (id(eng), str(dev), rows)
        ent = self._nms_tables.get(key)
        if ent is None:
            self._nms_tables.clear()        # one at a time, as the output set
            ent = self._nms_tables[key] = (eng, eng.pack_nms_table(rows, dev))
        return ent[1]

    @staticmethod
    def _canvas(imgsz):
        """The canvas of frames that differ in size (LetterBox(auto=False)): imgsz rounded up to the stride."""
        new_shape = (imgsz, imgsz) if isinstance(imgsz, int) else tuple(imgsz)
        H, W = (max(math.ceil(x / 32) * 32, 32) for x in new_shape)
        return H, W

    def _ragged_outputs(self, eng, dev, B, max_det, shapes, native_frames):
        """The cached output set of a table predict.  native_frames: the FrameTable of `shapes` for the ragged set
        (Engine.alloc_outputs(native_frames=)), cached per (engine, B, max_det, shapes); None for canvas-size masks."""
        okey = (id(eng), B, max_det, tuple(shapes) if native_frames is not None else None)
        o = self._outs.get(okey)
        if o is None:
            self._outs.clear()
            o = self._outs[okey] = eng.alloc_outputs(B, max_det, B * max_det, "bits", dev, native_frames=native_frames)
        return o

    def _predict_outputs_frames(self, source, shapes, conf, iou, max_det, imgsz, agnostic_nms, swap_rb, keep_frames=False,
                                retina_masks=False, nms=None):
        """_predict_outputs for frames of differing sizes: the frames are flattened into one pinned staging buffer, copied with one
        asynchronous H2D and run through one vti_predict_frames on the stride-rounded imgsz canvas.  The packed frame table, the
        staging buffer and its device twin are cached per (engine, shapes).  -> (engine, output set, FrameTable, (H, W)).
        keep_frames: as _predict_outputs -- the flat device buffer this predict consumed stays in _last_frames for a caller that
        draws on it.  retina_masks: vti_predict_frames_native into the ragged output set (Engine.alloc_outputs(native_frames=)),
        cached per (engine, B, max_det, shapes) as the uniform retina set is per native_hw.  nms: as _predict_outputs."""
        H, W = self._canvas(imgsz)
        B = len(shapes)
        eng = self._engine(H, W, B, max_det)
        dev = torch.device("cuda", self.device) if isinstance(self.device, int) else torch.device(self.device)
        table, buf = self._frame_buffer(eng, source, shapes, dev)
        o = self._ragged_outputs(eng, dev, B, max_det, shapes, table if retina_masks else None)
        eng.predict_frames_into(buf, table, o, conf, iou, max_det, agnostic_nms, swap_rb, self.mask_mode, "bits", native=bool(retina_masks),
                                nms=nms(eng, dev) if nms is not None else None)
        if keep_frames:
            self._last_frames = buf
        return eng, o, table, (H, W)

    def _frame_buffer(self, eng, source, shapes, dev):
        """The frames of a list source (or DecodedFrames / RawBatch) in the flat device buffer of their frame table on `eng`:
        -> (FrameTable, buffer).  The packed table, the pinned staging buffer and its device twin are cached per (engine, shapes)."""
        key = (id(eng), tuple(shapes))
        ent = self._frame_tables.get(key)
        if ent is None:
            table, _, total = eng.pack_frames(shapes, dev)
            self._frame_tables.clear()      # one rig at a time, as the output set
            ent = self._frame_tables[key] = (table, torch.empty(total, dtype=torch.uint8, pin_memory=True),
                                             torch.empty(total, dtype=torch.uint8, device=dev))
        table, stage, buf = ent
        if isinstance(source, DecodedFrames):       # already on the device, in this very layout (vti_decode_jpeg, layout 0)
            buf = source.buf
        elif isinstance(source, RawBatch):          # raw camera frames: converted on the device into this very layout
            self._raw_to_frame_buffer(eng, source, table, buf, dev)
        else:
            flat = stage.numpy()
            for f, (h, w), off in zip(source, shapes, table.byte_offsets):
                a = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
                if a.dtype != np.uint8:
                    raise ValueError(f"every frame of a list source must be uint8 HxWx3, got {a.dtype}")
                flat[off:off + 3 * h * w] = a.reshape(-1)
            buf.copy_(stage, non_blocking=True)
        return table, buf

    @staticmethod
    def _windows_arg(window, shapes):
        """predict's `window=` for frames of `shapes` -> [(x0, y0, w, h)] per frame: one (x0, y0, x1, y1) for every frame, or a list
        with one entry per frame (None: the whole frame); x1, y1 exclusive.  Anything else is a ValueError."""
        B = len(shapes)
        per_frame = isinstance(window, (list, tuple)) and len(window) > 0 and all(
            w is None or (not isinstance(w, (str, bytes)) and hasattr(w, "__len__")) for w in window)
        if not per_frame:
            window = [window] * B
        elif len(window) != B:
            raise ValueError(f"predict: window has {len(window)} entries but the batch has {B} frames")
        return [check_window(w, h0, w0, f"predict: window of frame {b}") for b, (w, (h0, w0)) in enumerate(zip(window, shapes))]

    def _predict_outputs_windows(self, source, shapes, windows, conf, iou, max_det, imgsz, agnostic_nms, swap_rb, keep_frames=False, nms=None):
        """_predict_outputs_frames(retina_masks=True) on one window (x0, y0, w, h) of each frame: one vti_predict_windows on the canvas
        predict() would pick for the contiguous crops -- LetterBox(auto=True) of the window when all windows have one size (a stacked
        batch of crops), the stride-rounded imgsz canvas otherwise.  source: a device batch u8 [B,H0,W0,3], or what
        _predict_outputs_frames takes.  -> (engine, ragged output set, WindowTable, (H, W))."""
        B = len(shapes)
        sizes = {(w[3], w[2]) for w in windows}
        H, W = letterbox_shape(*next(iter(sizes)), imgsz) if len(sizes) == 1 else self._canvas(imgsz)
        eng = self._engine(H, W, B, max_det)
        dev = torch.device("cuda", self.device) if isinstance(self.device, int) else torch.device(self.device)
        key = (id(eng), tuple(shapes), tuple(windows))
        wt = self._window_tables.get(key)
        if wt is None:
            wt = eng.pack_windows(shapes, windows, dev)
            self._window_tables.clear()     # one rig at a time, as the frame table
            self._window_tables[key] = wt
        if isinstance(source, torch.Tensor) and source.dim() == 4:      # a device batch: its bytes are the buffer where frames stay 16-byte aligned
            H0, W0 = shapes[0]
            if (3 * H0 * W0) % 16 == 0 or B == 1:
                buf = source.reshape(-1)
                if buf.numel() < wt.total_bytes:
                    buf = torch.cat((buf, buf.new_zeros(wt.total_bytes - buf.numel())))
            else:
                buf = torch.empty(wt.total_bytes, dtype=torch.uint8, device=source.device)
                for b, off in enumerate(wt.frames.byte_offsets):
                    buf[off:off + 3 * H0 * W0] = source[b].reshape(-1)
        else:
            buf = self._frame_buffer(eng, source, shapes, dev)[1]
        o = self._ragged_outputs(eng, dev, B, max_det, shapes, wt.frames)
        eng.predict_windows_into(buf, wt, o, conf, iou, max_det, agnostic_nms, swap_rb, self.mask_mode,
                                 nms=nms(eng, dev) if nms is not None else None)
        self._last_frames = buf if keep_frames else None
        return eng, o, wt, (H, W)

    def _predict_outputs(self, source, conf, iou, max_det, imgsz, agnostic_nms, swap_rb, retina_masks, keep_frames=False, nms=None):
        """The device half of predict(): enqueues the whole pipeline into the cached output set and returns
        (engine, output set, (B, H0, W0), letterbox (H, W)) without reading anything back (predict() and
        measure.StitchMeasurer both start here).  nms: None, or a callable (engine, device) -> (NmsTable, rows): the NMS then takes
        frame b's settings from row rows[b] of the table (Engine.nms_table) and max_det is the row stride and the upper bound."""
        if source is None:
            raise ValueError("predict() needs a source")
        frames = self._to_device_batch(source)
        B, H0, W0, _ = frames.shape
        H, W = letterbox_shape(H0, W0, imgsz)
        eng = self._engine(H, W, B, max_det)
        # the whole pipeline is enqueued without a host read in between (vti_predict: letterbox -> net -> NMS -> bit-packed
        # masks for up to B * max_det instances -> scale_boxes); the counts are read once, at the end, to cut the Results.
        # The output set (~1 GB for 64 frames x 300 slots of 640x640 bit masks) is allocated once per (engine, B, max_det) and
        # reused by later calls; what a Results object keeps are COPIES of its own rows (a few KB .. MB per frame).
        native_hw = (H0, W0) if retina_masks else None
        key = (id(eng), B, max_det, native_hw)
        o = self._outs.get(key)
        if o is None:
            self._outs.clear()              # one cached set at a time: a new shape replaces the old one
            o = self._outs[key] = eng.alloc_outputs(B, max_det, B * max_det, "bits", frames.device, native_hw=native_hw)
        eng.predict_into(frames, o, conf, iou, max_det, agnostic_nms, swap_rb, self.mask_mode, "bits", native=bool(retina_masks),
                         nms=nms(eng, frames.device) if nms is not None else None)
        # the device batch this predict consumed is kept only for a caller that draws on it (measure.py, annotate=): otherwise
        # the model holds no reference to it once the call returns
        self._last_frames = frames if keep_frames else None
        return eng, o, (B, H0, W0), (H, W)

    @torch.inference_mode()
    def predict(self, source=None, *, verbose=False, conf=0.25, iou=0.7, max_det=300, imgsz=640,
                agnostic_nms=False, swap_rb=True, retina_masks=False, mixed=False, window=None, classes=None, polygons=False,
                **_ignored):
        """Returns list[Results], one per frame.  `swap_rb=True` keeps Ultralytics' channel flip of
        ndarray sources.  retina_masks=True: masks at the frame size, Ultralytics'
        process_mask_native (8.1/8.2 scale_masks), made on the device from the frame-px boxes.
        A list / tuple of frames whose shapes differ is one batch too (vti_predict_frames): as Ultralytics does for such a list,
        every frame is letterboxed by its own gain onto one stride-rounded imgsz canvas (LetterBox(auto=False)); boxes and
        masks.xy come back in each frame's own pixels, masks.data at the canvas size.  retina_masks is a ValueError there unless
        mixed=True (keyword only, True or False) asks for it: then every frame's masks are made at that frame's own size
        (vti_predict_frames_native, the ragged mask buffer) and masks.data is [n, H0, W0] per frame, as Ultralytics returns for such
        a list.  On frames of one size, or without retina_masks, mixed changes nothing.
        JPEG sources -- bytes, a path (str / os.PathLike) or a list / tuple of these -- are decoded on the device
        (Engine.decode_jpeg); as with Ultralytics' file sources the network sees the file's R, G, B, so swap_rb does not apply to
        them.  orig_shape comes from the file's header; a refused file raises before any launch, a damaged one after the call.
        RawFrames sources -- one, or a list / tuple of them -- are raw camera buffers (YUYV, UYVY, NV12, NV21, I420, YV12) converted
        on the device (vti_convert_raw): the call is exactly predict on the BGR ndarray(s) rawframes.to_bgr gives, i.e. the frames
        cap.read() delivers without CAP_PROP_CONVERT_RGB = 0, with the same swap_rb meaning.  Members of differing sizes go
        through the frame table (vti_convert_raw_frames -> vti_predict_frames), members of one size keep the stacked path.
        polygons=True (keyword only, True or False): every Results.masks.xy / .xyn of the batch is made before predict returns --
        one vti_mask_polygons_frames call for a list whose frames differ in size (on the ragged frame-size rows with
        retina_masks=True, mixed=True), one vti_mask_polygons call over the live slots for frames of one size, and one copy of the
        points and offsets to the host; .xy / .xyn then return without touching the device.  Without it they are made per frame
        on first access, with the same values.
        classes (keyword only): None, an int, or a sequence / tensor of ints in [0, nc), as Ultralytics takes it: only anchors whose
        best class is in the set enter the NMS.  The filter runs on the device where Ultralytics' non_max_suppression has it --
        after the confidence test, before the greedy pass and max_det -- through a one-row NMS table (vti_set_nms_table); a bad
        value is a ValueError before a device is touched.  Without it the call takes the table-free path.
        window (keyword only): (x0, y0, x1, y1) for every frame, or a list with one entry per frame (None: the whole frame); x1 and y1
        are exclusive.  The network sees only that window of each frame, read in place (vti_predict_windows), and the Results are
        those of predict(crops, retina_masks=True, mixed=True, ...) on the contiguous crops frame[y0:y1, x0:x1] -- the same canvas,
        detections and scores -- carried back to the frame: orig_shape is the frame's, boxes are the crop's plus (x0, y0) (one f32
        add per coordinate), and masks are always frame-resolution rows [n, H0, 8 * ceil(W0 / 64)] with the crop's mask at the
        window's place and zeros elsewhere; masks.xy / polygons=True trace those rows.  A window that does not lie inside its frame
        with x0 < x1 and y0 < y1 is a ValueError before a device is touched."""
        classes = self._classes_arg(classes, self.nc)
        nms = None
        if classes is not None:
            row = NmsParams(float(conf), float(iou), int(max_det), bool(agnostic_nms), classes)
            nms = lambda eng, dev: (self._nms_table(eng, dev, (row,)), None)
        if not isinstance(mixed, (bool, np.bool_)):
            raise ValueError(f"predict: mixed must be True or False, got {mixed!r}")
        if not isinstance(polygons, (bool, np.bool_)):
            raise ValueError(f"predict: polygons must be True or False, got {polygons!r}")
        files = self._jpeg_files(source)
        info = None
        if files is not None:
            source, info = self._decode_jpeg(files, rgb=True)
            swap_rb = False
        raws = self._raw_source(source)
        if raws is not None:        # the BGR frames cap.read() would have delivered; swap_rb keeps its meaning for ndarray sources
            source = self._convert_raw(raws)
        shapes = self._differing_shapes(source)
        ragged = False
        if window is not None:
            if shapes is None and not isinstance(source, (DecodedFrames, RawBatch)):
                if source is None:
                    raise ValueError("predict() needs a source")
                if isinstance(source, (list, tuple)) and len(source) and all(isinstance(f, torch.Tensor) for f in source):
                    source = torch.stack(list(source))
                if not isinstance(source, torch.Tensor) or source.dim() not in (3, 4) or source.shape[-1] != 3 or source.dtype != torch.uint8:
                    source = np.stack([np.asarray(f) for f in source]) if isinstance(source, (list, tuple)) else np.asarray(source)
                    if source.ndim not in (3, 4) or source.shape[-1] != 3 or source.dtype != np.uint8:
                        raise ValueError(f"source must be uint8 HxWx3 or BxHxWx3, got {source.dtype} {tuple(source.shape)}")
                nB = 1 if len(source.shape) == 3 else int(source.shape[0])
                shapes = [tuple(int(v) for v in source.shape[-3:-1])] * nB
                windows = self._windows_arg(window, shapes)            # refused before a device is touched
                source = self._to_device_batch(source)
            else:
                windows = self._windows_arg(window, shapes)
            retina_masks, ragged = True, True
            eng, o, wt, (H, W) = self._predict_outputs_windows(source, shapes, windows, conf, iou, max_det, imgsz, agnostic_nms, swap_rb,
                                                               nms=nms)
            table, B = wt.frames, len(shapes)
        elif shapes is not None:
            if retina_masks and not mixed:
                raise ValueError("predict: retina_masks=True needs frames of one size; the frames of this list differ in shape "
                                 "(frame-resolution masks for mixed sizes are not supported)")
            ragged = bool(retina_masks)
            eng, o, table, (H, W) = self._predict_outputs_frames(source, shapes, conf, iou, max_det, imgsz, agnostic_nms, swap_rb,
                                                                  retina_masks=ragged, nms=nms)
            B = len(shapes)
        else:
            eng, o, (B, H0, W0), (H, W) = self._predict_outputs(source, conf, iou, max_det, imgsz, agnostic_nms, swap_rb, retina_masks,
                                                                 nms=nms)
            shapes, table = [(H0, W0)] * B, None
        self._raise_if_corrupt(info)
        dets, xyxy, masks = o["dets"], o["xyxy"], o["masks"]
        poly = None
        if polygons:                                       # the whole batch's polygons: one call, one copy to the host
            if table is not None:
                pts, po = eng.mask_polygons_frames(o, table, native=ragged)
            else:
                pts, po = eng.mask_polygons(masks, W0 if retina_masks else W, H0, W0, offsets=o["offsets"])
            host = torch.cat((pts.reshape(-1).view(torch.int32), po)).cpu().numpy()      # bits as int32, as Masks.xy copies them
            poly = (host[:pts.numel()].view(np.float32).reshape(-1, 2), host[pts.numel():])
        nonempty = None
        if self.drop_empty_masks and not retina_masks:     # m00 of every live slot straight from the bit-packed masks (vti_mask_stats_bits)
            nonempty = eng.mask_stats_bits(masks, H, W, offsets=o["offsets"])[:, 0] > 0
        cnt = o["counts"].cpu().tolist()
        off = o["offsets"].cpu().tolist()
        bases = o["mask_bases"].cpu().tolist() if ragged else None
        if self.drop_empty_masks and retina_masks and not ragged:     # native rows: pad bits are 0, so any set byte of a live slot is a pixel
            live = min(off[-1], masks.shape[0])
            nonempty = masks[:live].reshape(live, -1).amax(1) > 0
        out = []
        for b in range(B):
            H0, W0 = shapes[b]
            n = cnt[b]
            data = torch.cat((xyxy[b, :n], dets[b, :n, 4:6]), 1)
            keep = None
            if ragged:                                     # the frame's own rows: a view [n, H0, row_bytes] of the flat buffer
                mb, db = eng.frame_masks(masks, table, b, bases[b], n), dets[b, :n]
                if self.drop_empty_masks and n:            # the same "any set byte" rule, per frame
                    keep = mb.reshape(n, -1).amax(1) > 0
            else:
                mb, db = masks[off[b]:off[b] + n], dets[b, :n]
                if nonempty is not None and n:
                    keep = nonempty[off[b]:off[b] + n]
            if keep is not None:
                data, mb, db = data[keep], mb[keep], db[keep]
                n = int(data.shape[0])
            else:
                mb, db = mb.clone(), db.clone()
            m = Masks(mb, W0 if retina_masks else W, (H0, W0), eng) if n else None
            if m is not None and poly is not None:         # slot off[b] + i is instance i; the kept ones, in order
                which = range(cnt[b]) if keep is None else np.flatnonzero(keep.cpu().numpy()).tolist()
                m._xy = [poly[0][poly[1][off[b] + i]:poly[1][off[b] + i + 1]] for i in which]
            r = Results((H0, W0), self.names, Boxes(data, (H0, W0)), m, db)
            r._engine = eng
            out.append(r)
        return out

    __call__ = predict
