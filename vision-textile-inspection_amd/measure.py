"""process_frame's measurement record (measurement.py:240-510) as one batched device stage.

    params = MeasureParams.from_files("camera_calibration.json", "extrinsics.json")        measurement.py:130-140
    sm = StitchMeasurer(YOLO(path), params)
    records = sm.process_frames(frames)          # one dict per frame, as process_frame returns (main.py:211-226)
    mc = MultiCameraMeasurer(YOLO(path), [params_cam0, params_cam1, ...])
    records = mc.process_frames(frames, cameras) # a batch that mixes cameras: cameras[b] = the camera of frame b
    ck = StitchDistanceChecker(YOLO(path), CheckerParams.from_files(...))                  Utils/check_stitch_distance.py:176-222
    records = ck.process_frames(frames)          # the bench tool's numbers and info text per frame (vti_measure_checker)
    annotated, records = ck.process_frames(frames, annotate="all")     # and its picture (vti_annotate_checker)

The per-frame work (ROI filter, moments, fabric envelope, widths, row selection, proximity filter, distances, averages) runs in
libvti's vti_measure on the predict output set that is already on the device; the host reads back B small records once and keeps
only the reference's stateful smoothing (the two frame_buffer-long deques and their medians, measurement.py:474-484).

The annotated frame the reference also returns is drawn on request, for a selection of the batch (`annotate=`): libvti's
vti_annotate paints the overlay on the device batch predict consumed and the selected pictures come back in one copy; the text
(which holds the smoothed values) is returned as annotate.text_items and drawn by annotate.put_text where OpenCV is installed.
With `encode="jpeg"` the selected pictures are also encoded on the device (vti_encode_jpeg: the file cv2.imwrite would save of that
picture, jpeg.py) and only the files' bytes come back; the text still rides along as text_items; it is in the JPEG only with burn_text (below).
With `mixed=True` both also serve a list of frames whose sizes differ (vti_annotate_frames, vti_encode_jpeg_frames): every selected
frame is drawn and encoded at its own size, and the pictures or files still come back in one copy.
With `burn_text=True` the text IS in the pictures and files: the host rasterises each string once into a 1-bit stamp
(annotate.text_stamps), the stamps cross to the device and vti_stamp paints them onto the drawn pictures before they are copied or
encoded; `extra_text` adds the caller's own lines (main.py:302-309) the same way.
"""
import ctypes as C
import dataclasses
import functools
import inspect
import json
from collections import deque
from datetime import datetime

import numpy as np
import torch

from . import annotate as _annotate
from ._lib import (VTI_MEASURE_BAD_CAMERA, VTI_MEASURE_NO_FABRIC, VTI_MEASURE_NO_STITCHES, VTI_MEASURE_OK, VTI_STITCH_KEPT,
                   VTI_STITCH_NEAR, VTI_STITCH_SELECTED, VTI_STITCH_WIDTH, VtiCheckerParams, VtiMeasureParams)
from .consumer import rodrigues
from .engine import NmsParams, check_window

ERRORS = {VTI_MEASURE_NO_FABRIC: "Fabric not detected", VTI_MEASURE_NO_STITCHES: "No stitches detected",
          VTI_MEASURE_BAD_CAMERA: "Unknown camera"}     # the last one is this package's: a device-side index outside the table


@dataclasses.dataclass
class MeasureParams:
    """Calibration + config.py's measurement settings (the defaults are config.py's).  K f64 [3,3], dist f64 [5], R f64 [3,3]
    (cv2.Rodrigues of the extrinsics' rvec), t f64 [3].  roi = (x_min, y_min, x_max, y_max) in frame px."""
    K: np.ndarray
    dist: np.ndarray
    R: np.ndarray
    t: np.ndarray
    stitch_id: int = 0
    fabric_id: int = 1
    roi: tuple = (10, 300, 1270, 760)
    roi_enabled: bool = True
    min_stitches: int = 3
    max_px_distance: float = 250
    envelope_neighborhood: int = 3
    skip_cluster: bool = False
    two_row_threshold_px: float = 30
    frame_buffer: int = 8
    kmeans_iters: int = 10
    drop_empty: bool = False

    @classmethod
    def from_files(cls, calib_path, extr_path, **kw):
        """measurement.py:130-140: camera_matrix / dist_coeffs from the intrinsics file, rvec / tvec from the extrinsics file."""
        with open(calib_path) as f:
            calib = json.load(f)
        with open(extr_path) as f:
            extr = json.load(f)
        K = np.array(calib["camera_matrix"], dtype=np.float64)
        dist = np.array(calib["dist_coeffs"], dtype=np.float64).ravel()
        rvec = np.array(extr["rvec"], dtype=np.float64).reshape(3, 1)
        t = np.array(extr["tvec"], dtype=np.float64).reshape(3,)
        return cls(K=K, dist=dist, R=rodrigues(rvec), t=t, **kw)

    def to_c(self):
        p = VtiMeasureParams()
        for name, n in (("K", 9), ("dist", 5), ("R", 9), ("t", 3)):
            a = np.ascontiguousarray(np.asarray(getattr(self, name), dtype=np.float64).ravel())
            if a.size != n:
                raise ValueError(f"MeasureParams.{name}: expected {n} values, got {a.size}")
            setattr(p, name, (C.c_double * n)(*a.tolist()))
        p.max_px_distance = float(self.max_px_distance)
        p.two_row_threshold_px = float(self.two_row_threshold_px)
        p.stitch_id, p.fabric_id = int(self.stitch_id), int(self.fabric_id)
        p.roi_enabled = int(bool(self.roi_enabled))
        p.roi = (C.c_int32 * 4)(*(int(v) for v in self.roi))
        p.min_stitches = int(self.min_stitches)
        p.envelope_neighborhood = int(self.envelope_neighborhood)
        p.skip_cluster = int(bool(self.skip_cluster))
        p.kmeans_iters = int(self.kmeans_iters)
        p.drop_empty = int(bool(self.drop_empty))
        p.frame_buffer = int(self.frame_buffer)
        return p


@dataclasses.dataclass
class CheckerParams:
    """Calibration + the stitch-distance checker's settings (the defaults are check_stitch_distance.py:20-39's module constants).
    K, dist, R, t as MeasureParams.  The checker has no ROI and no two-row threshold."""
    K: np.ndarray
    dist: np.ndarray
    R: np.ndarray
    t: np.ndarray
    stitch_id: int = 0
    fabric_id: int = 1
    min_stitches: int = 3
    max_px_distance: float = 150
    envelope_neighborhood: int = 3
    skip_cluster: bool = False
    frame_buffer: int = 8
    kmeans_iters: int = 10
    drop_empty: bool = False

    @classmethod
    def from_files(cls, calib_path, extr_path, **kw):
        """check_stitch_distance.py:188-201: the same two files StitchMeasurementApp reads."""
        m = MeasureParams.from_files(calib_path, extr_path)
        return cls(K=m.K, dist=m.dist, R=m.R, t=m.t, **kw)

    def to_c(self):
        p = VtiCheckerParams()
        for name, n in (("K", 9), ("dist", 5), ("R", 9), ("t", 3)):
            a = np.ascontiguousarray(np.asarray(getattr(self, name), dtype=np.float64).ravel())
            if a.size != n:
                raise ValueError(f"CheckerParams.{name}: expected {n} values, got {a.size}")
            setattr(p, name, (C.c_double * n)(*a.tolist()))
        p.max_px_distance = float(self.max_px_distance)
        p.stitch_id, p.fabric_id = int(self.stitch_id), int(self.fabric_id)
        p.min_stitches = int(self.min_stitches)
        p.envelope_neighborhood = int(self.envelope_neighborhood)
        p.skip_cluster = int(bool(self.skip_cluster))
        p.kmeans_iters = int(self.kmeans_iters)
        p.drop_empty = int(bool(self.drop_empty))
        p.frame_buffer = int(self.frame_buffer)
        return p


class CameraStream:
    """One camera's smoothing state: the reference's two frame_buffer-long deques (measurement.py:474-484)."""

    def __init__(self, frame_buffer):
        self.dist = deque(maxlen=frame_buffer)
        self.width = deque(maxlen=frame_buffer)

    def record(self, f64, i32):
        """measurement.py:285-287, 333-337 (errors: nothing appended) and 469-510 (averages -> deques -> medians)."""
        status = int(i32[0])
        if status in ERRORS:
            return {'edge_distance_mm': None, 'stitch_width_mm': None, 'stitch_count': 0, 'timestamp': datetime.now(),
                    'error': ERRORS[status]}
        avg_dist = None if np.isnan(f64[0]) else float(f64[0])
        avg_width = None if np.isnan(f64[1]) else float(f64[1])
        smooth_dist = smooth_width = None
        if avg_dist is not None:
            self.dist.append(avg_dist)
            smooth_dist = float(np.median(self.dist))
        if avg_width is not None:
            self.width.append(avg_width)
            smooth_width = float(np.median(self.width))
        return {'edge_distance_mm': smooth_dist, 'stitch_width_mm': smooth_width, 'stitch_count': int(i32[4]),
                'timestamp': datetime.now()}


def _bool_keyword(name, value):
    """A keyword-only switch of process_frames: True or False, anything else is a ValueError."""
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError(f"process_frames: {name} must be True or False, got {value!r}")
    return bool(value)


def _mixed_keyword(public):
    """process_frames' keyword-only `mixed`, `annotate_native`, `burn_text`, `extra_text` and `rasterise`.  `public` carries the signature and the documentation -- its parameter list, which ends
    in annotate, encode, jpeg_quality for positional callers and for inspect.signature, stays as it was -- and the work is in the
    class's _process_frames, which takes the same parameters by name and the keyword-only ones next to them: arguments all the way
    down, no state on the measurer."""
    sig = inspect.signature(public)

    @functools.wraps(public)
    def process_frames(self, *args, mixed=False, burn_text=False, extra_text=None, rasterise=None, annotate_native=False, **kw):
        mixed, annotate_native = _bool_keyword("mixed", mixed), _bool_keyword("annotate_native", annotate_native)
        # the two measurers' keyword-only window (StitchMeasurer: window=, MultiCameraMeasurer: windows=) and window_margin; a class
        # without _window_keyword does not take them (sig.bind then refuses them as any unknown keyword)
        wkw, name = {}, getattr(self, "_window_keyword", None)
        if name is not None:
            if name in kw:
                wkw["window"] = kw.pop(name)
            if "window_margin" in kw:
                wkw["window_margin"] = kw.pop("window_margin")
        bound = sig.bind(self, *args, **kw)             # a TypeError for a bad call, as calling `public` would give
        bound.apply_defaults()
        named = dict(bound.arguments)
        del named["self"]
        return self._process_frames(mixed=mixed, burn_text=burn_text, extra_text=extra_text, rasterise=rasterise,
                                    annotate_native=annotate_native, **named, **wkw)
    return process_frames


def _annotate_native_keyword(public):
    """MultiCameraChecker.process_frames' keyword-only `annotate_native`, carried as _mixed_keyword carries its keywords: `public` keeps
    the parameter list inspect.signature shows, the work is in the class's _process_frames, which takes the keyword next to them."""
    sig = inspect.signature(public)

    @functools.wraps(public)
    def process_frames(self, *args, annotate_native=False, **kw):
        annotate_native = _bool_keyword("annotate_native", annotate_native)
        bound = sig.bind(self, *args, **kw)             # a TypeError for a bad call, as calling `public` would give
        bound.apply_defaults()
        named = dict(bound.arguments)
        del named["self"]
        return self._process_frames(annotate_native=annotate_native, **named)
    return process_frames


class _Deferred(list):
    """[(frame index, None, per-slot rows)] of a selection whose drawn pictures wait on the device for their text (burn_text): the
    strings hold the smoothed values, which exist once the records are built.  shapes[k]: picture k's (H0, W0); finish(stamps per
    picture) paints them (vti_stamp) and returns the pictures, or with encode the files, as _annotated would have."""
    shapes = finish = None


def _burn_refusals(annotate, burn_text, extra_text, rasterise):
    """What process_frames refuses about the text in the pictures, before anything is predicted."""
    if burn_text and annotate is None:
        raise ValueError("process_frames: burn_text needs annotate (the text is burned into the annotated selection)")
    if extra_text is not None and not burn_text:
        raise ValueError("process_frames: extra_text needs burn_text=True (without it the text stays with the caller)")
    if burn_text and rasterise is None:
        import cv2  # noqa: F401  (ImportError: no OpenCV and no rasteriser of the caller's)


def _extra_items(extra_text, b, record):
    """The caller's own items for frame b: extra_text[b], or extra_text(b, record) when it is callable (a line that quotes the record
    this very call built, as main.py:297-309 does)."""
    if extra_text is None:
        return []
    return list(extra_text(b, record) if callable(extra_text) else extra_text.get(b, []))


def _burned(annotated, items, rasterise):
    """annotated with the items of picture k burned into it: [(frame index, picture or file, items[k])].  Without burn_text the
    pictures are already there and nothing is painted."""
    if isinstance(annotated, _Deferred):
        pics = annotated.finish([_annotate.text_stamps(it, h, w, rasterise) for it, (h, w) in zip(items, annotated.shapes)])
    else:
        pics = [pic for _, pic, _ in annotated]
    return [(a[0], pic, it) for a, pic, it in zip(annotated, pics, items)]


class _DeviceStage:
    """predict + one measure call + one device -> host read of the B frame records."""

    _mixed_sizes = True         # the stage has a frame-table form (vti_measure_frames)

    def __init__(self, model):
        self.model = model
        self._res = {}

    def _measure(self, eng, o, params, H0, W0, **kw):
        """The stage's one measure call on the predict outputs (Engine.measure's contract)."""
        return eng.measure(o, params, H0, W0, **kw)

    @staticmethod
    def _per_camera_nms(n_cams, conf, iou, max_det):
        """conf, iou, max_det of a rig's process_frames, each a scalar or a sequence with one entry per camera -> (conf, iou, max_det,
        nms_rows): all scalars give them back with nms_rows None (the table-free predict); otherwise nms_rows is one NmsParams per
        camera, max_det the largest one (the row stride of the output set) and conf, iou what the call passes along unused.  A
        sequence of another length is a ValueError."""
        seq = lambda v: isinstance(v, (list, tuple, np.ndarray, torch.Tensor)) and np.ndim(v) == 1
        if not any(seq(v) for v in (conf, iou, max_det)):
            return conf, iou, max_det, None
        per = {}
        for name, v in (("conf", conf), ("iou", iou), ("max_det", max_det)):
            vals = [x.item() if hasattr(x, "item") else x for x in v] if seq(v) else [v] * n_cams
            if len(vals) != n_cams:
                raise ValueError(f"process_frames: {name} has {len(vals)} entries but the rig has {n_cams} cameras "
                                 "(a scalar, or one entry per camera)")
            per[name] = vals
        rows = tuple(NmsParams(float(c), float(i), int(m), False, None) for c, i, m in zip(per["conf"], per["iou"], per["max_det"]))
        if min(r.max_det for r in rows) < 1:
            raise ValueError("process_frames: every max_det must be >= 1")
        return rows[0].conf, rows[0].iou, max(r.max_det for r in rows), rows

    @torch.inference_mode()
    def _frame_records(self, frames, params, cameras, conf, iou, max_det, imgsz, retina_masks, annotate=None, encode=None,
                       jpeg_quality=95, mixed=False, rows=False, burn_text=False, extra_text=None, rasterise=None, nms_rows=None,
                       window=None, window_margin=32, window_params=None, annotate_native=False):
        """-> (f64 [B,2], i32 [B,6]) on the host, and with `annotate` a third item: [(frame index, BGR ndarray, per-slot rows)] of the
        selected frames (encode="jpeg": the JPEG file's bytes in place of the ndarray), and a fourth: their height H0 (frames of
        differing sizes, which `mixed` allows with annotate: the list of every frame's H0).  params /
        cameras as Engine.measure takes them; a callable `params` is called with (engine, device) once the outputs exist (the
        camera table needs both).  rows (without annotate): a third item, every frame's per-slot rows as `_slot_rows` gives them.
        burn_text: the third item is a _Deferred -- the pictures are drawn but neither copied nor encoded yet.
        nms_rows (with cameras): one NmsParams per camera -- the predict runs under their NMS table with `cameras` as the row index,
        and max_det is the output set's row stride.
        window: None, or what _frame_windows takes -- the predict then sees one window of each frame (vti_predict_windows) and the
        measurement runs on its frame-px boxes and frame-resolution masks (native rows, whatever retina_masks says);
        window_params(b): frame b's MeasureParams, for "roi".
        annotate_native (with mixed, on frames of differing sizes): annotate may go with retina_masks or a window -- the pictures are
        drawn from the ragged frame-resolution rows (vti_annotate_frames_native).  On frames of one size it changes nothing."""
        nms = None
        if nms_rows is not None:
            nms = lambda eng, dev: (self.model._nms_table(eng, dev, nms_rows), np.asarray(cameras))
        if encode is not None:
            if encode != "jpeg":
                raise ValueError(f'process_frames: encode must be None or "jpeg", got {encode!r}')
            if annotate is None:
                raise ValueError("process_frames: encode needs annotate (the frames to encode are the annotated selection)")
            if isinstance(jpeg_quality, bool) or not isinstance(jpeg_quality, (int, np.integer)) or not 1 <= jpeg_quality <= 100:
                raise ValueError(f"process_frames: jpeg_quality must be an integer in 1..100, got {jpeg_quality!r}")
        _burn_refusals(annotate, burn_text, extra_text, rasterise)
        files = self.model._jpeg_files(frames)
        info = None
        if files is not None:       # the batch cap.read() would have delivered: the files decoded to BGR on the device
            frames, info = self.model._decode_jpeg(files, rgb=False)
        raws = self.model._raw_source(frames)
        if raws is not None:        # raw camera buffers (RawFrames): converted on the device to that same BGR batch
            frames = self.model._convert_raw(raws)
        shapes = self.model._differing_shapes(frames)
        table = None
        if window is not None:
            retina_masks = True
            if shapes is not None:
                if annotate is not None and not (mixed and annotate_native):
                    raise ValueError("process_frames: retina_masks=True needs frames of one size; the frames of this list differ in shape")
                wins = self._frame_windows(window, window_margin, shapes, window_params)
                eng, o, wt, _ = self.model._predict_outputs_windows(frames, shapes, wins, conf, iou, max_det, imgsz, False, False,
                                                                    keep_frames=annotate is not None, nms=nms)
                table, B, H0, W0 = wt.frames, len(shapes), None, None
            else:
                if isinstance(frames, (list, tuple)):
                    frames = torch.stack(list(frames)) if isinstance(frames[0], torch.Tensor) else np.stack([np.asarray(f) for f in frames])
                shp = tuple(frames.shape) if hasattr(frames, "shape") else np.shape(frames)
                if len(shp) not in (3, 4) or shp[-1] != 3:
                    raise ValueError(f"source must be uint8 HxWx3 or BxHxWx3, got shape {shp}")
                B, (H0, W0) = (1 if len(shp) == 3 else int(shp[0])), (int(shp[-3]), int(shp[-2]))
                wins = self._frame_windows(window, window_margin, [(H0, W0)] * B, window_params)      # refused before a device is touched
                batch = self.model._to_device_batch(frames)
                eng, o, wt, _ = self.model._predict_outputs_windows(batch, [(H0, W0)] * B, wins, conf, iou, max_det, imgsz, False, False,
                                                                    nms=nms)
                self.model._last_frames = batch if annotate is not None else None
                # frames of one size: the ragged buffer IS the uniform native layout (slot offsets[b] + i, all slots live), so the
                # uniform native measure and annotate calls take it as a view
                u = o.get("_uniform")
                if u is None:
                    rb = eng.mask_native_layout(H0, W0)["row_bytes"]
                    u = o["_uniform"] = dict(o, masks=o["masks"].view(-1, H0, rb))
                o = u
        elif shapes is not None:
            if not self._mixed_sizes:
                raise ValueError(f"process_frames: {type(self).__name__} needs frames of one size; the frames of this list differ in shape")
            if annotate is not None and not mixed:
                raise ValueError("process_frames: annotate needs frames of one size; the frames of this list differ in shape "
                                 "(vti_annotate has no frame-table form)")
            # mixed + retina_masks measures; its pictures are drawn from the ragged rows, on request (annotate_native)
            if retina_masks and (not mixed or (annotate is not None and not annotate_native)):
                raise ValueError("process_frames: retina_masks=True needs frames of one size; the frames of this list differ in shape")
            eng, o, table, _ = self.model._predict_outputs_frames(frames, shapes, conf, iou, max_det, imgsz, False, False,
                                                                  keep_frames=annotate is not None, retina_masks=bool(retina_masks),
                                                                  nms=nms)
            B, H0, W0 = len(shapes), None, None
        else:
            eng, o, (B, H0, W0), _ = self.model._predict_outputs(frames, conf, iou, max_det, imgsz, False, False, retina_masks,
                                                                 keep_frames=annotate is not None, nms=nms)
        self.model._raise_if_corrupt(info)
        sel = None
        if annotate is not None:
            sel = np.arange(B) if isinstance(annotate, str) and annotate == "all" else np.asarray(annotate)
            if isinstance(annotate, str) and annotate != "all":
                raise ValueError('process_frames: annotate must be None, "all" or a sequence of frame indices')
            if sel.ndim != 1 or sel.size < 1 or sel.dtype.kind not in "iu" or sel.min() < 0 or sel.max() >= B:
                raise ValueError(f"process_frames: annotate must name frames in [0, {B})")
        key = (id(o), B)
        res = self._res.get(key)
        if res is None:           # one buffer for both records: a single device -> host read
            buf = torch.empty(B * 16 + B * 24, dtype=torch.uint8, device=o["dets"].device)
            res = dict(buf=buf, frame_f64=buf[:B * 16].view(torch.float64).view(B, 2),
                       frame_i32=buf[B * 16:].view(torch.int32).view(B, 6))
            self._res = {key: res}
        if callable(params):
            params = params(eng, o["dets"].device)
        want_rows = sel is not None or bool(rows)
        if table is None and cameras is None:
            r = self._measure(eng, o, params, H0, W0, native=bool(retina_masks), stitch_rows=want_rows, result=res)
        else:
            r = self._measure(eng, o, params, H0, W0, native=bool(retina_masks), stitch_rows=want_rows, result=res, cameras=cameras,
                              frames=table)
        if want_rows:             # measure() allocated the per-slot rows into its copy of the dict: keep them for the next call
            res.update(stitch_f64=r["stitch_f64"], stitch_i32=r["stitch_i32"])
        host = res["buf"].cpu().numpy()
        f64, i32 = host[:B * 16].view(np.float64).reshape(B, 2), host[B * 16:].view(np.int32).reshape(B, 6)
        if sel is None:
            return (f64, i32, self._slot_rows(o, res, np.arange(B))) if rows else (f64, i32)
        got = (f64, i32, self._annotated(eng, o, res, params, cameras, sel, bool(retina_masks),
                                         int(jpeg_quality) if encode else None, table, bool(burn_text)),
               H0 if table is None else [h for h, _ in shapes])
        return got + (self._slot_rows(o, res, np.arange(B)),) if rows else got      # rows next to annotate: a fifth item, every frame's

    @staticmethod
    def _frame_windows(window, margin, shapes, params_of):
        """process_frames' window -> [(x0, y0, w, h)] per frame.  window: (x0, y0, x1, y1) for every frame, a list with one entry per
        frame (None: the whole frame), or "roi": frame b's clamped ROI (measurement.py:220-238, inclusive bounds) grown by `margin` px
        on every side and clipped to the frame; a disabled or degenerate ROI means the whole frame.  Bad values are a ValueError."""
        if isinstance(margin, (bool, np.bool_)) or not isinstance(margin, (int, np.integer)) or margin < 0:
            raise ValueError(f"process_frames: window_margin must be an integer >= 0, got {margin!r}")
        B = len(shapes)

        def roi(b):
            h0, w0 = shapes[b]
            r = _annotate.roi_bounds(h0, w0, params_of(b))
            if r is None:
                return None
            return max(0, r[0] - margin), max(0, r[1] - margin), min(w0, r[2] + 1 + margin), min(h0, r[3] + 1 + margin)
        if isinstance(window, str):
            if window != "roi":
                raise ValueError(f'process_frames: window must be None, "roi", (x0, y0, x1, y1) or one of these per frame, got {window!r}')
            window = ["roi"] * B
        per_frame = isinstance(window, (list, tuple)) and len(window) > 0 and all(
            w is None or isinstance(w, str) or hasattr(w, "__len__") for w in window)
        if not per_frame:
            window = [window] * B
        elif len(window) != B:
            raise ValueError(f"process_frames: the window list has {len(window)} entries but the batch has {B} frames")
        out = []
        for b, w in enumerate(window):
            if isinstance(w, str):
                if w != "roi":
                    raise ValueError(f'process_frames: window of frame {b}: a string must be "roi", got {w!r}')
                w = roi(b)
            out.append(check_window(w, shapes[b][0], shapes[b][1], f"process_frames: window of frame {b}"))
        return out

    def _annotated(self, eng, o, res, params, cameras, sel, native, jpeg_quality=None, table=None, burn=False):
        """vti_annotate on the batch predict consumed; the selected pictures in one device -> host copy, and of the per-slot rows only
        those of the selected frames.  jpeg_quality: the pictures go through vti_encode_jpeg first and the copy is of the files'
        bytes (one read of the offsets, one of out[:offsets[n]]).  table: the FrameTable of a batch whose frames differ in size --
        vti_annotate_frames and vti_encode_jpeg_frames; the one copy is then of the flat buffer, sliced into [H0, W0, 3] arrays.
        burn: the pictures stay on the device and the per-slot rows come back in a _Deferred, whose finish() stamps, encodes and
        copies once the caller has built the text."""
        ann = self._draw(eng, self.model._last_frames, o, res, params, sel, cameras, native, table)
        self.model._last_frames = None            # the launches are enqueued: the batch need not outlive the call
        if burn:
            rows = self._slot_rows(o, res, np.unique(sel))
            later = _Deferred((int(b), None, rows[int(b)]) for b in sel)
            later.shapes = list(ann["shapes"]) if table is not None else [tuple(int(v) for v in ann["frames"].shape[1:3])] * len(sel)
            later.finish = lambda stamps: self._pictures(eng, ann, len(sel), jpeg_quality, table, stamps, later.shapes)
            return later
        pics = self._pictures(eng, ann, len(sel), jpeg_quality, table)
        rows = self._slot_rows(o, res, np.unique(sel))
        return [(int(b), pics[k], rows[int(b)]) for k, b in enumerate(sel)]

    @staticmethod
    def _pictures(eng, ann, n, jpeg_quality, table, stamps=None, shapes=None):
        """The n drawn pictures of `ann` on the host (jpeg_quality: their files), with `stamps` (per picture) painted first."""
        if stamps is not None:
            pictures = ann["buf"] if table is not None else ann["frames"]
            eng.stamp(pictures, eng.pack_stamps(stamps, shapes, pictures.device), table=ann["table"] if table is not None else None)
        if jpeg_quality is None and table is not None:
            flat = ann["buf"].cpu().numpy()
            pics = [flat[at:at + 3 * h * w].reshape(h, w, 3) for (h, w), at in zip(ann["shapes"], ann["byte_offsets"])]
        elif jpeg_quality is None:
            pics = ann["frames"].cpu().numpy()
        else:
            if table is not None:
                data, off = eng.encode_jpeg(ann["buf"], quality=jpeg_quality, table=ann["table"])
            else:
                data, off = eng.encode_jpeg(ann["frames"], quality=jpeg_quality)
            off = off.cpu().numpy()
            data = data[:int(off[-1])].cpu().numpy().tobytes()
            pics = [data[off[k]:off[k + 1]] for k in range(n)]
        return pics

    def _draw(self, eng, frames, o, res, params, sel, cameras, native, table):
        """The stage's one drawing call on the batch predict consumed (Engine.annotate's contract)."""
        return eng.annotate(frames, o, res, params, sel, cameras=cameras, native=native, table=table)

    @staticmethod
    def _slot_rows(o, res, uniq):
        """{frame b: dict(f64 [n,7], flags [n], rank [n])} of the frames `uniq`: the per-slot rows of their live slots, on the host."""
        dev = o["dets"].device
        cnt_off = torch.cat((o["counts"], o["offsets"])).cpu().numpy()
        B = o["counts"].shape[0]
        cap = o["masks"].shape[0]
        spans = {int(b): (min(int(cnt_off[B + b]), cap), min(int(cnt_off[B + b]) + int(cnt_off[b]), cap)) for b in uniq}
        idx = np.concatenate([np.arange(lo, hi) for lo, hi in spans.values()] + [np.zeros(0, np.int64)]).astype(np.int64)
        di = torch.from_numpy(idx).to(dev)
        sf = res["stitch_f64"].index_select(0, di).cpu().numpy()
        si = res["stitch_i32"].index_select(0, di).cpu().numpy()
        rows, at = {}, 0
        for b, (lo, hi) in spans.items():
            rows[b] = dict(f64=sf[at:at + hi - lo], flags=si[at:at + hi - lo, 0], rank=si[at:at + hi - lo, 1])
            at += hi - lo
        return rows

    @staticmethod
    def _with_text(annotated, records, i32, min_stitches, H0, extra_text=None, rasterise=None):
        """[(frame index, picture, rows)] -> [(frame index, picture, text_items)] with the strings built from the frames' records
        (picture: the BGR ndarray of height H0, or its JPEG file's bytes).  H0: one height, or every frame's own.  A _Deferred
        selection (burn_text) gets its items, followed by extra_text's for that frame, burned in before the pictures come back."""
        items = []
        for b, pic, rows in annotated:
            rows = dict(rows, status=i32[b, 0], n_stitch=i32[b, 1], n_fabric=i32[b, 2], n_dist=i32[b, 4], n_width=i32[b, 5])
            h0 = H0[b] if isinstance(H0, (list, tuple)) else H0
            items.append(_annotate.text_items(records[b], rows, h0, min_stitches(b)) + _extra_items(extra_text, b, records[b]))
        return _burned(annotated, items, rasterise)


class StitchMeasurer(_DeviceStage):
    """StitchMeasurementApp.process_frame without the camera: model = a vti_amd YOLO, params = MeasureParams.
    The smoothing deques live here, so consecutive calls continue one stream of frames, as the reference's app does."""

    def __init__(self, model, params, frame_buffer=8):
        super().__init__(model)
        self.params = dataclasses.replace(params, frame_buffer=int(frame_buffer), drop_empty=bool(model.drop_empty_masks))
        self._stream = CameraStream(frame_buffer)
        self.frame_buf_dist, self.frame_buf_width = self._stream.dist, self._stream.width
        self._record = self._stream.record
        self._cp = self.params.to_c()

    @_mixed_keyword
    def process_frames(self, frames, conf=0.20, iou=0.25, max_det=200, imgsz=960, retina_masks=False, annotate=None, encode=None,
                       jpeg_quality=95):
        """frames: BGR uint8 [B,H0,W0,3] (or one [H0,W0,3]) as the camera gives them, or a list of JPEG files (bytes) as a
        motion-JPEG camera delivers them: they are decoded on the device to the BGR batch cap.read() would have returned.
        RawFrames (one, or a list of them) are a camera's raw YUV buffers, converted on the device to that same BGR batch.
        The reference predicts on the RGB conversion
        with Ultralytics' channel flip of ndarray sources, i.e. the network sees the BGR frame: swap_rb=False here does the same.
        Returns one record per frame, in frame order, with the smoothing applied frame by frame.
        annotate: "all" or a sequence of frame indices -> (annotated, records): annotated = [(frame index, BGR ndarray H0 x W0 x 3 with
        the reference's overlay, text_items)] for the selection (drawn on the device, one copy to the host; the text is
        annotate.text_items', for annotate.put_text), records exactly as without it.
        encode="jpeg" (with annotate): each annotated item is (frame index, bytes, text_items), the bytes being the JPEG file
        cv2.imwrite(path, picture) saves at jpeg_quality (jpeg.encode, byte for byte), encoded on the device; the text is NOT in
        that picture, it still comes as text_items.  Any other encode, or encode without annotate, is a ValueError.
        mixed (keyword only, default False): True lets a LIST of frames whose sizes differ (ndarrays or JPEG files) be combined with
        annotate and encode: every selected frame is drawn (vti_annotate_frames) and encoded (vti_encode_jpeg_frames) at its own
        size, a picture is the [H0, W0, 3] ndarray of its frame, and text_items are placed by each frame's own height.  Without it
        such a list with annotate is refused, as before; on frames of one size it changes nothing.  mixed=True also lets
        retina_masks=True measure such a list (vti_predict_frames_native -> vti_measure_frames_native: every frame's masks at its own
        size); without mixed, or together with annotate, retina_masks=True with differing sizes stays refused.
        burn_text (keyword only, default False; needs annotate): True burns the text into the selected pictures on the device before
        they are copied or encoded (annotate.text_stamps -> vti_stamp), so the ndarray, or with encode="jpeg" the file, carries what
        cv2.putText would have written; the tuple stays (frame index, picture or bytes, items).  extra_text (needs burn_text): {frame
        index: [items in text_items' form]}, or a callable (frame index, the frame's record) -> items for lines that quote the record
        this call builds: the caller's own lines (main.py:297-309), burned in after the frame's own and appended to its items.  rasterise (keyword only): rasterise(canvas, item) in annotate.text_stamps' sense; default cv2.putText
        (ImportError, before anything is predicted, where OpenCV is not installed).  The records are the same with and without it.
        window (keyword only): None, (x0, y0, x1, y1) with x1, y1 exclusive, or "roi" -- the params' ROI clamped to the frame, grown by
        window_margin (keyword only, default 32) px and clipped to the frame; a disabled ROI means the whole frame.  The network then
        sees only that window of every frame, read in place (vti_predict_windows), at the canvas predict would pick for the crop;
        boxes come back in frame px and the masks as frame-resolution rows, and the records are those of the native measurement on
        them.  annotate and encode work on frames of one size; a list of differing sizes with annotate needs annotate_native.
        annotate_native (keyword only, default False; with mixed=True): True lets a list of differing sizes combine annotate (and
        encode, burn_text) with retina_masks=True or a window: every selected frame is drawn at its own size from its
        frame-resolution masks (vti_predict_frames_native or vti_predict_windows -> vti_measure_frames_native ->
        vti_annotate_frames_native), one copy to the host as with letterbox masks.  Without it those combinations stay refused; on
        frames of one size it changes nothing."""

    _window_keyword = "window"

    def _process_frames(self, frames, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality, mixed, burn_text=False,
                        extra_text=None, rasterise=None, window=None, window_margin=32, annotate_native=False):
        got = self._frame_records(frames, self._cp, None, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality, mixed,
                                  burn_text=burn_text, extra_text=extra_text, rasterise=rasterise, window=window,
                                  window_margin=window_margin, window_params=lambda b: self.params, annotate_native=annotate_native)
        f64, i32 = got[:2]
        records = [self._record(f64[b], i32[b]) for b in range(len(f64))]
        if annotate is None:
            return records
        return self._with_text(got[2], records, i32, lambda b: self.params.min_stitches, got[3], extra_text, rasterise), records

    def process_frame(self, frame, annotate=False, **kw):
        """One frame: the record process_frame returns; annotate=True: the reference's tuple (annotated BGR ndarray, record), the text
        drawn too where OpenCV is installed (annotate.put_text; without it the picture carries everything but the text)."""
        if not annotate:
            return self.process_frames(np.asarray(frame)[None], **kw)[0]
        annotated, records = self.process_frames(np.asarray(frame)[None], annotate=[0], **kw)
        _, pic, items = annotated[0]
        try:
            _annotate.put_text(pic, items)
        except ImportError:
            pass
        return pic, records[0]


class MultiCameraMeasurer(_DeviceStage):
    """StitchMeasurer for batches that mix cameras: params_by_camera[c] = camera c's MeasureParams (calibration, ROI, thresholds).
    One predict, one vti_measure_cameras and one device -> host read per batch; every camera keeps its own smoothing stream, so the
    records equal those of one StitchMeasurer per camera, each fed only its camera's frames in the same order."""

    def __init__(self, model, params_by_camera, frame_buffer=8):
        super().__init__(model)
        self.params = [dataclasses.replace(p, frame_buffer=int(frame_buffer), drop_empty=bool(model.drop_empty_masks))
                       for p in params_by_camera]
        if not self.params:
            raise ValueError("MultiCameraMeasurer: at least one camera")
        self.streams = [CameraStream(frame_buffer) for _ in self.params]
        self._tables = {}

    def _table(self, eng, device):
        key = (id(eng), str(device))
        if key not in self._tables:       # packed, validated and uploaded once per engine and device
            self._tables[key] = (eng, eng.pack_cameras(self.params, device))
        return self._tables[key][1]

    @_mixed_keyword
    def process_frames(self, frames, cameras, conf=0.20, iou=0.25, max_det=200, imgsz=960, retina_masks=False, annotate=None,
                       encode=None, jpeg_quality=95):
        """frames as StitchMeasurer.process_frames, or a list of frames whose sizes differ (cameras of several resolutions in one
        batch: one predict, one vti_measure_frames, one read); cameras: one index into params_by_camera per frame (host integers).
        Returns one record per frame, in frame order, each with a 'camera' key; frames of the same camera are smoothed in frame
        order.  annotate, encode, jpeg_quality, mixed: as StitchMeasurer.process_frames (frames of differing sizes only with
        mixed=True) -> (annotated, records).  burn_text, extra_text, rasterise (keyword only): as StitchMeasurer.process_frames, with
        mixed=True too (vti_stamp_frames: every picture gets its text at its own size).
        conf, iou, max_det: each a scalar, or a sequence with one entry per camera (stations with their own thresholds, config.py:
        69-73): the one predict then runs under an NMS table of one row per camera with `cameras` as the row index
        (vti_set_nms_table), every frame comes out as its camera's scalars alone would give it, and the output set is allocated for
        the largest max_det.  A sequence of another length is a ValueError before anything is predicted.
        windows (keyword only): None, "roi", or a list with one entry per CAMERA -- (x0, y0, x1, y1), "roi" or None (the whole frame):
        as StitchMeasurer.process_frames' window, every frame taking its camera's; window_margin (keyword only, default 32).
        annotate_native (keyword only): as StitchMeasurer.process_frames."""

    _window_keyword = "windows"

    def _process_frames(self, frames, cameras, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality, mixed,
                        burn_text=False, extra_text=None, rasterise=None, window=None, window_margin=32, annotate_native=False):
        cams = np.asarray(cameras.cpu() if isinstance(cameras, torch.Tensor) else cameras)      # Engine.measure range-checks them
        conf, iou, max_det, nms_rows = self._per_camera_nms(len(self.params), conf, iou, max_det)
        if window is not None and not isinstance(window, str):                      # one window per CAMERA -> one per frame
            if not isinstance(window, (list, tuple)) or len(window) != len(self.params):
                raise ValueError(f"process_frames: windows must be None, \"roi\" or a list with one entry per camera ({len(self.params)})")
            if cams.ndim != 1 or cams.dtype.kind not in "iu" or (cams.size and (cams.min() < 0 or cams.max() >= len(self.params))):
                raise ValueError(f"process_frames: cameras must be integers in [0, {len(self.params)})")
            window = [window[int(c)] for c in cams]
        got = self._frame_records(frames, self._table, cams, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality,
                                  mixed, burn_text=burn_text, extra_text=extra_text, rasterise=rasterise, nms_rows=nms_rows, window=window,
                                  window_margin=window_margin, window_params=lambda b: self.params[int(cams[b])],
                                  annotate_native=annotate_native)
        f64, i32 = got[:2]
        records = self._records(f64, i32, cams.tolist())
        if annotate is None:
            return records
        return self._with_text(got[2], records, i32, lambda b: self.params[int(cams[b])].min_stitches, got[3], extra_text,
                               rasterise), records

    def _records(self, f64, i32, cams):
        """Frame b's record from camera cams[b]'s stream, in frame order."""
        return [dict(self.streams[c].record(f64[b], i32[b]), camera=int(c)) for b, c in enumerate(cams)]


class StitchDistanceChecker(_DeviceStage):
    """Utils/check_stitch_distance.py's StitchMeasurementApp.process_frame without the camera and the window: model = a vti_amd YOLO,
    params = CheckerParams.  One predict, one vti_measure_checker and one device -> host read per batch; the two smoothing deques
    (:215-216, :519-530) live here, so consecutive calls continue one stream of frames.  Frames of one size, one camera (a rig of
    several cameras or resolutions: MultiCameraChecker); the checker's picture (:293-545) is drawn on request, for a selection of the batch (`annotate=`): vti_annotate_checker paints it
    on the device batch predict consumed, annotate.checker_display_list states what it holds, checker_text_items gives its text."""

    _mixed_sizes = False

    def __init__(self, model, params, frame_buffer=8):
        super().__init__(model)
        self.params = dataclasses.replace(params, frame_buffer=int(frame_buffer), drop_empty=bool(model.drop_empty_masks))
        self.frame_buf_dist, self.frame_buf_width = deque(maxlen=int(frame_buffer)), deque(maxlen=int(frame_buffer))
        self._cp = self.params.to_c()

    def _measure(self, eng, o, params, H0, W0, **kw):
        return eng.measure_checker(o, params, H0, W0, **kw)

    def _draw(self, eng, frames, o, res, params, sel, cameras, native, table):
        return eng.annotate_checker(frames, o, res, params, sel, native=native)

    def _record(self, f64, i32):
        return _checker_record(self.frame_buf_dist, self.frame_buf_width, self.params.min_stitches, f64, i32)

    def process_frames(self, frames, conf=0.20, iou=0.45, max_det=200, imgsz=640, retina_masks=False, rows=False, annotate=None,
                       encode=None, jpeg_quality=95, burn_text=False, extra_text=None, rasterise=None):
        """frames: as StitchMeasurer.process_frames takes them (a BGR uint8 batch, a list of JPEG files, RawFrames), all of one size.
        The defaults are the checker's predict call (:286: conf 0.20, iou 0.45, max_det 200, imgsz not passed: 640).  Returns one
        record per frame, in frame order, smoothed frame by frame: edge_distance_mm, stitch_width_mm (None: no value yet),
        stitch_count (the `n` of the info text: the number of widths), info_text (the string process_frame returns), timestamp, and
        `error` on the two failures.  rows=True -> (records, rows): rows[b] is what checker_text_items takes for frame b (one more
        device -> host read, of the per-slot rows).
        annotate: "all" or a sequence of frame indices -> (annotated, records): annotated = [(frame index, BGR ndarray H0 x W0 x 3 with
        the checker's picture, text_items)] for the selection, as StitchMeasurer.process_frames returns them (drawn on the device by
        vti_annotate_checker, one copy to the host; the text is checker_text_items', for annotate.put_text), records exactly as
        without it.  encode="jpeg" (with annotate): the picture is the bytes of the JPEG file cv2.imwrite saves of it at
        jpeg_quality, encoded on the device; any other encode, or encode without annotate, is a ValueError before anything is
        predicted.  With rows=True as well: (annotated, records, rows).
        burn_text, extra_text, rasterise: as StitchMeasurer.process_frames -- the items of checker_text_items, then extra_text's,
        burned into the selected pictures on the device (vti_stamp) before they are copied or encoded."""
        got = self._frame_records(frames, self._cp, None, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality,
                                  rows=bool(rows), burn_text=burn_text, extra_text=extra_text, rasterise=rasterise)
        f64, i32 = got[:2]
        records = [self._record(f64[b], i32[b]) for b in range(len(f64))]
        full = lambda r, b: dict(r, status=i32[b, 0], n_stitch=i32[b, 1], n_fabric=i32[b, 2], n_dist=i32[b, 4], n_width=i32[b, 5])
        if annotate is None:
            return (records, [full(got[2][b], b) for b in range(len(f64))]) if rows else records
        annotated = _burned(got[2], [checker_text_items(records[b], full(r, b), got[3]) + _extra_items(extra_text, b, records[b])
                                     for b, _, r in got[2]], rasterise)
        return (annotated, records, [full(got[4][b], b) for b in range(len(f64))]) if rows else (annotated, records)

    def process_frame(self, frame, annotate=False, **kw):
        """One frame: its record; annotate=True: the checker's tuple in this package's form, (annotated BGR ndarray, record), the text
        drawn too where OpenCV is installed (annotate.put_text; without it the picture carries everything but the text)."""
        if not annotate:
            return self.process_frames(np.asarray(frame)[None], **kw)[0]
        annotated, records = self.process_frames(np.asarray(frame)[None], annotate=[0], **kw)[:2]
        _, pic, items = annotated[0]
        try:
            _annotate.put_text(pic, items)
        except ImportError:
            pass
        return pic, records[0]


def _checker_record(buf_dist, buf_width, min_stitches, f64, i32):
    """One frame's record of the checker from its two smoothing deques: :345-347, :404-406 (the two early returns: nothing appended)
    and :515-540 (averages -> deques -> medians -> text)."""
    status = int(i32[0])
    if status != VTI_MEASURE_OK:
        text = ERRORS[status]
        return {'edge_distance_mm': None, 'stitch_width_mm': None, 'stitch_count': 0, 'info_text': text,
                'timestamp': datetime.now(), 'error': text}
    n_found = int(i32[5])
    smooth_dist = smooth_width = None
    if not np.isnan(f64[0]):
        buf_dist.append(float(f64[0]))
        smooth_dist = float(np.median(buf_dist))
    if not np.isnan(f64[1]):
        buf_width.append(float(f64[1]))
        smooth_width = float(np.median(buf_width))
    return {'edge_distance_mm': smooth_dist, 'stitch_width_mm': smooth_width, 'stitch_count': n_found,
            'info_text': checker_info_text(smooth_dist, smooth_width, n_found, min_stitches),
            'timestamp': datetime.now()}


class MultiCameraChecker(_DeviceStage):
    """StitchDistanceChecker for a rig: params_by_camera[c] = camera c's CheckerParams (calibration, class ids, thresholds), the
    frames of one call may come from any of the cameras and, as a list, differ in size.  One predict, one vti_measure_checker_cameras
    (a list of differing sizes: vti_measure_checker_frames, with retina_masks vti_measure_checker_frames_native) and one device ->
    host read per batch; every camera keeps its own pair of smoothing deques, so records, rows, annotated tuples and text items are
    those of one StitchDistanceChecker per camera, each fed only its camera's frames in the same order."""

    _mixed_sizes = True

    def __init__(self, model, params_by_camera, frame_buffer=8):
        super().__init__(model)
        self.params = [dataclasses.replace(p, frame_buffer=int(frame_buffer), drop_empty=bool(model.drop_empty_masks))
                       for p in params_by_camera]
        if not self.params:
            raise ValueError("MultiCameraChecker: at least one camera")
        self.buffers = [(deque(maxlen=int(frame_buffer)), deque(maxlen=int(frame_buffer))) for _ in self.params]      # (dist, width)
        self._tables = {}

    def _table(self, eng, device):
        key = (id(eng), str(device))
        if key not in self._tables:       # packed, validated and uploaded once per engine and device
            self._tables[key] = (eng, eng.pack_checker_cameras(self.params, device))
        return self._tables[key][1]

    def _measure(self, eng, o, params, H0, W0, **kw):
        return eng.measure_checker(o, params, H0, W0, **kw)

    def _draw(self, eng, frames, o, res, params, sel, cameras, native, table):
        return eng.annotate_checker(frames, o, res, params, sel, native=native, cameras=cameras, table=table)

    def _records(self, f64, i32, cams):
        """Frame b's record from camera cams[b]'s deques, in frame order."""
        return [dict(_checker_record(*self.buffers[c], self.params[c].min_stitches, f64[b], i32[b]), camera=int(c))
                for b, c in enumerate(cams)]

    def _cameras(self, frames, cameras):
        """cameras -> host int array, one index into params_by_camera per frame; refused before anything is predicted."""
        cams = np.asarray(cameras.cpu() if isinstance(cameras, torch.Tensor) else cameras)
        if cams.ndim != 1 or cams.dtype.kind not in "iu":
            raise ValueError("process_frames: cameras must be integers, one per frame")
        n = len(frames) if isinstance(frames, (list, tuple)) else (frames.shape[0] if getattr(frames, "ndim", 0) == 4 else None)
        if n is not None and n != cams.size:
            raise ValueError(f"process_frames: {n} frames but {cams.size} cameras")
        if cams.size and (cams.min() < 0 or cams.max() >= len(self.params)):
            raise ValueError(f"process_frames: camera index outside [0, {len(self.params)})")
        return cams

    @_annotate_native_keyword
    def process_frames(self, frames, cameras, conf=0.20, iou=0.45, max_det=200, imgsz=640, retina_masks=False, rows=False,
                       annotate=None, encode=None, jpeg_quality=95, *, mixed=False, burn_text=False, extra_text=None, rasterise=None):
        """frames as StitchDistanceChecker.process_frames takes them (a BGR uint8 batch, a list of ndarrays or JPEG files, RawFrames),
        or a list whose frames differ in size; cameras: one index into params_by_camera per frame (host integers; a wrong length or
        an index outside is a ValueError before anything is predicted).  Returns what StitchDistanceChecker.process_frames returns --
        records, with rows=True (records, rows), with annotate (annotated, records[, rows]) -- every record with a 'camera' key and
        smoothed within its camera in frame order.  mixed (keyword only): True lets a list of differing sizes be combined with
        annotate and encode (vti_annotate_checker_frames, vti_encode_jpeg_frames, vti_stamp_frames: every picture at its own size,
        the text placed by its own height), and lets retina_masks=True measure such a list (no annotate then); without it those
        combinations are refused, as MultiCameraMeasurer refuses them.  burn_text, extra_text, rasterise: as there.
        conf, iou, max_det: each a scalar or one entry per camera, as MultiCameraMeasurer.process_frames takes them.
        annotate_native (keyword only, default False; with mixed=True): True lets retina_masks=True on a list of differing sizes go
        with annotate -- the pictures are drawn from the frame-resolution masks (vti_measure_checker_frames_native ->
        vti_annotate_checker_frames_native); without it that combination stays refused, on frames of one size it changes nothing."""

    def _process_frames(self, frames, cameras, conf, iou, max_det, imgsz, retina_masks, rows, annotate, encode, jpeg_quality, mixed,
                        burn_text, extra_text, rasterise, annotate_native=False):
        cams = self._cameras(frames, cameras)
        conf, iou, max_det, nms_rows = self._per_camera_nms(len(self.params), conf, iou, max_det)
        got = self._frame_records(frames, self._table, cams, conf, iou, max_det, imgsz, retina_masks, annotate, encode, jpeg_quality,
                                  bool(mixed), rows=bool(rows), burn_text=burn_text, extra_text=extra_text, rasterise=rasterise,
                                  nms_rows=nms_rows, annotate_native=annotate_native)
        f64, i32 = got[:2]
        records = self._records(f64, i32, cams.tolist())
        full = lambda r, b: dict(r, status=i32[b, 0], n_stitch=i32[b, 1], n_fabric=i32[b, 2], n_dist=i32[b, 4], n_width=i32[b, 5])
        if annotate is None:
            return (records, [full(got[2][b], b) for b in range(len(f64))]) if rows else records
        h0 = lambda b: got[3][b] if isinstance(got[3], (list, tuple)) else got[3]
        annotated = _burned(got[2], [checker_text_items(records[b], full(r, b), h0(b)) + _extra_items(extra_text, b, records[b])
                                     for b, _, r in got[2]], rasterise)
        return (annotated, records, [full(got[4][b], b) for b in range(len(f64))]) if rows else (annotated, records)


def checker_info_text(smooth_dist, smooth_width, n_found, min_stitches):
    """check_stitch_distance.py:533-540."""
    if smooth_dist is not None and smooth_width is not None:
        return f"Edge Dist: {smooth_dist:.2f}mm | Avg Width: {smooth_width:.2f}mm (n={n_found})"
    if smooth_dist is not None:
        return f"Edge Distance: {smooth_dist:.2f}mm (n={n_found})"
    if smooth_width is not None:
        return f"Avg Width: {smooth_width:.2f}mm (n={n_found})"
    return f"Insufficient stitches (found {n_found}, need {int(min_stitches)})"


def checker_text_items(record, rows, h):
    """What the checker passes to cv2.putText for one frame, in annotate.text_items' form [(text, org, fontFace name, scale, colour,
    thickness)], for annotate.put_text.  record: the frame's StitchDistanceChecker record; rows: dict(status, n_stitch, n_fabric
    (frame_i32[b,0], [1], [2]), flags [n], rank [n], f64 [n,7]) of the frame's slots; h: the frame's height.  Host only."""
    font = _annotate.FONT
    status = int(rows["status"])
    if status != VTI_MEASURE_OK:          # :346, :405: the error text, and nothing else is written
        return [(ERRORS[status], (10, 55), font, 0.7, (0, 0, 255), 2)] if status in ERRORS else []
    f64 = np.asarray(rows["f64"], dtype=np.float64).reshape(-1, 7)
    flags = [int(f) for f in rows["flags"]]
    order = [i for _, i in sorted((int(r), i) for i, r in enumerate(rows["rank"]) if flags[i] & VTI_STITCH_KEPT and int(r) >= 0)]
    sel_near = VTI_STITCH_SELECTED | VTI_STITCH_NEAR
    any_near = any(flags[i] & sel_near == sel_near for i in order)
    items, last = [], None
    for i in order:                       # :465-512: the final set in order; the label shows per_widths[-1], the last width so far
        if not (flags[i] & VTI_STITCH_SELECTED and (not any_near or flags[i] & VTI_STITCH_NEAR)):
            continue
        if flags[i] & VTI_STITCH_WIDTH:
            last = float(f64[i, 4])
        if last is not None:
            items.append((f"w:{last:.1f}mm", (int(round(float(f64[i, 0]))) + 6, int(round(float(f64[i, 1]))) + 6), font, 0.45,
                          (0, 255, 0), 1))
    items.append((record["info_text"], (10, 30), font, 0.7, (0, 0, 255), 2))
    items.append((f"Stitches: {int(rows['n_stitch'])} | Fabric: {int(rows['n_fabric'])}", (10, h - 10), font, 0.5, (255, 255, 255), 1))
    return items
