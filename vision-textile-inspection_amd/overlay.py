"""The model-check viewer's picture (Utils/check_model.py:155-256, annotate_result) -- the host SPECIFICATION of vti_overlay.

The product draws it on the device (libvti.so `vti_overlay`, csrc/overlay.hip, Engine.overlay), byte for byte what `render(...)`
returns; the functions below stay as the statement of the semantics and as the reference of tests/test_gpu_overlay.py (pure numpy
and Python: about a second per full-size frame, so the package never calls them on the hot path).

What the reference draws, for one h x w BGR frame with n instances in detection order (no ROI filter, no class filter):
  overlay   = the frame with every instance's mask painted in its class colour, in order (`overlay[mask > 0] = color`): `tint`;
  annotated = the frame with, per instance in order, the mask's outer contours (thickness 2), its int-truncated box (thickness 2), a
              filled label plate and the label's text: `display_list` + annotate.rasterise (+ `put_labels` on the host);
  result    = cv2.addWeighted(overlay, 0.30, annotated, 0.70, 0): `add_weighted`.

The instance bitmap is get_instance_mask (:168-194): the mask as predict returns it stretched to (h, w) by cv2.INTER_NEAREST
(annotate.frame_bitmap, pad rows of a letterbox mask included, exactly as the reference stretches them); a frame-size mask is taken
as it is; an empty bitmap is None (no tint, no contour; the box and the plate are still drawn).  The reference then falls back to
cv2.fillPoly of `masks.xy[idx]`: that can never fire for this package, because the polygon of an empty mask has no vertices
(polygons.masks2segments gives [0, 2]) and fillPoly needs three.  An instance without a mask slot (past the capacity) is None too.

Deviations and unpinned parity, as annotate.py's:
  * cv2 is not available here, so PARITY IS UNPINNED against OpenCV itself (drawing rules: annotate.py; contours: polygons.py; the
    blend: below).  tests/test_overlay_cv2.py compares with cv2 where it exists.
  * RETR_EXTERNAL: the contours are those of polygons.find_external_contours -- one per 8-connected component, including a component
    that lies inside a hole of another one, which OpenCV's RETR_EXTERNAL leaves out.  vti_annotate's outline has the same deviation.
  * addWeighted: OpenCV 4's dispatched kernel computes v_fma(a, alpha, b * beta) in float32 (gamma = 0): the product b * beta is rounded
    to float32, the fused multiply-add is rounded once, and the sum is rounded half to even and saturated.  `add_weighted` states that
    form.  A cv2 built without FMA rounds a * alpha as well (`add_weighted_unfused`); the two differ by at most 1 on a few of the
    65 536 (a, b) pairs.
  * Text stays on the host (Hershey glyphs): `label_items`, `plates` and `put_labels` need cv2 for the metrics and the drawing.
"""
import numpy as np

from . import annotate, polygons

__all__ = ["PALETTE", "DRAW", "BLEND", "BOTH", "MODES", "OUTLINE_SKIPPED", "ALPHA", "BETA", "FONT", "FONT_SCALE", "FONT_THICKNESS",
           "colour", "instance_bitmap", "tint", "contours", "display_list", "fill_rect", "rasterise", "add_weighted",
           "add_weighted_unfused", "render", "label_name", "label_items", "plates", "put_labels", "annotate_result", "annotate_results"]

# BGR: build_color's palette (check_model.py:157-164), in its order
PALETTE = ((0, 255, 0), (0, 165, 255), (255, 0, 255), (255, 255, 0), (0, 255, 255), (255, 128, 0))
DRAW, BLEND, BOTH = 1, 2, 3
MODES = {"draw": DRAW, "blend": BLEND, "both": BOTH}
OUTLINE_SKIPPED = 1         # status bit: the frame's contours needed more than max_points vertices (or the tracer hit its bound)
ALPHA, BETA = 0.30, 0.70
FONT, FONT_SCALE, FONT_THICKNESS = "FONT_HERSHEY_SIMPLEX", 0.55, 2


def colour(cls, palette=PALETTE):
    """build_color: palette[cls % len(palette)]."""
    return tuple(int(v) for v in palette[int(cls) % len(palette)])


# ---- the instance bitmaps and the tint ----------------------------------------------------------------------------------------
def instance_bitmap(mask, h, w):
    """get_instance_mask (:168-194): u8 0/1 [h, w], or None for an empty mask or an instance without a mask slot."""
    if mask is None:
        return None
    bm = annotate.frame_bitmap(mask, h, w)
    return bm if np.count_nonzero(bm) else None


def tint(frame, cls, bitmaps, palette=PALETTE):
    """`overlay[mask > 0] = color` in detection order: a pixel takes the colour of the highest-index instance whose bitmap covers it,
    otherwise it stays the frame's."""
    out = np.array(frame, dtype=np.uint8, copy=True)
    for c, bm in zip(cls, bitmaps):
        if bm is not None:
            out[bm > 0] = colour(c, palette)
    return out


def contours(bitmap):
    """polygons.find_external_contours of a frame-size bitmap (identity scale, CHAIN_APPROX_SIMPLE), traced on the bounding box of
    its set pixels (the same contours in the same order: the crop shifts every pixel alike)."""
    ys, xs = np.flatnonzero(bitmap.any(axis=1)), np.flatnonzero(bitmap.any(axis=0))
    if not len(ys):
        return []
    y0, x0 = int(ys[0]), int(xs[0])
    sub = bitmap[y0:int(ys[-1]) + 1, x0:int(xs[-1]) + 1]
    return [c + np.array([x0, y0], np.int32) for c in polygons.find_external_contours(sub)]


# ---- what is drawn ------------------------------------------------------------------------------------------------------------
def display_list(h, w, cls, xyxy, bitmaps, plates=None, palette=PALETTE, max_points=None, with_status=False):
    """The ordered primitives of check_model.py:215-243 for one h x w frame; a later primitive overwrites an earlier one.
    cls [n], xyxy f32 [n,4] (frame px), bitmaps: per instance instance_bitmap()'s answer; plates: None, or per instance None or
    (xa, ya, xb, yb).  Per instance: the closed polylines of its contours (thickness 2), ("rect", ..., 2) of its int-truncated box,
    and ("fillrect", (xa, ya), (xb, yb), colour) when it has a plate.  max_points: vti_overlay's bound on the contour vertices of the
    whole frame; when they need more, NONE of the frame's contours is drawn and the status word is OUTLINE_SKIPPED (vti_annotate's
    rule); everything else stands.  -> [primitive] (with_status: and the status word)."""
    n = len(cls)
    ib = np.trunc(np.asarray(xyxy, dtype=np.float64).reshape(-1, 4)).astype(np.int64)
    conts = [contours(bm) if bm is not None else [] for bm in bitmaps]
    word = 0
    if max_points is not None and sum(len(c) for cs in conts for c in cs) > max_points:
        word, conts = OUTLINE_SKIPPED, [[] for _ in range(n)]
    prims = []
    for i in range(n):
        col = colour(cls[i], palette)
        for c in conts[i]:
            prims.append(("polyline", np.asarray(c, dtype=np.int32).reshape(-1, 2), True, col, 2))
        box = tuple(int(v) for v in ib[i])
        prims.append(("rect", box[:2], box[2:], col, 2))
        if plates is not None and plates[i] is not None:
            xa, ya, xb, yb = (int(v) for v in plates[i])
            prims.append(("fillrect", (xa, ya), (xb, yb), col))
    return (prims, word) if with_status else prims


def fill_rect(img, pa, pb, col):
    """cv2.rectangle(img, pa, pb, col, -1) for xa <= xb and ya <= yb: every in-frame pixel with xa <= x <= xb and ya <= y <= yb
    (FillConvexPoly on the four corners covers exactly those: tests/test_overlay.py).  A rectangle with xb < xa or yb < ya draws
    nothing (the reference's plates never are: text_w + 8 > 0)."""
    h, w = img.shape[:2]
    (xa, ya), (xb, yb) = pa, pb
    x0, x1, y0, y1 = max(xa, 0), min(xb, w - 1), max(ya, 0), min(yb, h - 1)
    if xb < xa or yb < ya or x0 > x1 or y0 > y1:
        return
    img[y0:y1 + 1, x0:x1 + 1] = col


def rasterise(frame, primitives):
    """annotate.rasterise, and ("fillrect", ...): -> a copy of the frame with the primitives painted in list order."""
    img = np.array(frame, dtype=np.uint8, copy=True)
    run = []
    for p in list(primitives) + [None]:
        if p is not None and p[0] != "fillrect":
            run.append(p)
            continue
        if run:
            img = annotate.rasterise(img, run)
            run = []
        if p is not None:
            fill_rect(img, tuple(map(int, p[1])), tuple(map(int, p[2])), p[3])
    return img


# ---- the blend ----------------------------------------------------------------------------------------------------------------
def add_weighted(a, b, alpha=ALPHA, beta=BETA):
    """cv2.addWeighted(a, alpha, b, beta, 0) on uint8, OpenCV 4's v_fma form: t = fma(f32(a), f32(alpha), f32(b) * f32(beta)), the
    product rounded to float32, the fma rounded ONCE to float32; the result is t rounded half to even, saturated to 0..255.
    The fma is computed exactly in float64 (an 8-bit by 24-bit product plus a 24-bit term: exact while the exponents of alpha and
    beta are within 2^20 of each other) and rounded once."""
    a32, b32 = np.asarray(a, dtype=np.uint8).astype(np.float32), np.asarray(b, dtype=np.uint8).astype(np.float32)
    al, be = np.float32(alpha), np.float32(beta)
    p = (b32 * be).astype(np.float32)
    t = (a32.astype(np.float64) * np.float64(al) + p.astype(np.float64)).astype(np.float32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


def add_weighted_unfused(a, b, alpha=ALPHA, beta=BETA):
    """The form a cv2 built without FMA computes: f32(a * alpha) + f32(b * beta), every step rounded to float32.  Tests and
    documentation only."""
    a32, b32 = np.asarray(a, dtype=np.uint8).astype(np.float32), np.asarray(b, dtype=np.uint8).astype(np.float32)
    t = ((a32 * np.float32(alpha)).astype(np.float32) + (b32 * np.float32(beta)).astype(np.float32)).astype(np.float32)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


# ---- the picture --------------------------------------------------------------------------------------------------------------
def render(frame, cls, xyxy, masks, plates=None, mode=BOTH, annotated=None, alpha=ALPHA, beta=BETA, palette=PALETTE,
           max_points=None, with_status=False):
    """annotate_result (:197-256) without its text, for one BGR frame [h,w,3].  cls [n], xyxy f32 [n,4] in detection order; masks: the n
    masks as predict returns them (letterbox or frame size; None: no mask slot); plates: see display_list.
    DRAW  -> the frame with the display list rasterised (the reference's `annotated` before the blend);
    BLEND -> add_weighted(tint(frame), annotated): `annotated` is the caller's picture (None: the frame itself);
    BOTH  -> BLEND applied to DRAW's output.
    With n = 0 the reference returns the bare copy: nothing is drawn or tinted, and BLEND of a frame with itself is the identity.
    -> u8 [h,w,3] (with_status: and the status word)."""
    if mode not in (DRAW, BLEND, BOTH):
        raise ValueError(f"render: mode must be DRAW, BLEND or BOTH, got {mode!r}")
    frame = np.asarray(frame, dtype=np.uint8)
    h, w = frame.shape[:2]
    bitmaps = [instance_bitmap(m, h, w) for m in masks]
    word = 0
    pic = frame if annotated is None else np.asarray(annotated, dtype=np.uint8)
    if mode & DRAW:
        prims, word = display_list(h, w, cls, xyxy, bitmaps, plates, palette, max_points, with_status=True)
        pic = rasterise(frame, prims)
    if mode & BLEND:
        pic = add_weighted(tint(frame, cls, bitmaps, palette), pic, alpha, beta)
    pic = np.array(pic, dtype=np.uint8, copy=True)
    return (pic, word) if with_status else pic


# ---- text (host) --------------------------------------------------------------------------------------------------------------
def label_name(cls, names):
    """check_model.py:227-232."""
    c = int(cls)
    if isinstance(names, dict):
        return names.get(c, str(c))
    if isinstance(names, list) and 0 <= c < len(names):
        return names[c]
    return str(c)


def label_items(cls, conf, xyxy, names):
    """Per instance what the reference passes to cv2.putText (:234-253): [(text, org, fontFace name, scale, colour, thickness,
    lineType name)], text = f"{name} {score:.2f}", org = (x1 + 4, text_y - 2) with text_y = max(20, y1 - 8)."""
    ib = np.trunc(np.asarray(xyxy, dtype=np.float64).reshape(-1, 4)).astype(np.int64)
    items = []
    for i in range(len(cls)):
        x1, y1 = int(ib[i, 0]), int(ib[i, 1])
        text_y = max(20, y1 - 8)
        items.append((f"{label_name(cls[i], names)} {float(conf[i]):.2f}", (x1 + 4, text_y - 2), FONT, FONT_SCALE, (0, 0, 0),
                      FONT_THICKNESS, "LINE_AA"))
    return items


def plates(items):
    """The filled rectangle behind every label (:235-243): int [n,4] (xa, ya, xb, yb).  Needs cv2.getTextSize: raises ImportError
    where OpenCV is not installed."""
    import cv2
    out = np.zeros((len(items), 4), np.int32)
    for i, (text, org, face, scale, _, thickness, _) in enumerate(items):
        (tw, th), base = cv2.getTextSize(text, getattr(cv2, face), scale, thickness)
        x1, text_y = org[0] - 4, org[1] + 2
        out[i] = (x1, text_y - th - base - 4, x1 + tw + 8, text_y + 4)
    return out


def put_labels(img, items):
    """cv2.putText for every item of label_items(), in place.  Raises ImportError where OpenCV is not installed."""
    import cv2
    for text, org, face, scale, col, thickness, line in items:
        cv2.putText(img, text, org, getattr(cv2, face), scale, col, thickness, getattr(cv2, line))
    return img


def _have_cv2():
    try:
        import cv2  # noqa: F401
        return True
    except ImportError:
        return False


# ---- the drop-in ----------------------------------------------------------------------------------------------------------------
def annotate_result(frame, result, names=None, labels=None):
    """check_model.py's annotate_result(frame, result, names) on the device: the viewer changes one import.  `result` is one Results
    of YOLO.predict; it needs the Engine that made it (result._engine: RuntimeError otherwise, as Masks.xy; there is no CPU
    fallback).  labels=None: where cv2 is importable.  With labels the plates come from plates(), DRAW runs on the device, ONE copy
    goes to the host, put_labels draws the text there, one copy goes back and BLEND runs on the device: up to the FMA note above, the
    reference's picture including its blended text.  Without labels: BOTH in one call and one copy to the host (the picture
    render(...) gives).  -> u8 [h,w,3] ndarray."""
    import torch
    eng = getattr(result, "_engine", None)
    if eng is None:
        raise RuntimeError("overlay.annotate_result needs the Engine that made the result (YOLO.predict's Results); there is no host path")
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    n = len(result.boxes) if getattr(result, "boxes", None) is not None else 0
    if n == 0:
        return frame.copy()
    if labels is None:
        labels = _have_cv2()
    h, w = frame.shape[:2]
    data = result.boxes.data
    dev = data.device
    bits = result.masks.bits if result.masks is not None else torch.zeros((0, 1, 8), dtype=torch.uint8, device=dev)
    native = result.masks is not None and tuple(bits.shape[1:]) == (h, 8 * -(-w // 64)) and result.masks._W == w
    out = dict(dets=result.dets.reshape(1, n, -1).contiguous(), xyxy=data[:, :4].reshape(1, n, 4).contiguous(),
               counts=torch.tensor([n], dtype=torch.int32, device=dev), offsets=torch.tensor([0, n], dtype=torch.int32, device=dev),
               masks=bits.contiguous())
    dframe = torch.from_numpy(frame).to(dev).unsqueeze(0)
    if not labels:
        return eng.overlay(dframe, out, [0], native=native, mode="both")["frames"][0].cpu().numpy()
    host = data.cpu().numpy()
    items = label_items(host[:, 5], host[:, 4], host[:, :4], names)
    pl = torch.from_numpy(plates(items)).to(dev)
    if pl.shape[0] < bits.shape[0]:
        pl = torch.cat((pl, torch.zeros((bits.shape[0] - pl.shape[0], 4), dtype=torch.int32, device=dev)))
    drawn = eng.overlay(dframe, out, [0], native=native, plates=pl[:bits.shape[0]].contiguous(), mode="draw")["frames"]
    pic = put_labels(drawn[0].cpu().numpy(), items)
    back = torch.from_numpy(pic).to(dev).unsqueeze(0)
    return eng.overlay(dframe, out, [0], native=native, mode="blend", annotated=back)["frames"][0].cpu().numpy()


def annotate_results(frames, results, names=None, labels=None):
    """The batch form of annotate_result: `frames` is the list (or [B,h,w,3] array) one YOLO.predict call took and `results` its list
    of Results; the frames may differ in size and the masks may be letterbox ones or those of retina_masks=True (mixed=True for
    sizes that differ).  Every frame with detections is drawn at its own size by ONE Engine.overlay(..., table=) call on the flat
    frame buffer (vti_overlay_frames).  Without labels: BOTH and one copy to the host.  With labels (None: where cv2 is
    importable): DRAW, one copy out, put_labels per picture, one copy back, BLEND.  -> [u8 [h,w,3] ndarray], each byte for byte
    annotate_result(frames[b], results[b], names, labels); a frame without detections is its bare copy.  All results must come
    from one Engine (RuntimeError without one; there is no CPU fallback)."""
    import torch
    frames = [np.ascontiguousarray(f, dtype=np.uint8) for f in frames]
    results = list(results)
    if len(frames) != len(results):
        raise ValueError(f"annotate_results: {len(frames)} frames but {len(results)} results")
    for f in frames:
        if f.ndim != 3 or f.shape[2] != 3:
            raise ValueError(f"annotate_results: every frame must be uint8 HxWx3, got shape {f.shape}")
    counts = [len(r.boxes) if getattr(r, "boxes", None) is not None else 0 for r in results]
    sel = [b for b, n in enumerate(counts) if n]
    pics = [f.copy() for f in frames]
    if not sel:
        return pics
    eng = getattr(results[sel[0]], "_engine", None)
    if eng is None or any(getattr(results[b], "_engine", None) is not eng for b in sel):
        raise RuntimeError("overlay.annotate_results needs the one Engine that made the results (one YOLO.predict call's Results); "
                           "there is no host path")
    if labels is None:
        labels = _have_cv2()
    B, M = len(frames), max(counts)
    shapes = tuple(f.shape[:2] for f in frames)
    dev = results[sel[0]].boxes.data.device
    # frame-size rows or letterbox bits: a frame of the canvas's own size whose width is a multiple of 64 has the same layout in
    # both forms (and the same picture), so it does not vote; only a real mix is refused
    natives = set()
    for b in sel:
        m, (h, w) = results[b].masks, shapes[b]
        if m is None:
            continue
        rows, as_native, as_letterbox = tuple(m.bits.shape[1:]), (h, 8 * -(-w // 64)), (eng.H, eng.W // 8)
        if not (as_native == as_letterbox and m._W == w):
            natives.add(rows == as_native and m._W == w)
    if len(natives) > 1:
        raise ValueError("annotate_results: the results mix letterbox masks and frame-size masks")
    native = bool(natives and natives.pop())
    row = results[sel[0]].dets.shape[-1]
    dets = torch.zeros((B, M, row), dtype=torch.float32, device=dev)
    xyxy = torch.zeros((B, M, 4), dtype=torch.float32, device=dev)
    bits = []
    for b in sel:
        n = counts[b]
        dets[b, :n] = results[b].dets.reshape(n, row)
        xyxy[b, :n] = results[b].boxes.data[:, :4]
        if results[b].masks is not None:
            bits.append(results[b].masks.bits.contiguous())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = dict(dets=dets, xyxy=xyxy, counts=torch.tensor(counts, dtype=torch.int32, device=dev), offsets=torch.from_numpy(offsets).to(dev))
    if native:          # the ragged rows of masks_native_frames: frame b's n slots back to back from mask_bases[b] on
        nbytes = [results[b].masks.bits.numel() if counts[b] and results[b].masks is not None else 0 for b in range(B)]
        out["masks"] = torch.cat([m.reshape(-1) for m in bits]) if bits else torch.zeros(0, dtype=torch.uint8, device=dev)
        out["mask_bases"] = torch.from_numpy(np.concatenate([[0], np.cumsum(nbytes)]).astype(np.int64)).to(dev)
        slots = B * M
    else:
        out["masks"] = torch.cat(bits) if bits else torch.zeros((0, eng.H, eng.W // 8), dtype=torch.uint8, device=dev)
        slots = int(out["masks"].shape[0])
    table = eng.pack_frames(shapes, dev)[0]
    flat = np.zeros(table.total_bytes, np.uint8)
    for f, at in zip(frames, table.byte_offsets):
        flat[at:at + f.size] = f.reshape(-1)
    dflat = torch.from_numpy(flat).to(dev)

    def cut(host, got):
        for k, b in enumerate(sel):
            h, w = shapes[b]
            at = got["byte_offsets"][k]
            pics[b] = host[at:at + 3 * h * w].reshape(h, w, 3)
        return pics
    if not labels:
        got = eng.overlay(dflat, out, sel, native=native, mode="both", table=table)
        return cut(got["buf"].cpu().numpy(), got)
    items, rows = {}, np.zeros((max(slots, 1), 4), np.int32)
    for b in sel:
        host = results[b].boxes.data.cpu().numpy()
        items[b] = label_items(host[:, 5], host[:, 4], host[:, :4], names)
        pl = plates(items[b])
        live = max(0, min(counts[b], slots - int(offsets[b])))
        rows[offsets[b]:offsets[b] + live] = pl[:live]
    got = eng.overlay(dflat, out, sel, native=native, plates=torch.from_numpy(rows[:slots]).to(dev) if slots else None, mode="draw",
                      table=table)
    host = got["buf"].cpu().numpy()
    for k, b in enumerate(sel):                     # the text goes into `host` itself, whatever put_labels returns
        h, w = shapes[b]
        view = host[got["byte_offsets"][k]:][:3 * h * w].reshape(h, w, 3)
        view[...] = put_labels(view, items[b])
    back = torch.from_numpy(host).to(dev)
    got = eng.overlay(dflat, out, sel, native=native, mode="blend", annotated=back, table=table)
    return cut(got["buf"].cpu().numpy(), got)
