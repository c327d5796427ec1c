/*
 * vti.h -- C ABI of libvti.so: MI355X (gfx950) YOLOv8-seg inference hot path.
 *
 * Drop-in boundary for the reference's `ultralytics.YOLO` object protocol
 * (RishWijewardhena/vision-textile-inspection):
 *     model = YOLO(path)                                   measurement.py:145
 *     model.predict(img, conf=, iou=, max_det=, imgsz=)    measurement.py:208-210,
 *                                                          Utils/check_model.py:331-337
 *     Results.boxes.{xyxy,cls,conf}, Results.masks.data    measurement.py:74-75,242-245
 * and for measurement.py's mask post-processing (measurement.py:70-86,160-185,300-330).
 *
 * The reference has no FFI of its own; the binding a maintainer adds is the ctypes
 * shim shown in INTEGRATION.md (shipped as vti_amd/ in this repo).
 *
 * Conventions
 *  - Every function returns VTI_OK (0) or a negative vti_status; it never aborts or
 *    exits the process (measurement.py:207-216 catches every predict exception and
 *    keeps running).  vti_last_error(ctx) gives a message for the last failure.
 *  - All `dev_*` pointers are DEVICE pointers owned by the caller (torch-ROCm tensors'
 *    data_ptr()).  The library never allocates caller-visible memory; its only device
 *    allocation is the packed weight image made by vti_load_weights.
 *  - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream).
 *    Calls enqueue work on it and return; no hidden synchronisation.
 *  - One ctx per (device, host thread) (main.py:187-211: single-threaded use).  A ctx is bound to the device passed to
 *    vti_load_weights; entry points that launch work return VTI_ERR_STATE when another device is current.
 *  - Multi-GPU is one process per GPU above this ABI: frames are independent, so the only exchange steps
 *    are a scatter of uint8 frames and a gather of detections + consumer reductions, done by the host shim with
 *    torch.distributed (backend "nccl" = RCCL over xGMI; vti_amd/dataparallel.py).  The library itself opens no communicator
 *    and exports no vti_dp_* entry points: there is no collective inside the model.
 *  - Tensor layouts (T = fp16 for VTI_F16, fp32 for VTI_F32 and VTI_H2):
 *      frames   u8  [B,H0,W0,3]           camera frames, any channel order (see swap_rb)
 *      input    u8  [B,H,W,3]             letterboxed frames (H,W multiples of 32)
 *      pred     f32 [B,A,4+nc+nm]         decoded head output, ANCHOR-MAJOR: Ultralytics' [B,4+nc+nm,A] transposed, so that
 *                                         an anchor's box, class scores and mask coefficients are one contiguous row (the head
 *                                         towers write it and NMS reads it row-wise; the Python shim hands out the
 *                                         [B,4+nc+nm,A] view of the same memory)
 *                                          (cx,cy,w,h in letterboxed px; sigmoid class scores; coeffs)
 *      proto    T   [B,H/4,W/4,nm]        mask prototypes, NHWC
 *      dets     f32 [B,max_det,6+nm]      rows x1,y1,x2,y2,conf,cls,coeff[nm]; conf-descending;
 *                                          boxes in letterboxed px (vti_scale_boxes maps to frame px)
 *      counts   i32 [B]                   detections per frame
 *      masks    u8  [cap,H,W] (VTI_PACK_U8, 0/1 per byte) or u8 [cap,H,W/8] (VTI_PACK_BITS,
 *               LSB-first); instance i of frame b lives in slot offsets[b]+i.  vti_masks_native: u8 [cap,H0,W0] or
 *               u8 [cap,H0,8*ceil(W0/64)] (vti_mask_native_layout)
 *      offsets  i32 [B+1]                 exclusive prefix sum of counts (written by vti_masks)
 */
#ifndef VTI_H
#define VTI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vti_ctx vti_ctx;

typedef enum {
    VTI_OK = 0,
    VTI_ERR_ARG = -1,        /* bad argument / shape */
    VTI_ERR_STATE = -2,      /* weights or workspace not set */
    VTI_ERR_WEIGHTS = -3,    /* container does not match the model description */
    VTI_ERR_HIP = -4,        /* HIP runtime error (message in vti_last_error) */
    VTI_ERR_NOMEM = -5,      /* workspace too small */
    VTI_ERR_UNSUPPORTED = -6
} vti_status;

/* Storage type of weights and activations.  VTI_H2 = split-fp16: every element is the fp16 pair (hi, lo) of value * 16
 * (22-23 significant bits) and every product runs on the fp16 matrix pipe (two 16x16x32 MFMAs per 16 channels, fp32
 * accumulation): the results meet the reference tolerance (mask IoU >= 0.999, |d box| < 1e-3) like VTI_F32 at ~4x its matrix rate.
 * Range of a stored VTI_H2 activation: |v| <= 4094, SATURATING (every epilogue clamps before it encodes: 4094 * 16 = 65504 is the
 * largest fp16; a larger result is stored as +-4094, never as inf or NaN) -- 1/16 of plain fp16's range.  The lo half is a normal
 * fp16 number down to |v| ~ 8e-3; below that a value has an absolute floor of 2^-28.  Weights carry one power-of-two scale per
 * conv; channels far below their conv's largest have subnormal lo halves, which the fp16 MFMA keeps (measured: bit for bit).
 * NaN inputs are not specified.
 * proto is f32 for VTI_H2 and VTI_F32, fp16 for VTI_F16. */
enum { VTI_F16 = 0, VTI_F32 = 1, VTI_H2 = 2 };
enum { VTI_MASK_LOGIT = 0,     /* current Ultralytics: crop, bilinear upsample, > 0.0 */
       VTI_MASK_SIGMOID = 1 }; /* Ultralytics 8.0.x : sigmoid, crop, upsample, > 0.5  */
enum { VTI_PACK_U8 = 0, VTI_PACK_BITS = 1 };
/* vti_predict mask_mode flag: frame-resolution masks (Ultralytics predict(retina_masks=True)) through vti_masks_native. */
#define VTI_MASK_NATIVE 0x10
/* vti_masks work-list size: one call handles at most max_batch * VTI_MASK_SLOTS_PER_FRAME instances (capacity above that is
 * VTI_ERR_UNSUPPORTED); vti_workspace_bytes() is sized for it.  Ultralytics' default max_det is 300, the reference's 200. */
#define VTI_MASK_SLOTS_PER_FRAME 512
/* The full decode kernel keeps its anchors' rows of 64 + nc + nm logits (and one word of padding each) in 64 KiB of LDS: 64
 * anchors per workgroup up to nc + nm = 191, fewer above that, and one row must fit: at most this many class + coefficient
 * channels.  It runs in the plans whose class / coefficient towers do not write pred themselves (VTI_NO_PRED_SCATTER=1, or towers
 * that do not end in a fused 1x1 stage, as with 160 classes and more); vti_create refuses such a plan above the limit
 * (VTI_ERR_ARG, the message names both numbers). */
#define VTI_DECODE_MAX_CHANNELS 16319

/* Model description: replaces what YOLO(model_path) reads out of the .pt (measurement.py:145). */
typedef struct {
    char scale;        /* 'n','s','m','l','x' */
    int32_t nc;        /* classes (reference: 2 -- stitch=0, fabric=1, config.py:69-70); >= 1.  A plan that keeps the full decode
                          kernel needs nc + nm <= VTI_DECODE_MAX_CHANNELS: vti_create says so otherwise */
    int32_t nm;        /* mask coefficients, 32 */
    int32_t reg_max;   /* DFL bins, 16 */
    int32_t H, W;      /* letterboxed input size, multiples of 32 */
    int32_t max_batch; /* largest B any call will pass */
    int32_t dtype;     /* VTI_F16 / VTI_F32 / VTI_H2: storage type of weights and activations */
} vti_desc;

/* One row of the fused conv table (replaces walking model.model[*] of the unpickled net). */
typedef struct {
    char name[48];               /* Ultralytics tensor-name prefix, e.g. "model.2.m.0.cv1" */
    int32_t c1, c2, k, s, kind;  /* kind: 0 conv+BN+SiLU (folded), 1 conv+bias, 2 ConvTranspose2d+bias */
    int32_t h_in, w_in, h_out, w_out;
    int64_t macs;                /* multiply-accumulates per frame */
    int32_t tile_h, tile_w;      /* launch geometry: output pixels per workgroup tile */
    int32_t waves_n, nrep;       /* waves along Cout, 16-wide cout tiles per wave */
    int32_t lds_bytes;
    int32_t fused;               /* 1: this 1x1 conv runs inside the previous conv's kernel (register-level fusion) */
    int32_t persistent;          /* 1: persistent LDS-DMA kernel (conv_pk.hip): tile_h/4 * waves_n compute waves + as many loader waves */
} vti_conv_info;

/* ---- lifetime -------------------------------------------------------------------- */
/* Builds the network plan on the host.  Touches no GPU: usable on a CPU-only box. */
int32_t vti_create(const vti_desc* desc, vti_ctx** out);
void vti_destroy(vti_ctx* ctx);
const char* vti_last_error(const vti_ctx* ctx);   /* ctx may be NULL: last create error */

/* ---- plan introspection (host only) ------------------------------------------------ */
int32_t vti_num_convs(const vti_ctx* ctx);
int32_t vti_conv_at(const vti_ctx* ctx, int32_t i, vti_conv_info* out);
int32_t vti_num_anchors(const vti_ctx* ctx);
int64_t vti_fused_params(const vti_ctx* ctx);     /* incl. the frozen DFL arange, as model.info() */
int64_t vti_macs_per_frame(const vti_ctx* ctx);   /* conv + deconv MACs */
int64_t vti_workspace_bytes(const vti_ctx* ctx);  /* for max_batch frames */
int32_t vti_num_launches(const vti_ctx* ctx);     /* kernels per vti_forward call */

/* ---- device setup ---------------------------------------------------------------- */
/* Parses a VTIW1 container held in HOST memory (fused OIHW fp32 + bias per conv, table
 * order), repacks it into MFMA fragment order and uploads it to `device`. */
int32_t vti_load_weights(vti_ctx* ctx, const void* host_blob, size_t nbytes, int32_t device);
/* Caller-owned device scratch of at least vti_workspace_bytes(), 256-B aligned. */
int32_t vti_set_workspace(vti_ctx* ctx, void* dev_ws, size_t nbytes);

/* ---- the hot path: stages of predict() ------------------------------------------- */
/* U1 LetterBox: resize (OpenCV u8 INTER_LINEAR fixed point; the rounded 2x2 box mean OpenCV substitutes -- INTER_AREA --
 * when the frame is exactly twice the resized size) + pad 114 to HxW.  A frame already HxW is copied through. */
int32_t vti_letterbox(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0,
                      uint8_t* dev_input, void* stream);
/* U2-U5 network forward.  swap_rb=1 reproduces Ultralytics' channel flip of ndarray sources. */
int32_t vti_forward(vti_ctx* ctx, const uint8_t* dev_input, int32_t B, int32_t swap_rb,
                    float* dev_pred, void* dev_proto, void* stream);
/* U6 non_max_suppression (class-aware unless agnostic), torchvision.ops.nms semantics. */
int32_t vti_nms(vti_ctx* ctx, const float* dev_pred, int32_t B, float conf, double iou,
                int32_t max_det, int32_t agnostic, float* dev_dets, int32_t* dev_counts, void* stream);
/* U5 -> U6 hand-over without re-reading the class scores: vti_forward_scored also writes, for every anchor, the pair (best class
 * score, index of the first class that has it, as a float) into dev_anchor_best (f32 [B, A, 2]) -- from the class towers' epilogue,
 * where the scores are in registers -- and vti_nms_scored takes its candidates (score > conf) from those 8 bytes per anchor instead of
 * scanning nc scores per anchor of dev_pred (Ultralytics: x[:, 4:4+nc].amax(1) > conf_thres, the first thing non_max_suppression
 * does).  Same detections as vti_forward + vti_nms, bit for bit; the pairs must belong to the dev_pred they are passed with. */
int32_t vti_forward_scored(vti_ctx* ctx, const uint8_t* dev_input, int32_t B, int32_t swap_rb,
                           float* dev_pred, void* dev_proto, float* dev_anchor_best, void* stream);
int32_t vti_nms_scored(vti_ctx* ctx, const float* dev_pred, const float* dev_anchor_best, int32_t B, float conf, double iou,
                       int32_t max_det, int32_t agnostic, float* dev_dets, int32_t* dev_counts, void* stream);
/* U7 process_mask(upsample=True) + threshold.  Writes slots [0, min(offsets[B], capacity)) of dev_masks completely; slots
 * beyond that are left untouched (no whole-buffer memset: the cost follows the number of instances, not the capacity). */
int32_t vti_masks(vti_ctx* ctx, const float* dev_dets, const int32_t* dev_counts, const void* dev_proto,
                  int32_t B, int32_t max_det, int32_t mode, int32_t packing,
                  uint8_t* dev_masks, int32_t capacity, int32_t* dev_offsets, void* stream);
/* U7' process_mask_native + threshold (Ultralytics predict(retina_masks=True), the 8.1/8.2 scale_masks form): coefficients x
 * prototypes, crop of the prototype grid to the frame's letterbox content [top,bottom) x [left,right) (pads computed in double,
 * truncated), bilinear resize (align_corners=False, torch's fp32 taps; up or down) straight to H0xW0, crop to the FRAME-px boxes
 * dev_xyxy of vti_scale_boxes (x1 <= col < x2, y1 <= row < y2), threshold as vti_masks.  Masks are u8 [cap,H0,row_bytes]:
 * VTI_PACK_BITS row_bytes = 8*ceil(W0/64) (LSB-first, bits at columns >= W0 are 0; dev_masks 8-byte aligned), VTI_PACK_U8
 * row_bytes = W0.  Slots, offsets and the capacity rule as vti_masks; nm must be 32 (else VTI_ERR_UNSUPPORTED). */
int32_t vti_masks_native(vti_ctx* ctx, const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                         const void* dev_proto, int32_t B, int32_t max_det, int32_t H0, int32_t W0, int32_t mode,
                         int32_t packing, uint8_t* dev_masks, int32_t capacity, int32_t* dev_offsets, void* stream);
/* Host only: out[6] = {top, bottom, left, right, row_bytes, slot_bytes} of vti_masks_native for an H0xW0 frame. */
int32_t vti_mask_native_layout(const vti_ctx* ctx, int32_t H0, int32_t W0, int32_t packing, int32_t out[6]);
/* U8 scale_boxes + clip: letterboxed px -> frame px, writes f32 [B,max_det,4]. */
int32_t vti_scale_boxes(vti_ctx* ctx, const float* dev_dets, const int32_t* dev_counts, int32_t B,
                        int32_t max_det, int32_t H0, int32_t W0, float* dev_xyxy, void* stream);
/* All of the above on one stream (the scored pair of entry points, with the pairs in the workspace).  dev_input_scratch
 * (u8 [B,H,W,3]) may be NULL when H0xW0 == HxW.  mask_mode | VTI_MASK_NATIVE: dev_xyxy is required, vti_scale_boxes runs first
 * and the masks come from vti_masks_native (frame resolution, its layout). */
int32_t vti_predict(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0,
                    int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic,
                    int32_t mask_mode, int32_t packing, uint8_t* dev_input_scratch,
                    float* dev_pred, void* dev_proto, float* dev_dets, int32_t* dev_counts,
                    uint8_t* dev_masks, int32_t capacity, int32_t* dev_offsets, float* dev_xyxy,
                    void* stream);

/* ---- measurement.py's mask post-processing on device ------ */
/* A4 get_instance_mask_as_bitmap (measurement.py:70-86): u8 0/1 masks [n,H,W] ->
 * cv2.INTER_NEAREST resize to H0xW0, (>0); nonzero[i] = count of set pixels. */
int32_t vti_mask_to_frame(vti_ctx* ctx, const uint8_t* dev_masks, int32_t n, int32_t H, int32_t W,
                          int32_t H0, int32_t W0, uint8_t* dev_bitmaps, int32_t* dev_nonzero, void* stream);
/* A5+A6 _combine_masks + _fabric_lower_envelope (measurement.py:160-185): OR of the selected
 * bitmaps and, per column, the largest y with a set pixel (-1 if none). */
int32_t vti_union_envelope(vti_ctx* ctx, const uint8_t* dev_bitmaps, const int32_t* dev_select, int32_t nsel,
                           int32_t H0, int32_t W0, uint8_t* dev_union, int32_t* dev_envelope, void* stream);
/* A7 moments / extents (measurement.py:302-318): per bitmap i64 {m00, m10, m01, min_col, max_col}
 * (min/max = -1 when empty). */
int32_t vti_mask_stats(vti_ctx* ctx, const uint8_t* dev_bitmaps, int32_t n, int32_t H0, int32_t W0,
                       int64_t* dev_stats, void* stream);

/* The same reductions straight from the BIT-PACKED masks vti_masks writes (VTI_PACK_BITS, u8 [n,H,W/8]); the nearest resize of
 * A4 is folded into integer weights, so no [n,H0,W0] bitmap is materialised.  Results are identical to
 * vti_mask_to_frame followed by vti_mask_stats / vti_union_envelope.
 * A4+A7: i64 {m00, m10, m01, min_col, max_col} per instance (measurement.py:70-86,302-318).  dev_n_live (may be NULL) points
 * at the number of live slots of a fixed-capacity buffer (&dev_offsets[B] of vti_masks): slots at and beyond it are not read
 * and report the empty mask {0,0,0,-1,-1}. */
int32_t vti_mask_stats_bits(vti_ctx* ctx, const uint8_t* dev_masks_bits, int32_t n, const int32_t* dev_n_live,
                            int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t* dev_stats, void* stream);
/* A4+A5+A6, batched: envelope i32 [B,W0] = per frame and frame column the largest row covered by any of the frame's instances of
 * class `cls` (cls < 0: every instance), -1 if none (measurement.py:70-86,160-185; the reference selects FABRIC_CLASS_ID,
 * config.py:70).  dev_offsets / dev_dets / capacity as written by vti_masks / vti_nms; H, W are the ctx's. */
int32_t vti_envelope_bits(vti_ctx* ctx, const uint8_t* dev_masks_bits, const int32_t* dev_offsets, const float* dev_dets,
                          int32_t B, int32_t max_det, int32_t capacity, int32_t cls, int32_t H0, int32_t W0,
                          int32_t* dev_envelope, void* stream);

/* ---- measurement geometry, float64 as the reference; ctx may be NULL ------------------------ */
/* pixel_to_world_using_camera_plane (measurement.py:50-65) for n points: cv2.undistortPoints (5 fixed-point iterations of the
 * k1,k2,p1,p2,k3 model) + ray / fabric-plane intersection with the plane of compute_camera_plane (measurement.py:44-48).
 * dev_uv f64 [n,2]; host_K f64[9] row-major, host_dist f64[5], host_R f64[9] row-major, host_t f64[3] in HOST memory
 * (camera_calibration.json / extrinsics.json); dev_xyz f64 [n,3] world metres; dev_valid i32 [n] (0 where the reference
 * returns None: |n . ray| < 1e-9). */
int32_t vti_pixels_to_world(vti_ctx* ctx, const double* dev_uv, int32_t n, const double* host_K, const double* host_dist,
                            const double* host_R, const double* host_t, double* dev_xyz, int32_t* dev_valid, void* stream);
/* kmeans_1d_two_clusters (measurement.py:88-113), batched: dev_values f64 [B,max_n] (counts[b] valid entries per row, max_n <=
 * 1024) -> dev_labels i32 [B,max_n] (0 beyond counts[b]), dev_centers f64 [B,2]; same iteration and exit rules, means summed in
 * numpy's pairwise order. */
int32_t vti_kmeans1d2(vti_ctx* ctx, const double* dev_values, const int32_t* dev_counts, int32_t B, int32_t max_n,
                      int32_t max_iters, int32_t* dev_labels, double* dev_centers, void* stream);

/* ---- process_frame's measurement record on device (measurement.py:240-510; the drawing: vti_annotate below) ---------- */
/* Settings of vti_measure: the calibration (camera_calibration.json, extrinsics.json; R = cv2.Rodrigues(rvec), row-major) and
 * config.py's measurement settings.  Defaults (config.py): stitch_id 0, fabric_id 1, roi_enabled 1, roi {10, 300, 1270, 760},
 * min_stitches 3, max_px_distance 250, envelope_neighborhood 3, skip_cluster 0, two_row_threshold_px 30, kmeans_iters 10,
 * frame_buffer 8.  drop_empty = 1 mirrors YOLO(drop_empty_masks=True): instances whose mask (as predict returns it) is empty do
 * not exist.  frame_buffer is the host's smoothing window (the per-frame median over the last frame_buffer averages); vti_measure
 * itself does not read it. */
typedef struct {
    double K[9], dist[5], R[9], t[3];
    double max_px_distance;            /* keep a stitch when |cy - round(median envelope)| < this (measurement.py:419-420) */
    double two_row_threshold_px;       /* skip_cluster: cy spread above this means two rows (measurement.py:378-386) */
    int32_t stitch_id, fabric_id;      /* class ids, >= 0 and different */
    int32_t roi_enabled;
    int32_t roi[4];                    /* x_min, y_min, x_max, y_max in frame px; clamped to the frame, inactive if degenerate */
    int32_t min_stitches;              /* >= 1: an average needs at least this many values */
    int32_t envelope_neighborhood;     /* 0..64 columns either side of a stitch centre */
    int32_t skip_cluster;              /* 0: 2-means row selection; 1: the median split */
    int32_t kmeans_iters;              /* kmeans_1d_two_clusters' max_iters (the reference passes none: 10) */
    int32_t drop_empty;
    int32_t frame_buffer;
} vti_measure_params;

/* vti_measure's frame_i32 status and stitch_i32 flag bits. */
enum { VTI_MEASURE_OK = 0, VTI_MEASURE_NO_FABRIC = 1, VTI_MEASURE_NO_STITCHES = 2,
       VTI_MEASURE_BAD_CAMERA = 3 };   /* vti_measure_cameras only: the frame's camera index is outside [0, n_cams) */
enum { VTI_STITCH_KEPT = 1,       /* a stitch of stitch_meta: exists, class stitch_id, inside the ROI */
       VTI_STITCH_MASK = 2,       /* moments / extents from its mask (else the int-box fall-backs) */
       VTI_STITCH_SELECTED = 4,   /* in the selected row */
       VTI_STITCH_NEAR = 8,       /* within max_px_distance of the envelope (any stitch, selected or not) */
       VTI_STITCH_DIST = 16,      /* contributed to the edge distance (final set, edge and both points valid) */
       VTI_STITCH_WIDTH = 32 };   /* contributed to the stitch width */
/* Largest max_det vti_measure takes (the per-frame tables live in LDS). */
#define VTI_MEASURE_MAX_DET 1000

/* Host only: bytes of device scratch vti_measure needs for B frames, `capacity` mask slots and W0-px frames (0 on a bad argument). */
int64_t vti_measure_scratch_bytes(const vti_ctx* ctx, int32_t B, int32_t capacity, int32_t W0);
/* process_frame's measurement for B frames at once, from the outputs of one predict (vti_predict / vti_nms + vti_masks or
 * vti_masks_native + vti_scale_boxes): per frame b the instances are slots offsets[b] .. offsets[b] + counts[b] in detection order,
 * class dets[b,i,5], frame-px box dev_xyxy[b,i] (vti_scale_boxes).  native = 0: dev_masks are vti_masks' VTI_PACK_BITS slots at the
 * ctx's H x W (16-byte aligned), nearest-resized to H0 x W0 as measurement.py:70-86 does; native = 1: the frame-size rows of
 * vti_masks_native (8*ceil(W0/64) bytes, zero pad bits, 8-byte aligned).  A slot at or beyond `capacity` is an empty mask.  Masks
 * are zero outside their box (grown by 8 letterbox px; frame-px rows [y1, y2) for native rows), as vti_masks writes them.
 * dev_scratch: >= vti_measure_scratch_bytes(), 256-byte aligned.  Every argument check (VTI_ERR_ARG; a smaller scratch included)
 * runs before the first HIP call.  Outputs (device):
 *   frame_f64 [B,2]  avg_dist_mm, avg_width_mm (NaN for the reference's None)
 *   frame_i32 [B,6]  status (VTI_MEASURE_*), n_stitch (stitch_meta), n_fabric (non-empty kept fabric masks), n_selected, n_dist
 *                    (= the record's stitch_count when status is 0), n_width; n_selected, n_dist, n_width are 0 unless status is 0
 *   stitch_f64 [capacity,7] (may be NULL)  cx, cy, left, right, width_mm, edge_y, dist_mm; NaN where not computed (widths, edges
 *                    and distances only when status is 0, edges and distances only for the final set)
 *   stitch_i32 [capacity,2] (may be NULL)  VTI_STITCH_* flags, rank in stitch_meta (-1: not a stitch)
 * Per-slot rows are written for every slot offsets[b] + i (i < counts[b]) below capacity; other rows are left untouched.
 * Three launches on `stream`; no host synchronisation.  Smoothing over frames (measurement.py:474-484) is the caller's. */
int32_t vti_measure(vti_ctx* ctx, const vti_measure_params* params, const uint8_t* dev_masks, int32_t native, const float* dev_dets,
                    const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets, int32_t B, int32_t max_det,
                    int32_t capacity, int32_t H0, int32_t W0, void* dev_scratch, size_t scratch_bytes, double* frame_f64,
                    int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32, void* stream);

/* ---- the stitch-distance checker's measurement on device (Utils/check_stitch_distance.py:281-553; the drawing: vti_annotate_checker) */
/* Settings of vti_measure_checker: the calibration as in vti_measure_params, and the checker's module constants.  Defaults
 * (check_stitch_distance.py:20-39): stitch_id 0, fabric_id 1, min_stitches 3, max_px_distance 150, envelope_neighborhood 3,
 * skip_cluster 0, kmeans_iters 10, frame_buffer 8.  There is no ROI and no two_row threshold: the checker has neither.  drop_empty
 * and frame_buffer: as in vti_measure_params. */
typedef struct {
    double K[9], dist[5], R[9], t[3];
    double max_px_distance;            /* keep a stitch when 0 < cy - round(median envelope) < this (:442-443) */
    int32_t stitch_id, fabric_id;      /* class ids, >= 0 and different */
    int32_t min_stitches;              /* >= 1: an average needs at least this many values */
    int32_t envelope_neighborhood;     /* 0..64 columns either side of a stitch centre */
    int32_t skip_cluster;              /* 0: 2-means row selection; 1: every stitch is selected */
    int32_t kmeans_iters;              /* kmeans_1d_two_clusters' max_iters (the checker passes none: 10) */
    int32_t drop_empty;
    int32_t frame_buffer;
} vti_checker_params;

/* The checker's process_frame for B frames of one size at once, from the outputs of one predict.  Inputs, `native`, the scratch
 * (vti_measure_scratch_bytes(), 256-byte aligned) and the four outputs' layouts are vti_measure's; every argument check (VTI_ERR_ARG,
 * max_det above VTI_MEASURE_MAX_DET included) runs before the first HIP call.  What the checker computes differently:
 *   - no ROI.  Every kept fabric_id instance joins the fabric union: its nearest-resized mask if that has a set pixel, else the
 *     filled rectangle (int x1, int y1)..(int x2, int y2), corners inclusive, clipped to the frame (:329-334).  n_fabric counts
 *     all of them.  With drop_empty = 1 an instance whose mask is empty as predict returns it does not exist, box included.
 *     VTI_MEASURE_NO_FABRIC when the union is empty;
 *   - the fabric edge is the UPPER envelope: the smallest set row per column, -1 where there is none (:238-251);
 *   - row selection (:408-429): 2-means on the centroids' y with the checker's own kmeans_1d_two_clusters (:143-171, which returns
 *     the labels of its last assignment); the chosen cluster is the one whose mean is nearer to the mean envelope row, a tie is
 *     cluster 1; skip_cluster = 1 or fewer than 2 stitches: every stitch;
 *   - VTI_STITCH_NEAR is the signed test 0 < cy - round(median) < max_px_distance: the stitch lies strictly below the edge
 *     (:431-444, any stitch); the final set is the selected stitches with it, or every selected stitch when none has it;
 *   - width_mm, edge_y, dist_mm, VTI_STITCH_WIDTH and VTI_STITCH_DIST are set for the final set only.  A width whose left or
 *     right end has no world point is px_width / 10 * |world(cx + 10, cy) - world(cx, cy)| when those two exist (:488-507);
 *   - n_dist = len(per_dists), n_width = len(per_widths): the `n` of the checker's info text (:515, :533-540).
 * Three launches on `stream`; no host synchronisation.  Smoothing over frames (:519-530) is the caller's. */
int32_t vti_measure_checker(vti_ctx* ctx, const vti_checker_params* params, const uint8_t* dev_masks, int32_t native,
                            const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                            int32_t B, int32_t max_det, int32_t capacity, int32_t H0, int32_t W0, void* dev_scratch,
                            size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32,
                            void* stream);

/* ---- vti_measure for a batch that mixes cameras: every setting of vti_measure_params per frame ------------------------------ */
/* The settings live in a camera table in caller-owned DEVICE memory, one row per camera, and an i32 [B] device array names each
 * frame's row.  The table is packed on the host, uploaded once and reused; it does not depend on the frame size (the ROI is clamped
 * to H0 x W0 on the device).
 * Host only: bytes of a table of n_cams rows (0 when n_cams < 1). */
int64_t vti_measure_cameras_bytes(int32_t n_cams);
/* Host only: validates params[0 .. n_cams) with exactly vti_measure's checks of its one struct (VTI_ERR_ARG; vti_last_error names
 * the index of the first failing camera) and writes the table into host_table (nbytes >= vti_measure_cameras_bytes(n_cams)).  A
 * row holds the struct's settings plus the plane of compute_camera_plane (measurement.py:44-48); the format is private to the
 * library build that packed it, and equal inputs give equal bytes.  ctx only receives the error text. */
int32_t vti_measure_pack_cameras(vti_ctx* ctx, const vti_measure_params* params, int32_t n_cams, void* host_table, size_t nbytes);
/* vti_measure with frame b measured under row dev_camera_of_frame[b] of dev_cameras (16-byte aligned device copy of a packed
 * table); every other argument, the scratch size (vti_measure_scratch_bytes), the outputs and the three launches are vti_measure's,
 * and frame b's results are bit-identical to those of vti_measure called with that camera's struct on the same inputs.  Every
 * argument check (null table or index array, n_cams < 1, then vti_measure's shape, pointer, alignment and scratch checks) runs
 * before the first HIP call; the settings were checked when the table was packed.
 * The index array is device data the host cannot check: the kernels compare dev_camera_of_frame[b] with [0, n_cams) BEFORE they
 * form a table address.  A frame whose index is outside reports status VTI_MEASURE_BAD_CAMERA, NaN averages, zero counts, and
 * flags 0 / rank -1 / NaN in the per-slot rows of its instances; the other frames are unaffected.  The table's CONTENTS are
 * trusted to be what vti_measure_pack_cameras wrote: its validation is what bounds the kernels' loops (envelope_neighborhood <=
 * 64, kmeans_iters >= 0), so bytes from anywhere else are undefined behaviour. */
int32_t vti_measure_cameras(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams, const int32_t* dev_camera_of_frame,
                            const uint8_t* dev_masks, int32_t native, const float* dev_dets, const float* dev_xyxy,
                            const int32_t* dev_counts, const int32_t* dev_offsets, int32_t B, int32_t max_det, int32_t capacity,
                            int32_t H0, int32_t W0, void* dev_scratch, size_t scratch_bytes, double* frame_f64, int32_t* frame_i32,
                            double* stitch_f64, int32_t* stitch_i32, void* stream);

/* ---- batches whose frames differ in size: one call for cameras of several resolutions ---------------------------------------- */
/* Ultralytics letterboxes the sources of one predict() that do not share a shape with LetterBox(imgsz, auto=False): every frame is
 * resized by its own gain and centred on one common H x W canvas (the ctx's), and boxes, polygons and everything else in frame
 * pixels is mapped back with that frame's own gain and pads.  Here the B frames lie back to back in ONE device buffer (frame b:
 * u8 [H0[b], W0[b], 3] at byte_offset[b], a multiple of 16) and a FRAME TABLE describes them: packed and validated on the host,
 * uploaded once and reused while the same frame sizes keep the same batch positions (a fixed camera rig).  A row holds what the
 * kernels would otherwise recompute per pixel or per box: the resized size and pads, the resize scales, the scale_boxes gain and
 * pads (double, then one cast to f32, as vti_scale_boxes rounds them), the frame's offset and size; the header holds B, the
 * canvas, the largest H0 and W0 and total_bytes.  The format is private to the library build that packed it.
 * Host only: bytes of a table of B frames (0 when B < 1). */
int64_t vti_frame_table_bytes(int32_t B);
/* Host only: validates frame b = 0 .. B-1 for an H x W canvas (multiples of 32) -- 1 <= H0, W0 <= 16384, byte_offset >= 0 and a
 * multiple of 16, byte_offset + 3 * H0 * W0 <= total_bytes (the size of the frame buffer), the resized frame not below 1 px --
 * with VTI_ERR_ARG and the index of the first failing frame in vti_last_error, then writes the table into host_table (nbytes >=
 * vti_frame_table_bytes(B)).  Equal inputs give equal bytes.  ctx only receives the error text (may be NULL). */
int32_t vti_pack_frames(vti_ctx* ctx, int32_t H, int32_t W, const int32_t* H0, const int32_t* W0, const int64_t* byte_offset,
                        int32_t B, int64_t total_bytes, void* host_table, size_t nbytes);
/* Host only: what a packed table holds.  b = -1: out_i32 = {B, H, W, max H0, max W0, 0, total_bytes lo, hi}; 0 <= b < B: out_i32 =
 * {H0, W0, new_h, new_w, top, left, byte_offset lo, hi} and out_f64 (may be NULL) = {scale_x, scale_y, gain, padx, pady} (the
 * resize scales 1 / (new / orig); the scale_boxes values as the f32 the kernels use). */
int32_t vti_frame_table_info(const void* host_table, int32_t b, int32_t out_i32[8], double out_f64[5]);
/* The *_frames calls below take the table twice: host_table, the bytes vti_pack_frames wrote, and dev_table, their copy in device
 * memory (16-byte aligned).  Every argument check runs before the first HIP call, and it includes the table: host_table must be a
 * packed table for this ctx's canvas and for exactly B frames, and every row of it is validated again, so each value a kernel forms
 * an address from (offset, sizes, pads) was checked by the host at the call.  The device copy's CONTENTS are trusted to be those
 * same bytes, as the camera table's are: other bytes there are undefined behaviour.
 * U1 for B frames of individual sizes -> u8 [B,H,W,3]; every byte of dev_input is written.  Frame b's canvas equals what
 * vti_letterbox writes for that frame alone.  dev_frames 16-byte aligned, dev_input 4-byte aligned, B <= max_batch. */
int32_t vti_letterbox_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t B,
                             uint8_t* dev_input, void* stream);
/* U8 with gain, pads and clip bounds of frame b from its row: the same expression and rounding as vti_scale_boxes(H0[b], W0[b]). */
int32_t vti_scale_boxes_frames(vti_ctx* ctx, const float* dev_dets, const int32_t* dev_counts, const void* host_table,
                               const void* dev_table, int32_t B, int32_t max_det, float* dev_xyxy, void* stream);
/* vti_predict for such a batch: vti_letterbox_frames (always; dev_input_scratch is required), the scored forward, NMS, vti_masks
 * (masks at the canvas size, as Ultralytics' masks.data) and, when dev_xyxy is given, vti_scale_boxes_frames; one stream, no host
 * synchronisation.  mask_mode | VTI_MASK_NATIVE is VTI_ERR_UNSUPPORTED here: frame-resolution masks of frames of differing sizes do
 * not fit this call's slots of one size; they are vti_predict_frames_native's, below. */
int32_t vti_predict_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t B,
                           int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode,
                           int32_t packing, uint8_t* dev_input_scratch, float* dev_pred, void* dev_proto, float* dev_dets,
                           int32_t* dev_counts, uint8_t* dev_masks, int32_t capacity, int32_t* dev_offsets, float* dev_xyxy,
                           void* stream);
/* vti_measure_cameras with H0, W0 of frame b from the frame table (ROI clamp, column clip, resize of the masks): frame b's results
 * are bit-identical to those of vti_measure_cameras called with H0[b], W0[b] on the same inputs.  Letterbox bit masks only: native
 * = 1 is VTI_ERR_UNSUPPORTED (the ragged frame-size rows are vti_measure_frames_native's, below).  dev_scratch: >=
 * vti_measure_scratch_bytes(ctx, B, capacity, largest W0 of the table) (the envelope rows are pitched by it).  The slot -> frame
 * search of the moment kernel runs over dev_offsets[0 .. B] and ends inside [0, B) whatever they hold. */
int32_t vti_measure_frames(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams, const int32_t* dev_camera_of_frame,
                           const uint8_t* dev_masks, int32_t native, const float* dev_dets, const float* dev_xyxy,
                           const int32_t* dev_counts, const int32_t* dev_offsets, const void* host_table, const void* dev_table,
                           int32_t B, int32_t max_det, int32_t capacity, void* dev_scratch, size_t scratch_bytes, double* frame_f64,
                           int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32, void* stream);

/* ---- frame-resolution masks for frames of differing sizes: the ragged mask buffer --------------------------------------- */
/* retina_masks for a batch of vti_pack_frames.  Frames of different sizes have slots of different byte sizes, so the masks of one
 * call lie in one flat, 8-byte aligned u8 buffer, bit-packed (VTI_PACK_BITS only; VTI_PACK_U8 is VTI_ERR_UNSUPPORTED):
 *   - a slot of frame b has the layout vti_mask_native_layout(H0[b], W0[b], VTI_PACK_BITS) gives: H0[b] rows of row_bytes[b] =
 *     8*ceil(W0[b]/64) bytes, LSB-first, bits at columns >= W0[b] zero; slot_bytes[b] = H0[b] * row_bytes[b];
 *   - the slots lie back to back, frame-major, in detection order.  dev_offsets i32 [B+1] is vti_masks' prefix sum of the clamped
 *     counts (instance i of frame b is slot INDEX offsets[b] + i: the row of every per-slot output), and dev_mask_bases i64 [B+1]
 *     holds bases[b] = sum over b' < b of clamp(counts[b']) * slot_bytes[b'], not clipped by the capacity: instance i of frame b
 *     starts at BYTE bases[b] + i * slot_bytes[b].  Every base is a multiple of 8;
 *   - the capacity is in bytes: an instance is live iff its slot ends at or before capacity_bytes.  The bases are monotone, so the
 *     live instances are a prefix of the slot order; live slots are written completely and no byte after the last live slot is
 *     touched: no byte of a slot that did not fit is written.
 * Host only: the worst case, max_det slots for every frame of the table: sum over b of max_det * slot_bytes[b]; 0 on a bad argument
 * (NULL, max_det < 1, not a valid packed table for this ctx's canvas, more frames than max_batch). */
int64_t vti_mask_native_frames_bytes(const vti_ctx* ctx, const void* host_table, int32_t max_det);
/* vti_masks_native for such a batch: frame b's live slots are byte for byte those vti_masks_native(..., H0[b], W0[b], ...) writes for
 * frame b from the same dets, xyxy (vti_scale_boxes_frames), counts and prototypes -- one function computes a frame size's crop, scales,
 * tile height and slot layout for both calls.  Writes dev_offsets and dev_mask_bases (also when capacity_bytes is 0, and nothing else
 * then).  The table pair is checked as by every *_frames call; nm must be 32; every argument check runs before the first HIP call. */
int32_t vti_masks_native_frames(vti_ctx* ctx, const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                                const void* dev_proto, const void* host_table, const void* dev_table, int32_t B, int32_t max_det,
                                int32_t mode, int32_t packing, uint8_t* dev_masks, int64_t capacity_bytes, int32_t* dev_offsets,
                                int64_t* dev_mask_bases, void* stream);
/* vti_predict_frames with those masks: vti_letterbox_frames, the scored forward, NMS, vti_scale_boxes_frames (dev_xyxy is required)
 * and vti_masks_native_frames; one stream, no host synchronisation.  mask_mode: VTI_MASK_LOGIT or VTI_MASK_SIGMOID (the
 * VTI_MASK_NATIVE flag is implied and ignored).  dev_dets, dev_counts, dev_xyxy and dev_offsets are those of vti_predict_frames. */
int32_t vti_predict_frames_native(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t B,
                                  int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode,
                                  int32_t packing, uint8_t* dev_input_scratch, float* dev_pred, void* dev_proto, float* dev_dets,
                                  int32_t* dev_counts, uint8_t* dev_masks, int64_t capacity_bytes, int32_t* dev_offsets,
                                  int64_t* dev_mask_bases, float* dev_xyxy, void* stream);
/* vti_measure_frames on those rows (there is no `native` argument: the rows are the frame's own pixels, so the nearest resize of
 * measurement.py:70-86 is the identity).  dev_mask_bases and capacity_bytes: as vti_masks_native_frames wrote and took them;
 * `capacity` stays the number of rows of the per-slot outputs and the sizing of vti_measure_scratch_bytes(ctx, B, capacity, largest
 * W0).  A slot that is not live by the byte rule, or whose index is >= capacity, is an empty mask.  Frame b's results are
 * bit-identical to those of vti_measure_cameras(native = 1) at H0[b], W0[b] on frame b's rows. */
int32_t vti_measure_frames_native(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams, const int32_t* dev_camera_of_frame,
                                  const uint8_t* dev_masks, const int64_t* dev_mask_bases, int64_t capacity_bytes,
                                  const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                                  const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t capacity,
                                  void* dev_scratch, size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64,
                                  int32_t* stitch_i32, void* stream);

/* ---- Results.masks.xy on device: instance polygons in frame pixels ---------------------------------------------------- */
/* Ultralytics masks2segments + scale_coords as restated by the package's polygons.py, bit for bit: per mask the outer border of
 * every 8-connected component (traced from its top-most, then left-most pixel; pixels outside H x W, the pad bits of padded rows
 * included, are background), CHAIN_APPROX_SIMPLE-compressed, then mapped to the H0 x W0 frame as scale_coords((H, W), pts,
 * (H0, W0)): gain and pad in double, each rounded to f32 once, (x - pad) / gain in f32 with correctly rounded division, clipped
 * to [0, W0] and [0, H0].  Unlike OpenCV's RETR_EXTERNAL, a component inside a hole of another one has a border of its own.
 * VTI_POLY_LARGEST: the contour with the most vertices (ties: the first in raster order of the start pixels); VTI_POLY_CONCAT:
 * every contour, in raster order of the start pixels.  An empty mask has 0 vertices. */
#define VTI_POLY_LARGEST 0
#define VTI_POLY_CONCAT  1
/* Status word: the first int32 of dev_scratch after a vti_mask_polygons call has run (0 = ok). */
enum { VTI_POLY_OK = 0,
       VTI_POLY_ERR_BOUND = 1,    /* a labelling or border-following loop reached its bound (size-derived); points not written */
       VTI_POLY_ERR_RANGE = 2 };  /* the total vertex count is above INT32_MAX; offsets saturate, points not written */
/* Host only: device scratch bytes vti_mask_polygons needs for H x W masks with row_bytes bytes per row (0 on a bad argument).
 * It depends on neither the mask count nor the contents: 128 labelling areas of 8 * H * ceil(W/2) + 4 * (H + 1) bytes, plus 8 * H
 * * ceil(W/64) bytes each when the mask does not fit in LDS (H * ceil(W/64) * 8 > 156 KiB).  736 x 960: 362 MB; 960 x 1280: 630 MB. */
int64_t vti_mask_polygons_scratch_bytes(const vti_ctx* ctx, int32_t H, int32_t W, int32_t row_bytes);
/* dev_masks_bits: u8 [n, H, row_bytes] LSB-first bit masks, W <= 8 * row_bytes real columns: vti_masks' VTI_PACK_BITS slots
 * (row_bytes = W/8) or vti_masks_native's rows (row_bytes = 8*ceil(W0/64), W = W0).  dev_n_live (may be NULL): slots at and beyond
 * *dev_n_live are not read and have 0 vertices (&dev_offsets[B] of vti_masks).  1 <= H, W <= 16384, H * W <= 2^26.
 * dev_point_offsets i32 [n+1] always receives the exclusive scan of the per-slot vertex counts; dev_points f32 [max_points, 2]
 * (x, y) receives slot i's vertices at rows offsets[i] .. offsets[i+1] only when offsets[n] <= max_points (otherwise nothing is
 * written there: call again with a larger buffer).  dev_scratch: >= vti_mask_polygons_scratch_bytes(), 256-byte aligned; its
 * first int32 is the status word (VTI_POLY_*) once the work has run.  Every argument check (VTI_ERR_ARG) runs before the first
 * HIP call.  Three launches on `stream` (count, scan, write); no host synchronisation. */
int32_t vti_mask_polygons(vti_ctx* ctx, const uint8_t* dev_masks_bits, int32_t n, const int32_t* dev_n_live, int32_t H, int32_t W,
                          int32_t row_bytes, int32_t H0, int32_t W0, int32_t strategy, void* dev_scratch, size_t scratch_bytes,
                          int32_t* dev_point_offsets, float* dev_points, int64_t max_points, void* stream);

/* ---- the polygons of a whole batch whose frames differ in size: vti_mask_polygons on the slots of a frame table ---------------- */
/* The two calls of this section carry this (empty) marker. */
#define VTI_POLYGONS_FRAMES_API
/* Host only: device scratch bytes vti_mask_polygons_frames needs for the frames of host_table (0 on a bad argument: NULL, native
 * outside {0, 1}, not a table of vti_pack_frames for this ctx's canvas, a native frame above H0 * W0 = 2^26).  256 header bytes and
 * 128 labelling areas, each part of an area sized for the largest geometry of the table by vti_mask_polygons_scratch_bytes' formula:
 * native = 0: the canvas, so the value of vti_mask_polygons_scratch_bytes(H, W, W/8); native = 1: the maximum over the frames, the
 * image part counted for the frames that do not fit in LDS. */
VTI_POLYGONS_FRAMES_API int64_t vti_mask_polygons_frames_scratch_bytes(const vti_ctx* ctx, const void* host_table, int32_t native);
/* One vti_mask_polygons for the output set of vti_predict_frames (native = 0) or vti_predict_frames_native (native = 1): slot s
 * belongs to the frame b with dev_offsets[b] <= s < dev_offsets[b+1] (i32 [B+1]; the search ends inside [0, B) whatever the array
 * holds, and a table address is formed only then) and its vertices are, bit for bit, what vti_mask_polygons writes for that slot
 *   native = 0: with (H, W, W/8, H0[b], W0[b]) on dev_masks = u8 [capacity, H, W/8], the letterbox bit masks at the ctx's canvas
 *               (16-byte aligned; dev_mask_bases must be NULL);
 *   native = 1: with (H0[b], W0[b], 8*ceil(W0[b]/64), H0[b], W0[b]) on instance i of frame b = H0[b] rows of 8*ceil(W0[b]/64) bytes at
 *               byte dev_mask_bases[b] + i * slot_bytes[b] of dev_masks (8-byte aligned; dev_mask_bases i64 [B+1], 8-byte aligned).
 *               Every frame needs H0 * W0 <= 2^26.
 * A slot is live when its index is below min(dev_offsets[B], capacity) and, native = 1, its rows end at or before capacity_bytes; any
 * other slot is not read and has 0 vertices.  Outputs, status word, strategy and the max_points rule as vti_mask_polygons, with n =
 * capacity.  dev_scratch: >= vti_mask_polygons_frames_scratch_bytes(), 256-byte aligned.  The table pair is revalidated as by every
 * *_frames call; 1 <= B <= max_batch.  Every argument check (VTI_ERR_ARG) runs before the first HIP call.  Count and write are
 * launched once per form the table holds (image in LDS / in the scratch): three launches on `stream`, five when both occur. */
VTI_POLYGONS_FRAMES_API int32_t vti_mask_polygons_frames(vti_ctx* ctx, const uint8_t* dev_masks, int32_t native,
        const int64_t* dev_mask_bases, int64_t capacity_bytes, const int32_t* dev_offsets,
        const void* host_table, const void* dev_table, int32_t B, int32_t capacity, int32_t strategy,
        void* dev_scratch, size_t scratch_bytes, int32_t* dev_point_offsets, float* dev_points, int64_t max_points,
        void* stream);

/* ---- process_frame's annotated frame on device (measurement.py:219-504): the overlay on a selection of the batch -------------- */
/* The reference returns (annotated, measurements); vti_measure gives the second half, this call the first, for the n_sel frames
 * the caller wants a picture of (the ones a limit check flagged, every k-th, ...).  dev_out[k] is frame select[k] of dev_frames
 * (u8 [B,H0,W0,3] BGR, the batch predict consumed) with, in the reference's order and BGR colours: the clamped ROI (144,238,144) 2 px;
 * per ROI-kept instance in detection order its int-truncated box, stitch (255,255,0) 1 px, fabric (255,0,255) 2 px; [status
 * NO_FABRIC stops here] the lower envelope of the union of the kept fabric masks, every max(1, n / 1000)-th valid column, as an open
 * polyline (255,128,0) 2 px; [NO_STITCHES stops here] per stitch of stitch_meta in rank order filled circles r = 3 (200,200,0) at
 * (round(left), round(cy)) and (round(right), round(cy)), the 1-px line between them, a filled circle r = 3 (200,0,0) at (round(cx),
 * round(cy)); per stitch with VTI_STITCH_DIST a 1-px line (0,255,0) from (clip(round(cx)), round(edge_y)) to (round(cx), round(cy))
 * and a filled circle r = 2 (255,0,255) at the edge point; every outer contour of the union (the tracer of vti_mask_polygons,
 * CHAIN_APPROX_SIMPLE) as a closed polyline (0,0,255) 2 px.  round = half to even.  A later primitive overwrites an earlier one.
 * The pixels of a primitive are those of the package's annotate.py (OpenCV's LINE_8, shift = 0 drawing restated: LineIterator
 * walk, fixed-point thick-line quad with its outline and round caps, midpoint-circle spans), byte for byte; text is the host's
 * (annotate.text_items / put_text).  A frame with status VTI_MEASURE_BAD_CAMERA, or whose device camera index is outside [0, n_cams)
 * (compared in the kernels before a table address is formed), is copied as it is.
 * dev_cameras: a table of vti_measure_pack_cameras (16-byte aligned; one camera = a one-row table); dev_camera_of_frame i32 [B], or
 * NULL: row 0 for every frame.  Masks, dets, xyxy, counts, offsets, max_det, capacity, native: as vti_measure took them; frame_i32,
 * stitch_f64, stitch_i32: what it wrote (all three required).  The selection is given twice, as the frame table is: host_select
 * i32 [n_sel] is checked before the first HIP call (every entry in [0, B); any order, duplicates allowed) and dev_select is its
 * device copy, trusted to hold the same values.  1 <= H0, W0 <= 8192; 1 <= max_det <= VTI_MEASURE_MAX_DET; max_points >= 0 is the
 * room for the outline's vertices per frame.  dev_out u8 [n_sel,H0,W0,3]: every byte is written; nothing else is (dev_frames and the
 * frames not selected stay as they are).  dev_status i32 [n_sel]: 0, or VTI_ANNOTATE_OUTLINE_SKIPPED when the outline needed more than
 * max_points vertices or the tracer reached its bound -- that frame is drawn without its outline, everything else stands.
 * dev_scratch: >= vti_annotate_scratch_bytes(), 256-byte aligned.  Every argument check (VTI_ERR_ARG) runs before the first HIP call.
 * Three launches on `stream` (display list + union, outline, raster); no host synchronisation.  Frames of differing sizes (a frame
 * table): vti_annotate_frames below. */
enum { VTI_ANNOTATE_OUTLINE_SKIPPED = 1 };
/* Host only: bytes of device scratch vti_annotate needs (0 on a bad argument); it grows with n_sel and with max_points. */
int64_t vti_annotate_scratch_bytes(const vti_ctx* ctx, int32_t n_sel, int32_t max_det, int32_t H0, int32_t W0, int32_t max_points);
int32_t vti_annotate(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0, const void* dev_cameras,
                     int32_t n_cams, const int32_t* dev_camera_of_frame, const uint8_t* dev_masks, int32_t native,
                     const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                     int32_t max_det, int32_t capacity, const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                     const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t max_points, uint8_t* dev_out,
                     int32_t* dev_status, void* dev_scratch, size_t scratch_bytes, void* stream);
/* vti_annotate for a batch whose frames differ in size.  dev_frames / host_table / dev_table: the flat frame buffer and the frame table
 * of vti_predict_frames / vti_measure_frames (frame b: u8 [H0[b], W0[b], 3] BGR at byte_offset[b]); masks, dets, xyxy, counts, offsets:
 * as vti_measure_frames took them; frame_i32, stitch_f64, stitch_i32: what it wrote.  The OUTPUT is described by a second frame table,
 * the out table: n_sel rows packed with vti_pack_frames for the same canvas, row k with the H0, W0 of input row select[k] (otherwise
 * VTI_ERR_ARG, and vti_last_error names k); its byte offsets place picture k in dev_out and its total_bytes is the size of dev_out, so
 * one table type describes every ragged frame buffer of the library and (dev_out, out table) feeds vti_encode_jpeg_frames and
 * vti_predict_frames directly.  Every byte of each output picture is written and no other: not the gaps between pictures, not the
 * bytes past the last one; dev_frames is never written.  Picture k is byte for byte what vti_annotate writes for that frame when
 * called with H0[b], W0[b] on the same inputs; status, VTI_ANNOTATE_OUTLINE_SKIPPED, the plain copy of a frame with a bad camera,
 * duplicates and any order of the selection are vti_annotate's.  native = 1 is VTI_ERR_UNSUPPORTED (this call takes letterbox bit
 * masks only; the ragged frame-size rows are vti_annotate_frames_native's, below); a SELECTED frame above 8192 in either dimension
 * is VTI_ERR_ARG naming the frame (the table allows 16384, the raster's fixed point does not).  dev_frames and dev_out 16-byte aligned.  Every argument check -- both tables revalidated row by
 * row and the selection included -- runs before the first HIP call; the device copies (tables, selection) are trusted as the other
 * *_frames calls trust theirs.  The scratch regions are pitched by the largest selected frame; what lies in a region beyond a frame's
 * own extent is never read.  Three launches on `stream`, or four when the selection holds both frames whose union fits the tracer's
 * LDS image (H0 * ceil(W0 / 64) * 8 <= 156 KiB) and frames whose union does not: the outline kernel then runs in both forms, each on
 * its own frames.
 * Host only: scratch bytes for the pictures the out table describes (0 on a bad argument) = vti_annotate_scratch_bytes(n_sel, max_det,
 * largest H0, largest W0 of its rows, max_points). */
int64_t vti_annotate_frames_scratch_bytes(const vti_ctx* ctx, const void* host_out_table, int32_t max_det, int32_t max_points);
int32_t vti_annotate_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t B,
                            const void* dev_cameras, int32_t n_cams, const int32_t* dev_camera_of_frame, const uint8_t* dev_masks,
                            int32_t native, const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                            const int32_t* dev_offsets, int32_t max_det, int32_t capacity, const int32_t* frame_i32,
                            const double* stitch_f64, const int32_t* stitch_i32, const int32_t* host_select, const int32_t* dev_select,
                            int32_t n_sel, int32_t max_points, const void* host_out_table, const void* dev_out_table, uint8_t* dev_out,
                            int32_t* dev_status, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- the stitch-distance checker's picture on device (Utils/check_stitch_distance.py:293-545): vti_annotate for the checker -------- */
/* The checker returns (annotated, info_text); vti_measure_checker gives the second half, this call the first, for the n_sel frames
 * the caller wants a picture of.  dev_out[k] is frame select[k] of dev_frames (u8 [B,H0,W0,3] BGR, one frame size) with, in the
 * checker's order and BGR colours:
 *   a. per existing instance in detection order its int-truncated box, stitch (255,255,0) 1 px, fabric (255,0,255) 2 px (:323-336).
 *      There is no ROI and no keep test; "existing" is vti_measure_checker's rule: with drop_empty = 1 an instance whose mask is
 *      empty as predict returns it, or whose slot is at or past `capacity`, does not exist and has no box; with drop_empty = 0 every
 *      instance has one;
 *   b. [status VTI_MEASURE_NO_FABRIC stops here (:345-347)]
 *   c. the UPPER envelope of the fabric union -- the union of vti_measure_checker: per existing fabric instance its nearest-resized
 *      mask when that has a set pixel, else the filled rectangle (int x1, int y1)..(int x2, int y2), corners inclusive, clipped to
 *      the frame -- the smallest set row per column, every max(1, n / 1000)-th valid column, as an open polyline (255,128,0) 2 px
 *      (:349-360);
 *   d. [VTI_MEASURE_NO_STITCHES stops here (:404-406)]
 *   e. per stitch of the FINAL set (VTI_STITCH_SELECTED and VTI_STITCH_NEAR when any selected stitch is near, else every selected
 *      stitch) in rank order, its primitives together (:465-510): with VTI_STITCH_DIST a 1-px line (0,255,0) from (clip(round(cx), 0,
 *      W0 - 1), round(edge_y)) to (round(cx), round(cy)) and a filled circle r = 2 (255,0,255) at the edge point; with
 *      VTI_STITCH_WIDTH and when world(left, cy) and world(right, cy) both exist (|n . ray| >= 1e-9; a width from the local-scale
 *      estimate sets the flag and draws nothing) filled circles r = 3 (200,200,0) at (round(left), round(cy)) and (round(right),
 *      round(cy)) and the 1-px line between them; always a filled circle r = 4 (0,255,0) at (round(cx), round(cy));
 *   f. every outer contour of that union, filled boxes included (the tracer of vti_mask_polygons, CHAIN_APPROX_SIMPLE), as a closed
 *      polyline (255,128,0) 2 px (:543-545).
 * round = half to even.  A later primitive overwrites an earlier one.  The pixels of a primitive are vti_annotate's, byte for byte the
 * package's annotate.rasterise(frame, annotate.checker_display_list(...)); text is the host's (measure.checker_text_items /
 * annotate.put_text; all of it is drawn last).  A frame whose status is none of OK, NO_FABRIC, NO_STITCHES is copied as it is.
 * params: the struct vti_measure_checker took (its calibration decides the width markers; the class ids and drop_empty the boxes and
 * the union), checked as there.  Masks, dets, xyxy, counts, offsets, max_det, capacity, native: as vti_measure_checker took them;
 * frame_i32, stitch_f64, stitch_i32: what it wrote (all three required).  host_select / dev_select, n_sel, max_points, dev_out
 * u8 [n_sel,H0,W0,3] (every byte is written, nothing else is; dev_frames is never written), dev_status i32 [n_sel] (0 or
 * VTI_ANNOTATE_OUTLINE_SKIPPED: that frame is drawn without step f) and the limits 1 <= H0, W0 <= 8192, 1 <= max_det <=
 * VTI_MEASURE_MAX_DET are vti_annotate's.  dev_scratch: >= vti_annotate_scratch_bytes(ctx, n_sel, max_det, H0, W0, max_points),
 * 256-byte aligned: the layout is vti_annotate's.  Every argument check (VTI_ERR_ARG; vti_last_error names the argument) runs before
 * the first HIP call.  Three launches on `stream` (the checker's display list + union, then vti_annotate's outline and raster
 * kernels); no host synchronisation.  One frame size and one camera; several of either: vti_annotate_checker_cameras and
 * vti_annotate_checker_frames, below. */
int32_t vti_annotate_checker(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0, const vti_checker_params* params,
                             const uint8_t* dev_masks, int32_t native, const float* dev_dets, const float* dev_xyxy,
                             const int32_t* dev_counts, const int32_t* dev_offsets, int32_t max_det, int32_t capacity,
                             const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                             const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t max_points,
                             uint8_t* dev_out, int32_t* dev_status, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- the stitch-distance checker on a rig: a camera table of checker settings, frames of differing sizes ------------------------ */
/* The rig forms of vti_measure_checker and vti_annotate_checker, as vti_measure and vti_annotate have theirs: the settings of every
 * camera in one table in device memory, an i32 [B] device array that names each frame's row, and for frames of differing sizes the
 * frame table pair of vti_pack_frames.  The arithmetic is the one-struct calls' own: frame b comes out bit for bit (measurement) and
 * byte for byte (picture) as the one-struct call gives it with that camera's struct at that frame's size.
 * Marks the six entry points of the rig forms; libvti.so exports them as it does every other. */
#define VTI_CHECKER_RIG_API
/* Host only: vti_measure_pack_cameras for checker settings.  Validates params[0 .. n_cams) with exactly vti_measure_checker's checks
 * of its one struct (VTI_ERR_ARG; vti_last_error names the index of the first failing camera) and writes one row per camera into
 * host_table.  A checker table has the size of a measure table of as many rows: nbytes >= vti_measure_cameras_bytes(n_cams).  The
 * rows are NOT interchangeable with vti_measure_pack_cameras' (other settings); the format is private to the library build, and
 * equal inputs give equal bytes.  ctx only receives the error text. */
VTI_CHECKER_RIG_API int32_t vti_checker_pack_cameras(vti_ctx* ctx, const vti_checker_params* params, int32_t n_cams, void* host_table,
                                                     size_t nbytes);
/* vti_measure_checker with frame b measured under row dev_camera_of_frame[b] of dev_cameras (16-byte aligned device copy of a table of
 * vti_checker_pack_cameras); the argument list, the checks and their order are vti_measure_cameras', native 0 or 1.  The kernels
 * compare dev_camera_of_frame[b] with [0, n_cams) BEFORE they form a table address: a frame whose index is outside reports
 * VTI_MEASURE_BAD_CAMERA, NaN averages, zero counts, and flags 0 / rank -1 / NaN in the per-slot rows of its instances; the other
 * frames are unaffected.  The table's contents are trusted, as there. */
VTI_CHECKER_RIG_API int32_t vti_measure_checker_cameras(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams,
                                                        const int32_t* dev_camera_of_frame, const uint8_t* dev_masks, int32_t native,
                                                        const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                                                        const int32_t* dev_offsets, int32_t B, int32_t max_det, int32_t capacity,
                                                        int32_t H0, int32_t W0, void* dev_scratch, size_t scratch_bytes,
                                                        double* frame_f64, int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32,
                                                        void* stream);
/* vti_measure_checker_cameras with H0, W0 of frame b from the frame table (vti_measure_frames' argument list): frame b's results are
 * bit-identical to those of vti_measure_checker_cameras called with H0[b], W0[b] on the same inputs.  Letterbox bit masks only:
 * native = 1 is VTI_ERR_UNSUPPORTED (the ragged rows are the next call's).  dev_scratch: >= vti_measure_scratch_bytes(ctx, B,
 * capacity, largest W0 of the table); the envelope rows are pitched by that W0 and the columns past a frame's own W0 are neither
 * written nor read. */
VTI_CHECKER_RIG_API int32_t vti_measure_checker_frames(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams,
                                                       const int32_t* dev_camera_of_frame, const uint8_t* dev_masks, int32_t native,
                                                       const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                                                       const int32_t* dev_offsets, const void* host_table, const void* dev_table,
                                                       int32_t B, int32_t max_det, int32_t capacity, void* dev_scratch,
                                                       size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64,
                                                       int32_t* stitch_i32, void* stream);
/* The same from the ragged frame-size rows of vti_masks_native_frames (vti_measure_frames_native's argument list: dev_mask_bases i64
 * [B + 1], capacity_bytes).  Frame b's results are bit-identical to those of vti_measure_checker_cameras with native = 1 at H0[b],
 * W0[b] on that frame's rows.  LIVENESS: instance i of frame b is live when i < counts[b], its slot index dev_offsets[b] + i is below
 * `capacity` and its rows end at or before capacity_bytes.  An instance that is not live is what the one-size call makes of a slot at
 * or past `capacity`: an empty mask that STILL HAS ITS BOX -- with drop_empty = 0 a fabric instance joins the union with its filled
 * rectangle and a stitch is measured at the centre of its int box; with drop_empty = 1 it does not exist -- and its per-slot rows
 * are not written. */
VTI_CHECKER_RIG_API int32_t vti_measure_checker_frames_native(vti_ctx* ctx, const void* dev_cameras, int32_t n_cams,
                                                              const int32_t* dev_camera_of_frame, const uint8_t* dev_masks,
                                                              const int64_t* dev_mask_bases, int64_t capacity_bytes,
                                                              const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                                                              const int32_t* dev_offsets, const void* host_table,
                                                              const void* dev_table, int32_t B, int32_t max_det, int32_t capacity,
                                                              void* dev_scratch, size_t scratch_bytes, double* frame_f64,
                                                              int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32,
                                                              void* stream);
/* vti_annotate_checker with the settings of frame b from row dev_camera_of_frame[b] of a checker table (NULL: row 0 for every frame)
 * in place of the struct, at the position vti_annotate has them; one frame size, native 0 or 1; the checks are vti_annotate's.  A
 * frame whose camera index is outside [0, n_cams), or whose status is none of OK, NO_FABRIC, NO_STITCHES, is copied as it is. */
VTI_CHECKER_RIG_API int32_t vti_annotate_checker_cameras(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0,
                                                         const void* dev_cameras, int32_t n_cams, const int32_t* dev_camera_of_frame,
                                                         const uint8_t* dev_masks, int32_t native, const float* dev_dets,
                                                         const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                                                         int32_t max_det, int32_t capacity, const int32_t* frame_i32,
                                                         const double* stitch_f64, const int32_t* stitch_i32,
                                                         const int32_t* host_select, const int32_t* dev_select, int32_t n_sel,
                                                         int32_t max_points, uint8_t* dev_out, int32_t* dev_status, void* dev_scratch,
                                                         size_t scratch_bytes, void* stream);
/* The checker's pictures of frames of differing sizes (vti_annotate_frames' argument list and checks: the in table pair, the out table
 * pair whose row k must have the size of frame host_select[k], the selection given twice).  Picture k is byte for byte what
 * vti_annotate_checker_cameras writes for that frame at its size; the gaps between the pictures, the bytes past the last one and
 * dev_frames are never written.  Letterbox bit masks only: native = 1 is VTI_ERR_UNSUPPORTED (the ragged rows:
 * vti_annotate_checker_frames_native); a selected frame above 8192 in either dimension is VTI_ERR_ARG naming it.  dev_scratch: >= vti_annotate_frames_scratch_bytes(ctx, host_out_table, max_det, max_points). */
VTI_CHECKER_RIG_API int32_t vti_annotate_checker_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table,
                                                        const void* dev_table, int32_t B, const void* dev_cameras, int32_t n_cams,
                                                        const int32_t* dev_camera_of_frame, const uint8_t* dev_masks, int32_t native,
                                                        const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                                                        const int32_t* dev_offsets, int32_t max_det, int32_t capacity,
                                                        const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                                                        const int32_t* host_select, const int32_t* dev_select, int32_t n_sel,
                                                        int32_t max_points, const void* host_out_table, const void* dev_out_table,
                                                        uint8_t* dev_out, int32_t* dev_status, void* dev_scratch, size_t scratch_bytes,
                                                        void* stream);

/* ---- the model-check viewer's picture on device (Utils/check_model.py:155-256, annotate_result) ------------------------------------ */
/* The frames dev_select[k] of the batch as the viewer shows them, byte for byte the package's overlay.py (render): per instance in
 * detection order the mask's outer contours (thickness 2), the int-truncated box (thickness 2) and, with dev_plates, a filled label
 * plate, all in the class colour palette[cls % n_colours]; then cv2.addWeighted(tinted frame, alpha, that picture, beta, 0), the
 * tinted frame being the frame with every pixel in the colour of the LAST instance whose mask covers it.  The blend is OpenCV 4's
 * v_fma form: fma(a, alpha, b * beta) in float32, rounded half to even, saturated.
 * mode: VTI_OVERLAY_DRAW writes the drawn picture, VTI_OVERLAY_BLEND blends the tinted frame with the caller's picture dev_annotated
 * (u8 [n_sel,H0,W0,3]; e.g. DRAW's output with the label text put on it by the host), VTI_OVERLAY_BOTH is byte for byte BLEND applied
 * to DRAW's output, without the intermediate.  dev_annotated: non-NULL iff mode is BLEND.
 * dev_frames, dev_masks, native, dev_dets, dev_xyxy, dev_counts, dev_offsets, max_det, capacity, host_select / dev_select and n_sel are
 * exactly what vti_annotate takes (1 <= H0, W0 <= 8192); an instance past the capacity has no mask and no plate, its box is drawn.
 * dev_plates: i32 [capacity,4] (xa, ya, xb, yb) per mask slot, 16-byte aligned, or NULL: every in-frame pixel with xa <= x <= xb and
 * ya <= y <= yb; a row with xb < xa or yb < ya draws nothing.  host_palette: n_colours (1..16) BGR triplets in host memory, read
 * during the call.  alpha, beta: finite.  max_points: room for the contour vertices of one frame.
 * dev_out u8 [n_sel,H0,W0,3]: every byte is written and nothing else is; dev_frames and dev_annotated are never written.  In BLEND
 * dev_out may be the very buffer dev_annotated points to (the operation is per pixel); nothing else may overlap.  dev_status i32
 * [n_sel]: 0, or VTI_OVERLAY_OUTLINE_SKIPPED when the frame's contours needed more than max_points vertices (or the tracer reached a
 * loop bound): none of that frame's contours is then drawn, everything else stands.  All launches go on `stream`, ordered by kernel
 * boundaries only; no host synchronisation, nothing the caller must clear.  dev_scratch: >= vti_overlay_scratch_bytes(), 256-byte
 * aligned.  Every argument check (VTI_ERR_ARG) runs before the first HIP call.  No weights are needed.
 * Frames of differing sizes (a frame table): vti_overlay_frames below.  Not covered: text on the device (the label strings stay with
 * the host: overlay.py label_items / plates / put_labels). */
enum { VTI_OVERLAY_DRAW = 1, VTI_OVERLAY_BLEND = 2, VTI_OVERLAY_BOTH = 3 };
enum { VTI_OVERLAY_OUTLINE_SKIPPED = 1 };
/* Host only: bytes of device scratch vti_overlay needs (0 on a bad argument); it grows with n_sel and with max_points. */
int64_t vti_overlay_scratch_bytes(const vti_ctx* ctx, int32_t n_sel, int32_t max_det, int32_t H0, int32_t W0, int32_t max_points);
int32_t vti_overlay(vti_ctx* ctx, const uint8_t* dev_frames, int32_t B, int32_t H0, int32_t W0, const uint8_t* dev_masks,
                    int32_t native, const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts,
                    const int32_t* dev_offsets, int32_t max_det, int32_t capacity, const int32_t* dev_plates,
                    const uint8_t* host_palette, int32_t n_colours, float alpha, float beta, const int32_t* host_select,
                    const int32_t* dev_select, int32_t n_sel, int32_t mode, const uint8_t* dev_annotated, int32_t max_points,
                    uint8_t* dev_out, int32_t* dev_status, void* dev_scratch, size_t scratch_bytes, void* stream);
/* vti_overlay for a batch whose frames differ in size.  dev_frames / host_table / dev_table: the flat frame buffer and the frame table
 * of vti_predict_frames (frame b: u8 [H0[b], W0[b], 3] BGR at byte_offset[b]); dets, xyxy, counts, offsets, max_det: what it wrote.
 * The OUTPUT is described by a second frame table, the out table, exactly as vti_annotate_frames' is: n_sel rows packed with
 * vti_pack_frames for the same canvas, row k with the H0, W0 of input row select[k] (otherwise VTI_ERR_ARG, and vti_last_error names
 * k); its byte offsets place picture k in dev_out, and in dev_annotated (BLEND: a flat buffer laid out by the same out table,
 * typically DRAW's dev_out with the host's text on it; dev_out may be that very buffer).  Every byte of each picture is written and
 * no other: not the gaps between pictures, not the bytes past the last one; dev_frames and dev_annotated are never written.
 * Masks, native = 0: the letterbox bit masks [capacity, H, W/8] as vti_overlay takes them; dev_mask_bases must be NULL.
 * Masks, native = 1: the ragged frame-size rows of vti_masks_native_frames / vti_predict_frames_native with their dev_mask_bases (i64
 * [B + 1], 8-byte aligned) and capacity_bytes: slot i of frame b is H0[b] rows of 8 * ceil(W0[b] / 64) bytes at byte bases[b] + i *
 * slot_bytes[b]; it is live iff it ends at or before capacity_bytes and its slot index offsets[b] + i is below `capacity`.  A slot that
 * is not live is "no mask": no tint and no contour; the box is drawn, and the plate while the slot index is below `capacity`.
 * dev_plates stays i32 [capacity,4] per slot index.  capacity_bytes >= 0 in either form.
 * Picture k and dev_status[k] are byte for byte what vti_overlay writes for that frame when called with H0[b], W0[b] on the same inputs
 * (native: that frame's slots as a uniform [n, H0, row_bytes] buffer), in each of DRAW, BLEND and BOTH; VTI_OVERLAY_OUTLINE_SKIPPED,
 * duplicates and any order of the selection are vti_overlay's.  A SELECTED frame above 8192 in either dimension is VTI_ERR_ARG naming
 * the frame.  dev_frames, dev_out and dev_annotated 16-byte aligned.  Every argument check -- both tables revalidated row by row, the
 * selection, the alignments and a short scratch included -- runs before the first HIP call; the device copies (tables, selection,
 * bases) are trusted as the other *_frames calls trust theirs.  The scratch regions are pitched by the largest selected frame; what
 * lies in a region beyond a frame's own extent is never read.  Up to three launches on `stream` as vti_overlay's, or four when a DRAW
 * or BOTH selection holds both frames whose bitmap fits the tracer's LDS image (H0 * ceil(W0 / 64) * 8 <= 156 KiB) and frames whose
 * bitmap does not: the contour kernel then runs in both forms, each on its own frames.  No host synchronisation, nothing to clear.
 * Host only: scratch bytes for the pictures the out table describes (0 on a bad argument) = vti_overlay_scratch_bytes(n_sel, max_det,
 * largest H0, largest W0 of its rows, max_points). */
int64_t vti_overlay_frames_scratch_bytes(const vti_ctx* ctx, const void* host_out_table, int32_t max_det, int32_t max_points);
int32_t vti_overlay_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t B,
                           const uint8_t* dev_masks, int32_t native, const int64_t* dev_mask_bases, int64_t capacity_bytes,
                           const float* dev_dets, const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                           int32_t max_det, int32_t capacity, const int32_t* dev_plates, const uint8_t* host_palette,
                           int32_t n_colours, float alpha, float beta, const int32_t* host_select, const int32_t* dev_select,
                           int32_t n_sel, int32_t mode, const uint8_t* dev_annotated, int32_t max_points, const void* host_out_table,
                           const void* dev_out_table, uint8_t* dev_out, int32_t* dev_status, void* dev_scratch, size_t scratch_bytes,
                           void* stream);

/* ---- the saved JPEG on device (cv2.imwrite(save_path, annotated): main.py:314, measurement.py:536) -------------------------------- */
/* n frames u8 [n,H0,W0,3] (BGR as cv2's frames are; rgb = 1: RGB) -> n JPEG files, byte for byte the package's jpeg.py: libjpeg's
 * baseline file at `quality` (jpeg_set_quality, force_baseline), 8 bit, YCbCr 4:2:0, one interleaved scan, the Annex K quantisation
 * and Huffman tables, no restart interval; SOI, APP0 (JFIF 1.01, units 0, density 1 x 1), DQT 0, DQT 1, SOF0, DHT DC0, AC0, DC1, AC1,
 * SOS, data, EOI.  Integer arithmetic only (jccolor.c, h2v2_downsample with its 1, 2 bias, jfdctint.c, jcdctmgr.c's division,
 * jchuff.c); partial MCUs are completed by edge replication and by libjpeg's dummy blocks.
 * dev_frames: any byte address (vti_annotate's dev_out feeds it directly, so does a raw batch); never written.  1 <= n, 1 <= H0,
 * W0 <= 8192, n * ceil(H0/16) * ceil(W0/16) <= 2^28, 1 <= quality <= 100, rgb 0 or 1, max_bytes >= 0.
 * dev_byte_offsets i64 [n+1] always receives the exclusive scan of the n file sizes, exact whatever max_bytes is; dev_out receives
 * file k at offsets[k] .. offsets[k+1], back to back and unpadded, only when offsets[n] <= max_bytes (otherwise nothing is written
 * there: call again with a larger buffer; dev_out may be NULL when max_bytes is 0).  Bytes of dev_out at and beyond offsets[n] are
 * never written.  dev_scratch: >= vti_encode_jpeg_scratch_bytes(), 256-byte aligned.  Every argument check (VTI_ERR_ARG, a short
 * scratch included) runs before the first HIP call; ctx, device and weights rules as vti_mask_polygons (no weights needed).
 * Nine launches on `stream` (blocks, bit lengths, bit scan, zero, bits, 0xFF count, chunk scan, offsets, write), no memset, no host
 * synchronisation.  Positions in the bit stream are 64-bit.
 * Host only: device scratch bytes for n frames of H0 x W0 (0 on a bad argument); a function of these three only.  With M = ceil(H0/16)
 * * ceil(W0/16) MCUs per frame and S = ceil(6 * M * 1658 / 8) bytes, the longest unstuffed scan (1658 bits per block: DC 9 + 11, 63
 * AC coefficients of 16 + 10), rounded up to 4096-byte chunks: 1024 + 16 n + n * (768 M coefficients + 48 M bit positions + S + S /
 * 1024), each part rounded up to 256.  960 x 1280: 9.9 MB per frame, 633 MB for 64. */
int64_t vti_encode_jpeg_scratch_bytes(const vti_ctx* ctx, int32_t n, int32_t H0, int32_t W0);
/* Host only: an upper bound of dev_byte_offsets[n] for any content and quality (0 on a bad argument): n * (625 + 2 S). */
int64_t vti_encode_jpeg_max_bytes(int32_t n, int32_t H0, int32_t W0);
int32_t vti_encode_jpeg(vti_ctx* ctx, const uint8_t* dev_frames, int32_t n, int32_t H0, int32_t W0, int32_t rgb, int32_t quality,
                        void* dev_scratch, size_t scratch_bytes, int64_t* dev_byte_offsets, uint8_t* dev_out, int64_t max_bytes,
                        void* stream);
/* vti_encode_jpeg for n frames of differing sizes: frame k is u8 [H0[k], W0[k], 3] at byte_offset[k] of dev_frames (16-byte aligned
 * offsets: a frame table's buffer, e.g. vti_annotate_frames' dev_out with its out table, or vti_decode_jpeg's layout 0).  File k is
 * byte for byte vti_encode_jpeg(n = 1, H0[k], W0[k]) of that frame -- its SOF0 carries its own height and width -- and the files lie
 * back to back and unpadded at offsets[k] .. offsets[k+1]; dev_byte_offsets i64 [n+1] is always exact, dev_out is written only when
 * offsets[n] <= max_bytes.  Per frame 1 <= H0, W0 <= 8192, and at most 2^28 MCUs in the batch.  Every argument check -- the table
 * revalidated for this ctx's canvas and exactly n frames included -- runs before the first HIP call.  Ten launches on `stream`:
 * vti_encode_jpeg's nine behind a prefix launch that builds, from the device table into the scratch, the exclusive scans of the frames'
 * MCU and stream-chunk counts (blocks: 6 per MCU); the kernels find the frame of an MCU, block or chunk by binary search over those
 * n + 1 entries, which ends inside [0, n) whatever they hold.  DC prediction restarts at each frame's first block.
 * Host only: the scratch is laid out per frame, not pitched by the largest one: 1024 + 2 * 8 (n + 1) for the prefixes + 16 n + 768 M +
 * 48 M + 4096 C + 4 C, each part rounded up to 256, with M and C the MCUs and 4096-byte chunks of the whole batch -- at most the sum of
 * vti_encode_jpeg_scratch_bytes(ctx, 1, H0[k], W0[k]) plus the prefixes.  0 on a bad argument. */
int64_t vti_encode_jpeg_frames_scratch_bytes(const vti_ctx* ctx, const void* host_table);
/* Host only: the sum of vti_encode_jpeg_max_bytes(1, H0[k], W0[k]) over the table's frames (0 on a bad argument). */
int64_t vti_encode_jpeg_frames_max_bytes(const void* host_table);
int32_t vti_encode_jpeg_frames(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table, int32_t n,
                               int32_t rgb, int32_t quality, void* dev_scratch, size_t scratch_bytes, int64_t* dev_byte_offsets,
                               uint8_t* dev_out, int64_t max_bytes, void* stream);

/* ---- the text of the annotated pictures on device (cv2.putText: measurement.py:282, 333, 366-368, 501-504; main.py:302-309) ------ */
/* cv2.putText with the default line type writes ONE solid colour on a set of pixels that does not depend on the picture under it.  The
 * strings are the host's (they hold the smoothed values), so the host rasterises each string once into a 1-bit STAMP, the stamps
 * cross to the device, and vti_stamp paints them onto the pictures vti_annotate, vti_annotate_frames or vti_annotate_checker drew,
 * in place, before vti_encode_jpeg reads them.  The library holds no font: any rasteriser serves (the package's annotate.text_stamps
 * uses cv2.putText where OpenCV is installed), and the caller's own lines go the same way.
 * A stamp is a rectangle x, y, w, h of picture `picture`, a BGR colour and h rows of `pitch` 32-bit words in the bit buffer, the
 * first at word_offset: bit j of word q of row r is pixel (x + 32 q + j, y + r); it is painted when set.  Bits at columns >= w are
 * ignored, so a row may be padded with anything.  Applying a stamp sets every painted pixel to the colour; the stamps of a picture
 * are applied in array order, a later one overwrites an earlier one: byte for byte the package's annotate.stamp.
 * LIMITS: 1 <= n_pictures <= VTI_STAMP_MAX_PICTURES, pictures of 1 <= H0, W0 <= 8192 (vti_annotate's), at most
 * VTI_STAMP_MAX_PER_PICTURE stamps per picture and VTI_STAMP_MAX_TOTAL in a table (0 is allowed: nothing is painted), pitch <=
 * VTI_STAMP_MAX_PITCH words, 0 <= n_words <= 2^40. */
enum { VTI_STAMP_MAX_PICTURES = 4096, VTI_STAMP_MAX_PER_PICTURE = 65536, VTI_STAMP_MAX_TOTAL = 1 << 24, VTI_STAMP_MAX_PITCH = 65536 };
/* Marks the four entry points of the stamp calls; libvti.so exports them as it does every other. */
#define VTI_STAMP_API
typedef struct vti_stamp_desc {
    int32_t picture;            /* index of the picture, non-decreasing along the array */
    int32_t x, y, w, h;         /* the rectangle: w, h >= 1, inside the picture */
    int32_t pitch;              /* 32-bit words per row, >= ceil(w / 32) */
    uint8_t bgr[4];             /* B, G, R; the fourth byte is ignored */
    int32_t reserved;
    int64_t word_offset;        /* of row 0 in the bit buffer; word_offset + h * pitch <= n_words */
} vti_stamp_desc;
/* Host only: bytes of a stamp table (0 when a count is outside the limits): a header, a range of stamps per picture, a record per
 * stamp; the format is private to the library build. */
VTI_STAMP_API int64_t vti_stamp_table_bytes(int32_t n_pictures, int32_t n_stamps);
/* Host only: validates the n_stamps stamps against the pictures' sizes H0[k], W0[k] and the length n_words of the bit buffer and writes
 * the table (nbytes >= vti_stamp_table_bytes()).  Refused with VTI_ERR_ARG, vti_last_error naming the stamp's index (ctx only receives
 * the text and may be NULL): picture outside [0, n_pictures) or smaller than the previous stamp's; w or h < 1; a rectangle that is
 * not inside its picture; pitch < ceil(w / 32) or above the limit; word_offset < 0 or word_offset + h * pitch > n_words; more stamps
 * in one picture or in the table than the limits allow.  stamps may be NULL when n_stamps is 0.  Equal inputs give equal bytes. */
VTI_STAMP_API int32_t vti_pack_stamps(vti_ctx* ctx, const int32_t* H0, const int32_t* W0, int32_t n_pictures,
                                      const vti_stamp_desc* stamps, int32_t n_stamps, int64_t n_words, void* host_table, size_t nbytes);
/* Paints the table's stamps onto dev_pictures u8 [n,H0,W0,3] in place.  host_table: the whole table vti_pack_stamps wrote for these n
 * pictures of H0 x W0 and this n_words; dev_table: its device copy (16-byte aligned); dev_bits: u32 [n_words] on the device (4-byte
 * aligned; may be NULL when the table has no stamp).  A byte that no set bit covers keeps its value and is not even read; a picture
 * without stamps costs no picture traffic, and a table without stamps launches nothing.  Every argument check -- the host table
 * revalidated header, ranges and record by record, the sizes compared with H0, W0 (VTI_ERR_ARG naming the stamp or the picture) --
 * runs before the first HIP call; ctx, device and weights rules as vti_encode_jpeg (no weights needed).  The device copies are trusted
 * to hold the same bytes, as a frame table's copy is; the kernel still clamps every rectangle to its picture, every word address to
 * [0, n_words) and every record index to the table, so a device table that differs may paint wrong pixels of the pictures but
 * touches no byte outside them and reads nothing outside the bit buffer and the table.  One launch on `stream` (a workgroup per
 * 8192 pixels of a picture; one that no stamp of its picture reaches leaves after reading the records), no scratch, no memset, no
 * atomics on the pictures, no host synchronisation: annotate -> stamp -> encode may be captured in one graph. */
VTI_STAMP_API int32_t vti_stamp(vti_ctx* ctx, uint8_t* dev_pictures, int32_t n, int32_t H0, int32_t W0, const void* host_table,
                                const void* dev_table, const uint32_t* dev_bits, int64_t n_words, void* stream);
/* vti_stamp for pictures of differing sizes: dev_buf and the frame table pair are what vti_annotate_frames returned (its dev_out and
 * out table; any flat buffer with its frame table serves), picture k being frame k.  Picture k comes out byte for byte as vti_stamp
 * gives it at that picture's size; the gaps between the pictures and the bytes past the last one are never written.  The frame table
 * is checked as by every *_frames call, and the sizes in the stamp table must equal its rows (VTI_ERR_ARG naming k otherwise); a
 * picture above 8192 in either dimension is refused.  dev_buf 16-byte aligned.  Everything else is vti_stamp's. */
VTI_STAMP_API int32_t vti_stamp_frames(vti_ctx* ctx, uint8_t* dev_buf, const void* host_frame_table, const void* dev_frame_table,
                                       int32_t n, const void* host_table, const void* dev_table, const uint32_t* dev_bits,
                                       int64_t n_words, void* stream);

/* ---- NMS settings per frame, and Ultralytics' `classes` filter (config.py:69-73 per station; predict(classes=...)) -------------- */
/* conf, iou, max_det, agnostic and a class set per FRAME in place of per call: the settings live in a table of rows in device
 * memory and an i32 device array names each frame's row, as the camera tables of the measure calls do.  One row used for every
 * frame is predict(classes=[...]); one row per camera serves a batch that mixes stations with different thresholds.  Frame b comes
 * out bit for bit as the table-free call gives it with its row's settings (and max_det = min(row.max_det, the call's max_det)).
 * The class set is applied where Ultralytics' non_max_suppression applies it: to the class of each anchor's first maximal score,
 * after the confidence test and BEFORE the 30000 cut, the greedy pass and max_det.  An anchor whose best class is outside the set is
 * dropped even when another, allowed class of it scores above conf (the single-label rule), an excluded box never suppresses a wanted
 * one under agnostic NMS and never uses one of the max_det places -- which a filter on the returned rows cannot undo.
 * LIMITS: 1 <= n_rows <= VTI_NMS_TABLE_MAX_ROWS; a class set needs a model of at most VTI_NMS_TABLE_MAX_CLASSES classes (the width
 * of a row's bit mask). */
enum { VTI_NMS_TABLE_MAX_ROWS = 65536, VTI_NMS_TABLE_MAX_CLASSES = 1024 };
/* Marks the three entry points of the NMS table; libvti.so exports them as it does every other. */
#define VTI_NMS_TABLE_API
typedef struct {
    float conf;              /* 0 <= conf <= 1, finite */
    int32_t max_det;         /* >= 1; the effective limit is min(this, the call's max_det) */
    double iou;              /* 0 <= iou <= 1, finite */
    int32_t agnostic;        /* 0 or 1 */
    int32_t n_classes;       /* 0: every class; else classes[0 .. n_classes) */
    const int32_t* classes;  /* host; each in [0, nc); duplicates allowed */
} vti_nms_params;
/* Host only: bytes of a table of n_rows rows (0 when n_rows < 1 or above VTI_NMS_TABLE_MAX_ROWS): a header and a row per entry. */
VTI_NMS_TABLE_API int64_t vti_nms_table_bytes(int32_t n_rows);
/* Host only: validates params[0 .. n_rows) against the ctx's class count nc and writes the table (nbytes >= the size above).
 * VTI_ERR_ARG, vti_last_error naming the first failing row and its field: conf or iou outside [0, 1] or not finite, max_det < 1,
 * agnostic neither 0 nor 1, n_classes < 0, n_classes > 0 with a NULL list, a class outside [0, nc).  A row with a class set on a
 * model of more than VTI_NMS_TABLE_MAX_CLASSES classes is VTI_ERR_UNSUPPORTED.  A set that names every class packs as no set at all.
 * Equal inputs give equal bytes; the format is private to the library build.  ctx is required (it gives nc). */
VTI_NMS_TABLE_API int32_t vti_pack_nms_table(vti_ctx* ctx, const vti_nms_params* params, int32_t n_rows,
                                             void* host_table, size_t nbytes);
/* Installs the table: until it is cleared or replaced, EVERY NMS of the ctx -- vti_nms, vti_nms_scored, vti_predict,
 * vti_predict_frames, vti_predict_frames_native -- takes frame b's settings from row dev_row_of_frame[b] (NULL: row 0 for every
 * frame); the calls' own conf, iou and agnostic are ignored, their max_det stays the row stride of dev_dets and the upper bound of
 * every row's limit.  host_table: the bytes vti_pack_nms_table wrote for THIS ctx's nc and these n_rows (the ctx keeps a copy and
 * revalidates it here: VTI_ERR_ARG naming the row otherwise); NULL clears the table, the other arguments are then ignored.
 * dev_table: its device copy (16-byte aligned, trusted to hold the same bytes); dev_row_of_frame: i32, at least max_batch entries,
 * 4-byte aligned.  Both stay caller-owned and must live until the table is cleared or replaced.  The kernels compare
 * dev_row_of_frame[b] with [0, n_rows) BEFORE they form a table address: a frame whose index is outside gets counts[b] = 0 and
 * all-zero rows; the other frames are unaffected.  Host only: every check runs before any HIP call, and the setter makes none. */
VTI_NMS_TABLE_API int32_t vti_set_nms_table(vti_ctx* ctx, const void* host_table, const void* dev_table,
                                            int32_t n_rows, const int32_t* dev_row_of_frame);

/* ---- predict on a window of each frame: results in frame pixels ------------------------------------------------------------------ */
/* The reference measures inside a region of interest (config.py roi, measurement.py:249-272) and drops every detection outside it,
 * yet letterboxes the whole frame.  These calls run the pipeline on a WINDOW (x0, y0, w, h) of each frame, read in place from the
 * frame buffer of vti_pack_frames' layout, and return everything in FRAME pixels.  They are defined by the calls on contiguous crops:
 * with crop_b = frame_b[y0:y0+h, x0:x0+w], T_crop the frame table of the crops and T_full that of the full frames on the same canvas,
 *   canvas, pred, proto, dets, counts   == vti_letterbox_frames / vti_predict_frames_native on (crops, T_crop), byte for byte;
 *   xyxy                                 == vti_scale_boxes_frames(T_crop) + (float)(x0, y0, x0, y0), one f32 add per coordinate
 *                                           (rows at or past counts[b] stay zero);
 *   offsets, mask_bases, slot layout, liveness by capacity_bytes == vti_masks_native_frames on T_full; bit (y, x) of a live slot is
 *                                           bit (y - y0, x - x0) of the crop's mask inside the window and 0 elsewhere (the crop to the
 *                                           box uses the window-px box, not the shifted one); live slots are written completely, no
 *                                           byte after the last live slot is touched.
 * With the window (0, 0, W0, H0) for every frame every output byte equals vti_predict_frames_native on T_full.  So every consumer of
 * native = 1 rows or dev_mask_bases (vti_measure_frames_native, vti_annotate_frames_native, vti_mask_polygons_frames, vti_overlay_frames)
 * takes the result unchanged, together with T_full.
 * Marks the entry points of the window family; libvti.so exports them as it does every other. */
#define VTI_WINDOWS_API
/* Host only: bytes of a window table of B frames (0 when B < 1): a header and one row per frame. */
VTI_WINDOWS_API int64_t vti_window_table_bytes(int32_t B);
/* Host only: vti_pack_frames' checks of the B frames (H0, W0, byte_offset, total_bytes, the canvas H x W), then of each window
 * windows[b] = {x0, y0, w, h}: x0, y0 >= 0, w, h >= 1, x0 + w <= W0[b], y0 + h <= H0[b], and the window letterboxed onto the canvas
 * not below 1 px.  VTI_ERR_ARG with the index of the first failing frame in vti_last_error.  Writes the table (nbytes >=
 * vti_window_table_bytes(B)); equal inputs give equal bytes; the format is private to the library build.  ctx may be NULL (it
 * receives the error text); with a ctx, B above its max_batch is refused here, as every *_windows call would refuse the table. */
VTI_WINDOWS_API int32_t vti_pack_windows(vti_ctx* ctx, int32_t H, int32_t W, const int32_t* H0, const int32_t* W0,
                                         const int64_t* byte_offset, const int32_t* windows, int32_t B, int64_t total_bytes,
                                         void* host_table, size_t nbytes);
/* Host only: what row b holds.  out_i32[12] = {h, w, new_h, new_w, top, left, offset lo, offset hi, x0, y0, H0, W0}: the first eight
 * and out_f64[5] (may be NULL) are what vti_frame_table_info reports for the contiguous crop, with `offset` the byte of the window's
 * first pixel in the frame buffer -- for a whole-frame window exactly the frame's own row.  b = -1: the header, as
 * vti_frame_table_info gives it (max_H0, max_W0 of the full frames), the last four zero. */
VTI_WINDOWS_API int32_t vti_window_table_info(const void* host_table, int32_t b, int32_t out_i32[12], double out_f64[5]);
/* The *_windows calls take the table twice, as every *_frames call does: host_table is revalidated row by row before the first HIP
 * call (VTI_ERR_ARG naming the frame), dev_table is its device copy (16-byte aligned, trusted to hold the same bytes).
 * dev_frames: the frame buffer the table was packed for (16-byte aligned); never written; nothing outside a frame is read, and
 * bytes right of a window inside its frame only where their resize weight is 0.  dev_input u8 [B,H,W,3], 4-byte aligned. */
VTI_WINDOWS_API int32_t vti_letterbox_windows(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table,
                                              int32_t B, uint8_t* dev_input, void* stream);
/* dev_xyxy f32 [B, max_det, 4] (16-byte aligned): the boxes in FRAME px. */
VTI_WINDOWS_API int32_t vti_scale_boxes_windows(vti_ctx* ctx, const float* dev_dets, const int32_t* dev_counts, const void* host_table,
                                                const void* dev_table, int32_t B, int32_t max_det, float* dev_xyxy, void* stream);
/* Host only: vti_mask_native_frames_bytes of the full frames of the table (0 on a bad argument). */
VTI_WINDOWS_API int64_t vti_mask_native_windows_bytes(const vti_ctx* ctx, const void* host_table, int32_t max_det);
/* vti_masks_native_frames' arguments without dev_xyxy: the stage computes each box in window px from dev_dets with scale_boxes' own
 * expression.  packing must be VTI_PACK_BITS. */
VTI_WINDOWS_API int32_t vti_masks_native_windows(vti_ctx* ctx, const float* dev_dets, const int32_t* dev_counts, const void* dev_proto,
                                                 const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t mode,
                                                 int32_t packing, uint8_t* dev_masks, int64_t capacity_bytes, int32_t* dev_offsets,
                                                 int64_t* dev_mask_bases, void* stream);
/* vti_predict_frames_native's arguments with the window table in place of the frame table: letterbox, scored forward, NMS (a set NMS
 * table applies), scale boxes, masks on one stream with no host synchronisation. */
VTI_WINDOWS_API int32_t vti_predict_windows(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table, const void* dev_table,
                                            int32_t B, int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic,
                                            int32_t mask_mode, int32_t packing, uint8_t* dev_input_scratch, float* dev_pred,
                                            void* dev_proto, float* dev_dets, int32_t* dev_counts, uint8_t* dev_masks,
                                            int64_t capacity_bytes, int32_t* dev_offsets, int64_t* dev_mask_bases, float* dev_xyxy,
                                            void* stream);

/* ---- pictures of frames of differing sizes from their frame-resolution masks ------------------------------------------------------ */
/* vti_annotate_frames and vti_annotate_checker_frames for the ragged frame-size rows of vti_masks_native_frames /
 * vti_predict_frames_native / vti_predict_windows, measured by vti_measure_frames_native (checker: vti_measure_checker_frames_native).
 * The arguments are those of the letterbox forms with two changes: there is no `native` argument, and dev_mask_bases (i64 [B + 1],
 * 8-byte aligned, required) and capacity_bytes (>= 0) follow dev_masks, as in vti_measure_frames_native.  Instance i of frame b is
 * H0[b] rows of ceil(W0[b] / 64) 64-bit words from byte dev_mask_bases[b] + i * slot_bytes[b] on.  `capacity` counts slot INDICES
 * (dev_offsets[b] + i), the rows of stitch_f64 / stitch_i32 the measurement wrote.
 * Picture k and dev_status[k] are byte for byte what vti_annotate(native = 1) (checker: vti_annotate_checker_cameras(native = 1))
 * writes for frame b = select[k] when called with H0[b], W0[b] on that frame's run of slots as a uniform [n, H0, row_bytes] buffer,
 * and `capacity` cuts the slot index as it does there.  A slot that does not end at or before capacity_bytes is what the
 * measurement of its family made of it.  vti_annotate_frames_native: all zeros in that buffer, its per-slot rows still read --
 * vti_measure_frames_native wrote them, for the same empty mask.  vti_annotate_checker_frames_native: not in that buffer at all, a
 * slot at or beyond the uniform call's capacity (an empty mask with its box, no per-slot row) -- vti_measure_checker_frames_native
 * counts it so and writes no row for it.  No byte of dev_masks at or beyond capacity_bytes is read; a base that is negative or no
 * multiple of 8 gives its frame no readable slot.
 * Everything else is vti_annotate_frames': the out table, every byte of each picture written and no other, the plain copy of a frame
 * with a bad camera, duplicates and any order of the selection, VTI_ANNOTATE_OUTLINE_SKIPPED, the 8192 limit on a SELECTED frame,
 * three or four launches on `stream`, no host synchronisation.  Every argument check runs before the first HIP call: those of
 * vti_annotate_frames as they stand; dev_mask_bases non-null and 8-byte aligned; capacity_bytes >= 0; dev_masks 8-byte aligned when
 * capacity_bytes > 0, and NULL only when capacity_bytes == 0.  The checker form's letterbox "resize tables" canvas check does not
 * apply (no letterbox mask is resized).  dev_scratch: >= vti_annotate_frames_scratch_bytes(ctx, host_out_table, max_det, max_points).
 * Marks the two entry points; libvti.so exports them as it does every other. */
#define VTI_ANNOTATE_NATIVE_API
VTI_ANNOTATE_NATIVE_API int32_t vti_annotate_frames_native(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table,
                                                           const void* dev_table, int32_t B, const void* dev_cameras, int32_t n_cams,
                                                           const int32_t* dev_camera_of_frame, const uint8_t* dev_masks,
                                                           const int64_t* dev_mask_bases, int64_t capacity_bytes, const float* dev_dets,
                                                           const float* dev_xyxy, const int32_t* dev_counts, const int32_t* dev_offsets,
                                                           int32_t max_det, int32_t capacity, const int32_t* frame_i32,
                                                           const double* stitch_f64, const int32_t* stitch_i32,
                                                           const int32_t* host_select, const int32_t* dev_select, int32_t n_sel,
                                                           int32_t max_points, const void* host_out_table, const void* dev_out_table,
                                                           uint8_t* dev_out, int32_t* dev_status, void* dev_scratch, size_t scratch_bytes,
                                                           void* stream);
/* dev_cameras: a table of vti_checker_pack_cameras; frame_i32, stitch_f64, stitch_i32: what vti_measure_checker_frames_native wrote. */
VTI_ANNOTATE_NATIVE_API int32_t vti_annotate_checker_frames_native(vti_ctx* ctx, const uint8_t* dev_frames, const void* host_table,
                                                                   const void* dev_table, int32_t B, const void* dev_cameras,
                                                                   int32_t n_cams, const int32_t* dev_camera_of_frame,
                                                                   const uint8_t* dev_masks, const int64_t* dev_mask_bases,
                                                                   int64_t capacity_bytes, const float* dev_dets, const float* dev_xyxy,
                                                                   const int32_t* dev_counts, const int32_t* dev_offsets, int32_t max_det,
                                                                   int32_t capacity, const int32_t* frame_i32, const double* stitch_f64,
                                                                   const int32_t* stitch_i32, const int32_t* host_select,
                                                                   const int32_t* dev_select, int32_t n_sel, int32_t max_points,
                                                                   const void* host_out_table, const void* dev_out_table,
                                                                   uint8_t* dev_out, int32_t* dev_status, void* dev_scratch,
                                                                   size_t scratch_bytes, void* stream);

/* ---- JPEG files -> frames on device (cap.read() of a motion-JPEG camera, cv2.imread, Ultralytics' file sources) ----------------- */
/* n files -> n frames u8 [H0,W0,3], byte for byte the package's jpeg.decode, which is pinned to libjpeg-turbo's output with its
 * defaults (JDCT_ISLOW, fancy upsampling): jdhuff.c, jidctint.c with the dequantisation inside, jdsample.c, jdcolor.c; integer
 * arithmetic only.  SUPPORTED: baseline sequential (SOF0), 8-bit samples, three components YCbCr, luma sampling 2x2 (4:2:0), 2x1
 * (4:2:2) or 1x1 (4:4:4) with 1x1 chroma, one interleaved scan, 8-bit DQT, the file's DHT tables or Annex K's when it has none
 * (motion-JPEG), any DRI restart interval, APPn / COM segments and 0xFF fill bytes skipped, 1 <= H0, W0 <= 8192, a scan of at most
 * 2^28 bytes.  Everything else (progressive, greyscale, four components, Adobe transform 0, other sampling factors, 12-bit
 * samples, 16-bit DQT, arithmetic coding, several scans) is refused by the host parser with VTI_ERR_UNSUPPORTED and a text that
 * names the reason; a malformed or truncated header is VTI_ERR_ARG.  There is no approximate decoding.
 * Host only: bytes of a descriptor table of n files (0 when n < 1 or n > 4096). */
int64_t vti_decode_jpeg_table_bytes(int32_t n);
/* Host only: parses and validates file k = host_files[host_file_offsets[k] .. host_file_offsets[k+1]) for k = 0 .. n-1 (offsets
 * ascending from >= 0); the first failing file's index and the reason are in vti_last_error (ctx only receives the text and may be
 * NULL).  Writes the descriptor table (nbytes >= vti_decode_jpeg_table_bytes(n); its format is private to the library build),
 * out_H0 / out_W0 [n] from the headers, the frames' places out_byte_offsets [n+1] in dev_out and *out_scratch_bytes.  layout 0:
 * the frames back to back, each at a multiple of 16 bytes, [n] = the buffer's size (a multiple of 16, at least 16): exactly the
 * rule of vti_pack_frames' frame buffer, so dev_out feeds vti_predict_frames directly.  layout 1: dense u8 [n,H0,W0,3]; all files
 * must have one size (VTI_ERR_ARG otherwise).  segment_bytes: the bytes of the scan one lane decodes at a time, a power of two from
 * 16 to 4096, or 0 for the library's default (256).  Equal inputs give equal bytes.  The table describes the files at these very
 * offsets of the buffer that is later copied to the device. */
int32_t vti_decode_jpeg_plan(vti_ctx* ctx, const uint8_t* host_files, const int64_t* host_file_offsets, int32_t n,
                             int32_t segment_bytes, int32_t layout, void* host_table, size_t nbytes, int32_t* out_H0,
                             int32_t* out_W0, int64_t* out_byte_offsets, int64_t* out_scratch_bytes);
/* dev_files: the device copy of the bytes the plan parsed (any byte address; never written).  host_table: the bytes the plan wrote;
 * dev_table: their device copy (16-byte aligned), trusted to hold the same bytes, as a frame table's copy is.  rgb 1: R, G, B as
 * PIL gives them; 0: B, G, R as cv2.imread / cap.read() do.  dev_out (>= out_byte_offsets[n] bytes, out_bytes its size): every
 * byte of each frame is written and no other (not the gaps of layout 0).  dev_info i32 [n,4] = {status: 0 or VTI_JPEG_CORRUPT,
 * segments, rounds of the entropy stage used, blocks decoded}.  A damaged scan (an invalid code, data that ends early, a missing or
 * misnumbered RSTn, bytes left over) terminates, stays inside its buffers and sets the file's status; its pixels are unspecified
 * but lie inside its own frame, and the other files of the batch are unaffected.  dev_scratch: >= *out_scratch_bytes, 256-byte
 * aligned.  Every argument check (VTI_ERR_ARG), the table revalidated row by row included, runs before the first HIP call; ctx,
 * device and weights rules as vti_encode_jpeg (no weights needed).  Five launches on `stream` (zero, entropy, DC, IDCT, colour), no
 * memset, no host synchronisation.  The entropy stage decodes the scan in segments of segment_bytes, one workgroup per file, with
 * the self-synchronising scheme (every lane starts from a guessed state and is re-run from its predecessor's exit state until no
 * state changes, at most as many rounds as there are segments), so it waits on no other workgroup and has no unbounded loop. */
enum { VTI_JPEG_CORRUPT = 1 };
int32_t vti_decode_jpeg(vti_ctx* ctx, const uint8_t* dev_files, const void* host_table, const void* dev_table, int32_t n, int32_t rgb,
                        uint8_t* dev_out, int64_t out_bytes, int32_t* dev_info, void* dev_scratch, size_t scratch_bytes, void* stream);

/* ---- raw camera frames -> frames on device (cap.read() of a V4L2 camera that delivers YUV; CSI cameras, hardware decoders) ------- */
/* With cap.set(cv2.CAP_PROP_CONVERT_RGB, 0) cap.read() returns the camera's raw buffer instead of cvtColor(COLOR_YUV2BGR_*) of it; this
 * call is that conversion on the device, byte for byte the package's rawframes.to_bgr, which restates OpenCV 4.x's color_yuv.simd.hpp
 * (BT.601, limited range, 20-bit fixed point):
 *   u' = U - 128, v' = V - 128;  ruv = 2^19 + 1673527 v';  guv = 2^19 - 852492 v' - 409993 u';  buv = 2^19 + 2116026 u'
 *   y' = max(0, Y - 16) * 1220542;  R = clamp((y' + ruv) >> 20), G = clamp((y' + guv) >> 20), B = clamp((y' + buv) >> 20)
 * (arithmetic shift, clamp to 0..255).  Chroma is replicated, never interpolated: one (U, V) serves a horizontal pixel pair in 4:2:2
 * and a 2 x 2 block in 4:2:0.  Frames are tightly packed (no line padding; the caller compacts padded rows):
 *   VTI_RAW_YUYV  2*H0*W0 bytes   per pixel pair Y0 U Y1 V                           COLOR_YUV2BGR_YUYV
 *   VTI_RAW_UYVY  2*H0*W0         U Y0 V Y1                                          COLOR_YUV2BGR_UYVY
 *   VTI_RAW_NV12  H0*W0*3/2       Y plane, then interleaved U V (H0/2 x W0/2 pairs)  COLOR_YUV2BGR_NV12
 *   VTI_RAW_NV21  H0*W0*3/2       Y plane, then interleaved V U                      COLOR_YUV2BGR_NV21
 *   VTI_RAW_I420  H0*W0*3/2       Y plane, U plane, V plane                          COLOR_YUV2BGR_I420
 *   VTI_RAW_YV12  H0*W0*3/2       Y plane, V plane, U plane                          COLOR_YUV2BGR_YV12
 * W0 even; H0 even too for the 4:2:0 formats; 2 <= H0, W0 <= 8192.  Every byte string of the right length is a frame. */
enum { VTI_RAW_YUYV = 0, VTI_RAW_UYVY, VTI_RAW_NV12, VTI_RAW_NV21, VTI_RAW_I420, VTI_RAW_YV12 };
/* Host only: bytes of one frame; 0 on a bad argument (unknown fmt, a size outside the rules above). */
int64_t vti_raw_frame_bytes(int32_t fmt, int32_t H0, int32_t W0);
/* B frames of one size and format, frame b at dev_raw + b * vti_raw_frame_bytes() -> dev_frames u8 [B,H0,W0,3]; rgb 0: B, G, R as
 * cap.read() gives them, 1: R, G, B.  dev_raw and dev_frames may be any byte address (accesses at multiples of their size are 8-
 * or 16-byte vector accesses, the others go byte by byte, both exact); dev_raw is never written, every byte of dev_frames is and no
 * other.  1 <= B <= 4096.  Every argument check (VTI_ERR_ARG) runs before the first HIP call; ctx, device and weights rules as
 * vti_decode_jpeg (no weights needed).  One launch on `stream`, no scratch, no memset, no host synchronisation. */
int32_t vti_convert_raw(vti_ctx* ctx, const uint8_t* dev_raw, int32_t fmt, int32_t B, int32_t H0, int32_t W0, int32_t rgb,
                        uint8_t* dev_frames, void* stream);
/* Frames that differ in size and / or format: the raw table.  Host only: bytes of a table of n frames (0 when n < 1 or n > 4096). */
int64_t vti_raw_table_bytes(int32_t n);
/* Host only: validates the n frames (the first failing index and the reason are in vti_last_error; ctx only receives the text and may
 * be NULL), places them back to back, each at a multiple of 16 bytes, and writes the table (nbytes >= vti_raw_table_bytes(n); its
 * format is private to the library build).  out_raw_offsets [n+1]: frame k's first byte in the raw buffer; [n] is the buffer's size. */
int32_t vti_pack_raw_frames(vti_ctx* ctx, const int32_t* H0, const int32_t* W0, const int32_t* fmt, int32_t n, void* host_raw_table,
                            size_t nbytes, int64_t* out_raw_offsets);
/* dev_raw (raw_bytes >= out_raw_offsets[n] bytes): the raw frames at the table's offsets; never written.  host_raw_table /
 * dev_raw_table: the bytes vti_pack_raw_frames wrote and their device copy (16-byte aligned, trusted to hold the same bytes).  The
 * OUTPUT places come from a frame table (vti_pack_frames) of the same n frames: frame b is written as u8 [H0[b],W0[b],3] at its
 * byte_offset[b], so (dev_out, frame table) feeds vti_predict_frames, vti_annotate_frames and vti_encode_jpeg_frames as it is.
 * Checked on the host before the first HIP call (VTI_ERR_ARG, vti_last_error names the row): the frame table as by every *_frames
 * call, every row of the raw table again (format, size, length, offsets ascending without overlap at multiples of 16, inside the
 * table's raw_bytes), row b of both tables having the same H0 x W0, raw_bytes, and out_bytes >= the frame table's total_bytes.
 * Every byte of each frame is written and no other: not the gaps between frames.  One launch on `stream`: a grid as large as the
 * biggest frame needs, times n; a workgroup past its own frame's extent leaves at once. */
int32_t vti_convert_raw_frames(vti_ctx* ctx, const uint8_t* dev_raw, int64_t raw_bytes, const void* host_raw_table,
                               const void* dev_raw_table, const void* host_frame_table, const void* dev_frame_table, int32_t n,
                               int32_t rgb, uint8_t* dev_out, int64_t out_bytes, void* stream);

/* ---- per-layer access for parity tests ------------------------------------------- */
/* Copies the activation written by conv `i` of the last vti_forward into dev_out as
 * f32 NCHW [B,c2,h_out,w_out] (test hook; not on the hot path). */
int32_t vti_debug_conv_output(vti_ctx* ctx, int32_t i, int32_t B, float* dev_out, void* stream);

/* Runs ONE convolution of the engine's conv family on caller tensors (kernel unit tests and
 * micro-benchmarks; synchronous, allocates its own packed weights -- not on the hot path).
 * dev_in: T NHWC [B,H,W,in_ld] (or u8 [B,H,W,3] when c1==3, the stem conv); host_w: f32 OIHW
 * (kind 2: IOHW) in HOST memory; dev_out: T (or f32 if out_f32) NHWC with row pitch out_ld.
 * tile_h/tile_w/waves_n/nrep = 0 lets the planner choose; iters > 1 times iters-1 launches with
 * HIP events into *ms_out; cfg_out[5] receives {tile_h, tile_w, waves_n, nrep, lds_bytes}. */
int32_t vti_debug_conv2d(int32_t dtype, const void* dev_in, int32_t B, int32_t H, int32_t W, int32_t in_ld,
                         int32_t in_coff, int32_t c1, const float* host_w, const float* host_b, int32_t c2,
                         int32_t k, int32_t s, int32_t kind, const void* dev_res, int32_t res_ld, int32_t res_coff,
                         void* dev_out, int32_t out_ld, int32_t out_coff, int32_t out_f32, int32_t swap_rb,
                         int32_t tile_h, int32_t tile_w, int32_t waves_n, int32_t nrep, int32_t iters,
                         float* ms_out, int32_t* cfg_out, void* stream);

/* ---- the forward pass's non-GEMM kernels, one at a time (kernel unit tests) --------- */
/* Marks the single-kernel and single-op test hooks; libvti.so exports them as it does every other. */
#define VTI_DEBUG_OPS_API
/* Like vti_debug_conv2d these take no context and no weights; unlike it they only enqueue their one launch on `stream`.  Every
 * refusal below is VTI_ERR_ARG with a message in vti_last_error(NULL), made on the host before anything is launched.  T is the
 * element of `dtype`: fp16 (2 bytes), fp32 or an h2 pair (4 bytes); a "vector" is 16 bytes: 8 fp16 elements, 4 of the others.
 *
 * vti_debug_sppf_pool: the SPPF's three chained MaxPool2d(5, 1, 2) of channels [in_coff, in_coff + C) of dev_in (T NHWC
 * [B,H,W,ld]) into channels [out_coff, out_coff + 3 C) of dev_out (same shape and pitch): the 5x5, 9x9 and 13x13 window maxima,
 * C channels each.  dev_out may be dev_in, as in the engine, where the SPPF's concat buffer holds all four slices.  An h2 element
 * is compared by its value hi + lo and copied bit for bit; which of several elements of equal value is kept is unspecified.
 * *path_out (may be NULL) receives the kernel the launcher chose: 0 the global-memory kernel, 1 the LDS kernel with one vector
 * per lane group, 4 the LDS kernel with four.  Refused: a null pointer or one that is not 16-byte aligned, an unknown dtype, a
 * size below 1, a negative offset, C / ld / an offset that is no multiple of the vector, a slice that does not fit in ld, in and
 * out slices that overlap in one buffer, two different buffers whose byte ranges overlap, more than 2^31 - 1 elements. */
VTI_DEBUG_OPS_API int32_t vti_debug_sppf_pool(int32_t dtype, const void* dev_in, void* dev_out, int32_t B, int32_t H, int32_t W, int32_t C,
                            int32_t ld, int32_t in_coff, int32_t out_coff, int32_t* path_out, void* stream);
/* vti_debug_upsample2x: nn.Upsample(scale_factor=2, mode="nearest") of channels [in_coff, in_coff + C) of dev_in (T NHWC
 * [B,H,W,in_ld]) into channels [out_coff, out_coff + C) of dev_out (T NHWC [B,2H,2W,out_ld]); a pure copy, so h2 runs as the
 * 4-byte type it is.  Refused: as above, with the two buffers' byte ranges always having to be disjoint. */
VTI_DEBUG_OPS_API int32_t vti_debug_upsample2x(int32_t dtype, const void* dev_in, void* dev_out, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t in_ld, int32_t in_coff, int32_t out_ld, int32_t out_coff, void* stream);
/* vti_debug_decode: the Detect/Segment decode of three levels.  dev_box[l]: f32 [B, H[l]*W[l], 64] (4 sides x 16 DFL bins),
 * dev_cls[l]: f32 [B, H[l]*W[l], nc] logits, dev_mc[l]: f32 [B, H[l]*W[l], nm]; dev_pred: f32 [B, A, 4 + nc + nm] with
 * A = sum H[l]*W[l], levels concatenated.  box_only = 0 runs the full decode kernel (boxes, sigmoid scores, coefficients copied);
 * box_only = 1 the box-only kernel of the plans whose towers write scores and coefficients themselves: it writes the 4 box
 * values of every row and nothing else, and never reads dev_cls / dev_mc (they may be NULL).  Refused: a null array or pointer
 * (box_only = 0: in any of the nine), one that is not 4-byte aligned, box_only outside {0, 1}, a size, stride, B, nc or nm below
 * 1, more than 2^31 - 1 values in pred, and for box_only = 0 nc + nm > VTI_DECODE_MAX_CHANNELS. */
VTI_DEBUG_OPS_API int32_t vti_debug_decode(int32_t box_only, const float* const* dev_box, const float* const* dev_cls, const float* const* dev_mc,
                         const int32_t* H, const int32_t* W, const int32_t* stride, int32_t B, int32_t nc, int32_t nm,
                         float* dev_pred, void* stream);

/* ---- one op of the plan alone, on operands the caller wrote (kernel unit tests of the fused convs) --------- */
/* vti_debug_set_conv_output: the inverse of vti_debug_conv_output.  Writes dev_nchw, f32 NCHW [B,c2,h_out,w_out], into the view
 * conv `i`'s output has in the engine's storage, with the storage's own encode: round-to-nearest fp16, the saturating h2 pair
 * the conv epilogues write, or plain f32.  Only channels [coff, coff + C) of the buffer are touched.  Refused exactly as the
 * reader refuses: B out of range (VTI_ERR_ARG), no weights / no workspace (VTI_ERR_STATE), `i` out of range or a null pointer
 * (VTI_ERR_ARG), a conv whose output is never materialised (VTI_ERR_UNSUPPORTED), a view in a caller tensor that no forward or
 * vti_debug_run_op has named yet (VTI_ERR_STATE).  One copy kernel on `stream`. */
VTI_DEBUG_OPS_API int32_t vti_debug_set_conv_output(vti_ctx* ctx, int32_t i, int32_t B, const float* dev_nchw, void* stream);
/* vti_debug_run_op: issues, once and on `stream`, the launch of the ONE op of the plan that computes conv `i` -- whichever role
 * `i` has in it: the op's own conv, a 1x1 fused into its epilogue, the second 3x3 of a Bottleneck pair, the C2f's closing 1x1 in
 * the pair's tail, the 3x3 a ConvTranspose is folded into, or layer 1 of the stem kernel.  The launch record is the one
 * vti_forward builds for that op (same code); no fork / join events, no side streams.  The op reads whatever its input views
 * hold (vti_debug_set_conv_output) and writes its own outputs, which vti_debug_conv_output then reads.  out_convs (4 ints, may be
 * NULL) receives the conv indices the op computes, in execution order, the rest -1.  dev_input (u8 [B,H,W,3]) is read by the
 * stem op only, dev_pred / dev_best ([B,A,4+nc+nm] / [B,A,2] f32) are written by the towers that scatter into pred (dev_best
 * may be NULL: no pairs), dev_proto by the op that computes proto.cv3; each may be NULL for every other op.  VTI_ERR_ARG with a
 * message naming the argument: `i` or `B` (1..max_batch) out of range, dev_input NULL for the stem, dev_pred NULL for an op that
 * writes pred, dev_proto NULL for the op that writes proto; then vti_forward's state errors (no weights, no workspace). */
VTI_DEBUG_OPS_API int32_t vti_debug_run_op(vti_ctx* ctx, int32_t i, const uint8_t* dev_input, int32_t B, int32_t swap_rb, float* dev_pred,
                         void* dev_proto, float* dev_best, int32_t* out_convs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VTI_H */
