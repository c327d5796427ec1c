// C ABI of libvti.so (declared in include/vti.h): context lifetime, plan execution on the
// caller's HIP stream, error reporting.  Replaces the `ultralytics.YOLO` object the reference
// builds at measurement.py:145 and calls at measurement.py:208-210.
//
// Error convention: every entry point returns a vti_status and records a message; nothing
// throws across the boundary and nothing aborts (measurement.py:207-216 expects predict
// failures to be survivable).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "vti_internal.h"
#include "rawframes_dev.h"

using namespace vti;

struct vti_ctx {
    Options opt;               // the VTI_* switches as vti_create found them
    Plan plan;
    std::string err;
    int device = -1;
    void* d_wpk = nullptr;     // packed weights (device)
    float* d_bias = nullptr;   // biases (device)
    std::vector<float> alpha;  // per conv: accumulator scale of its packed weights (VTI_H2; 1 otherwise)
    char* ws = nullptr;        // caller-owned workspace
    size_t ws_bytes = 0;
    size_t act_bytes = 0;      // activations part; NMS scratch follows
    const void* last_input = nullptr;
    void* last_proto = nullptr;
    // side streams for the independent branches (proto chain, head levels); created with the weights
    hipStream_t side[kNumLanes] = {};
    hipEvent_t ev_fork[kNumLanes] = {};
    hipEvent_t ev_join[kNumLanes] = {};
    bool multi_stream = false;
    // vti_set_nms_table: the ctx's copy of the host bytes (empty: no table) and the caller's device pair
    std::vector<unsigned char> nms_host;
    NmsTable nms_table;
};

static std::string g_create_err;
static const int kMaskSlotsPerFrame = VTI_MASK_SLOTS_PER_FRAME;   // mask work-list capacity: max_batch * 512 instances per call

static int32_t fail(vti_ctx* c, int32_t code, const std::string& msg) {
    if (c) c->err = msg; else g_create_err = msg;
    return code;
}
static int32_t hip_fail(vti_ctx* c, hipError_t e, const char* what) {
    return fail(c, VTI_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// A refused argument: the message is "<fn>: <what>".
static int32_t refuse(vti_ctx* c, const char* fn, const std::string& what, int32_t code = VTI_ERR_ARG) {
    return fail(c, code, std::string(fn) + ": " + what);
}
#define VTI_TRY(call) do { if (int32_t rc_ = (call)) return rc_; } while (0)     // a check that refused: its status is the entry point's
#define VTI_HIP(c, call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return hip_fail((c), e_, (what)); } while (0)

#ifdef VTI_STAMPS
// diagnostic build: medians of the intervals between the in-kernel s_memtime stamps of one launch, to stderr
static void report_stamps(const std::vector<unsigned long long>& h, size_t nwg, bool pk) {
    const char* names[16] = {"start", "c0:top", "c0:A staged", "c0:B staged", "c0:barrier", "c0:mfma done",
                             "c1:top", "c1:A staged", "c1:B staged", "c1:barrier", "c1:mfma done", "epilogue start", "end", "stage2: mfma done", "stage2: stores issued", ""};
    const char* pkn[16] = {"start", "c0:before barrier", "c0:after barrier", "c0:sub-tile A done", "c0:sub-tile B done",
                           "c1:before barrier", "c1:after barrier", "c1:sub-tile A done", "c1:sub-tile B done", "", "", "epilogue start", "end", "", "", ""};
    if (pk) for (int i = 0; i < 16; ++i) names[i] = pkn[i];
    fprintf(stderr, "[stamps] %zu workgroups; median cycles since previous stamp (100 MHz s_memtime ticks x clock)\n", nwg);
    int prev = 0;
    const int order[13] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 12};     // 13: inside the fused stage, before `end` (14 / 15 hold s_memrealtime)
    for (int oi = 0; oi < 13; ++oi) {
        const int i = order[oi];
        std::vector<long long> d;
        for (size_t w = 0; w < nwg; ++w) if (h[w * 16 + i] && h[w * 16 + prev]) d.push_back((long long)(h[w * 16 + i] - h[w * 16 + prev]));
        if (d.empty()) continue;
        std::sort(d.begin(), d.end());
        fprintf(stderr, "[stamps] %-16s median %8lld  p10 %8lld  p90 %8lld\n", names[i], d[d.size() / 2], d[d.size() / 10], d[d.size() * 9 / 10]);
        prev = i;
    }
    std::vector<long long> tot;
    for (size_t w = 0; w < nwg; ++w) tot.push_back((long long)(h[w * 16 + 12] - h[w * 16]));
    std::sort(tot.begin(), tot.end());
    fprintf(stderr, "[stamps] whole workgroup   median %8lld\n", tot[tot.size() / 2]);
    std::vector<double> clk;            // in-kernel shader clock: s_memtime cycles per 100 MHz s_memrealtime tick
    for (size_t w = 0; w < nwg; ++w)
        if (h[w * 16 + 15] > h[w * 16 + 14]) clk.push_back((double)(h[w * 16 + 12] - h[w * 16]) / (double)(h[w * 16 + 15] - h[w * 16 + 14]) * 0.1);
    if (!clk.empty()) { std::sort(clk.begin(), clk.end()); fprintf(stderr, "[stamps] in-kernel clock    median %.3f GHz (p10 %.3f, p90 %.3f)\n", clk[clk.size() / 2], clk[clk.size() / 10], clk[clk.size() * 9 / 10]); }
}

// diagnostic build: launch() once with p.stamps pointing at nwg x 16 zeroed slots, wait, then the header line (if any) and the
// medians to stderr.  false when the stamp buffer could not be allocated (nothing was launched).
template <typename L>
static bool stamped_launch(ConvParams& p, size_t nwg, bool pk, hipStream_t st, const char* header, L&& launch) {
    unsigned long long* d_st = nullptr;
    if (hipMalloc((void**)&d_st, nwg * 16 * 8) != hipSuccess) return false;
    (void)hipMemset(d_st, 0, nwg * 16 * 8);
    p.stamps = d_st;
    (void)launch();
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> h(nwg * 16);
    (void)hipMemcpy(h.data(), d_st, nwg * 16 * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_st);
    p.stamps = nullptr;
    if (header) fprintf(stderr, "%s\n", header);
    report_stamps(h, nwg, pk);
    return true;
}

#endif

// The settings that vti_measure_params and vti_checker_params have in common: nullptr when they are valid.
template <typename P>
static const char* settings_error(const P& p) {
    if (p.stitch_id < 0 || p.fabric_id < 0 || p.stitch_id == p.fabric_id) return "stitch_id and fabric_id must be >= 0 and different";
    if (p.envelope_neighborhood < 0 || p.envelope_neighborhood > 64) return "envelope_neighborhood must be 0..64";
    if (p.min_stitches < 1 || p.kmeans_iters < 0 || (p.skip_cluster != 0 && p.skip_cluster != 1) ||
        (p.drop_empty != 0 && p.drop_empty != 1) || p.frame_buffer < 1)
        return "bad setting (min_stitches, frame_buffer >= 1; kmeans_iters >= 0; flags 0 or 1)";
    if (!(p.max_px_distance == p.max_px_distance)) return "NaN threshold";
    return nullptr;
}

// The checks of one vti_measure_params (vti_measure's struct, every entry of vti_measure_pack_cameras): nullptr when it is valid.
static const char* measure_params_error(const vti_measure_params& p) {
    if (const char* e = settings_error(p)) return e;
    return p.two_row_threshold_px == p.two_row_threshold_px ? nullptr : "NaN threshold";
}

// The single-kernel debug hooks (vti_debug_sppf_pool, vti_debug_upsample2x):
// One channel slice [coff, coff + C) of a T NHWC tensor of pitch ld: "" or what is wrong with it (vec = elements per 16 bytes).
static std::string slice_error(const char* what, int C, int ld, int coff, int vec) {
    if (C < 1 || ld < 1 || coff < 0) return std::string(what) + ": C and ld must be >= 1, the channel offset >= 0";
    if (C % vec || ld % vec || coff % vec)
        return std::string(what) + ": C, ld and the channel offset must be multiples of the 16-byte vector (" + std::to_string(vec) + " elements)";
    if ((int64_t)coff + C > ld) return std::string(what) + ": channels [" + std::to_string(coff) + ", " + std::to_string((int64_t)coff + C) +
                                       ") do not fit in ld = " + std::to_string(ld);
    return "";
}
static bool ranges_overlap(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

extern "C" {

int32_t vti_create(const vti_desc* desc, vti_ctx** out) {
    if (!desc || !out) return fail(nullptr, VTI_ERR_ARG, "vti_create: null argument");
    *out = nullptr;
    vti_ctx* c = new (std::nothrow) vti_ctx();
    if (!c) return fail(nullptr, VTI_ERR_NOMEM, "vti_create: out of host memory");
    std::string e;
    c->opt = options_from_env();
    try { e = c->plan.build(*desc, c->opt.plan); } catch (const std::exception& ex) { e = ex.what(); }
    if (!e.empty()) { delete c; return fail(nullptr, VTI_ERR_ARG, "vti_create: " + e); }
    c->act_bytes = c->plan.ws_bytes;
    *out = c;
    return VTI_OK;
}

void vti_destroy(vti_ctx* c) {
    if (!c) return;
    if (c->d_wpk) (void)hipFree(c->d_wpk);
    if (c->d_bias) (void)hipFree(c->d_bias);
    for (int l = 1; l < kNumLanes; ++l) {
        if (c->side[l]) (void)hipStreamDestroy(c->side[l]);
        if (c->ev_fork[l]) (void)hipEventDestroy(c->ev_fork[l]);
        if (c->ev_join[l]) (void)hipEventDestroy(c->ev_join[l]);
    }
    delete c;
}

const char* vti_last_error(const vti_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int32_t vti_num_convs(const vti_ctx* c) { return c ? (int32_t)c->plan.convs.size() : 0; }

int32_t vti_conv_at(const vti_ctx* c, int32_t i, vti_conv_info* o) {
    if (!c || !o || i < 0 || i >= (int32_t)c->plan.convs.size()) return VTI_ERR_ARG;
    const ConvRow& r = c->plan.convs[i];
    memset(o, 0, sizeof *o);
    snprintf(o->name, sizeof o->name, "%s", r.name.c_str());
    o->c1 = r.c1; o->c2 = r.c2; o->k = r.k; o->s = r.s; o->kind = r.kind;
    o->h_in = r.h_in; o->w_in = r.w_in; o->h_out = r.h_out; o->w_out = r.w_out;
    o->macs = r.macs();
    conv_geometry(c->plan, i, o);
    return VTI_OK;
}

int32_t vti_num_anchors(const vti_ctx* c) { return c ? c->plan.num_anchors : 0; }
int64_t vti_fused_params(const vti_ctx* c) { return c ? c->plan.fused_params : 0; }
int64_t vti_macs_per_frame(const vti_ctx* c) { return c ? c->plan.macs : 0; }
int64_t vti_workspace_bytes(const vti_ctx* c) {
    if (!c) return 0;
    const vti_desc& d = c->plan.desc;
    return (int64_t)(c->plan.ws_bytes + nms_workspace_bytes(d.max_batch, c->plan.num_anchors) +
                     masks_workspace_bytes(d.max_batch * kMaskSlotsPerFrame, d.H, d.W));
}
int32_t vti_num_launches(const vti_ctx* c) {
    if (!c) return 0;
    int32_t n = 0;
    for (const Op& op : c->plan.ops) n += (op.kind != OP_FORK && op.kind != OP_JOIN);
    return n;
}

int32_t vti_load_weights(vti_ctx* c, const void* blob, size_t nbytes, int32_t device) {
    if (!c) return VTI_ERR_ARG;
    std::vector<uint8_t> wpk;
    std::vector<float> bias;
    std::string e;
    try { e = pack_weights(c->plan, blob, nbytes, wpk, bias, c->alpha); } catch (const std::exception& ex) { e = ex.what(); }
    if (!e.empty()) return fail(c, VTI_ERR_WEIGHTS, e);
    VTI_HIP(c, hipSetDevice(device), "hipSetDevice");
    if (c->d_wpk) { (void)hipFree(c->d_wpk); c->d_wpk = nullptr; }
    if (c->d_bias) { (void)hipFree(c->d_bias); c->d_bias = nullptr; }
    VTI_HIP(c, hipMalloc(&c->d_wpk, wpk.size()), "hipMalloc(weights)");
    VTI_HIP(c, hipMalloc((void**)&c->d_bias, bias.size() * sizeof(float)), "hipMalloc(bias)");
    VTI_HIP(c, hipMemcpy(c->d_wpk, wpk.data(), wpk.size(), hipMemcpyHostToDevice), "hipMemcpy(weights)");
    VTI_HIP(c, hipMemcpy(c->d_bias, bias.data(), bias.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(bias)");
    c->device = device;
    // side streams (VTI_SINGLE_STREAM=1 keeps everything on the caller's stream)
    if (!c->opt.run.single_stream && !c->side[1]) {
        bool ok = true;
        for (int l = 1; l < kNumLanes && ok; ++l) {
            ok = hipStreamCreateWithFlags(&c->side[l], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&c->ev_fork[l], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&c->ev_join[l], hipEventDisableTiming) == hipSuccess;
        }
        c->multi_stream = ok;
    }
    return VTI_OK;
}

int32_t vti_set_workspace(vti_ctx* c, void* dev_ws, size_t nbytes) {
    if (!c) return VTI_ERR_ARG;
    if (!dev_ws || ((uintptr_t)dev_ws & 255)) return fail(c, VTI_ERR_ARG, "vti_set_workspace: pointer must be 256-B aligned");
    if ((int64_t)nbytes < vti_workspace_bytes(c)) return fail(c, VTI_ERR_NOMEM, "vti_set_workspace: workspace too small");
    c->ws = (char*)dev_ws;
    c->ws_bytes = nbytes;
    return VTI_OK;
}

// A ctx is bound to the device its weights were uploaded to (vti_load_weights); every launching entry point refuses to run
// with another device current instead of launching there with pointers of the wrong GPU.
static int32_t check_device(vti_ctx* c, const char* fn) {
    if (!c || c->device < 0) return VTI_OK;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != c->device)
        return fail(c, VTI_ERR_STATE, std::string(fn) + ": ctx is bound to device " + std::to_string(c->device) +
                    " but the current device is " + std::to_string(cur) + " (hipSetDevice / torch.cuda.set_device it first)");
    return VTI_OK;
}

static int32_t check_ready(vti_ctx* c, int32_t B, const char* fn) {
    if (!c) return VTI_ERR_ARG;
    if (int32_t rc = check_device(c, fn)) return rc;
    if (B < 0 || B > c->plan.desc.max_batch) return fail(c, VTI_ERR_ARG, std::string(fn) + ": B out of range (0..max_batch)");
    if (!c->d_wpk) return fail(c, VTI_ERR_STATE, std::string(fn) + ": weights not loaded");
    if (!c->ws) return fail(c, VTI_ERR_STATE, std::string(fn) + ": workspace not set");
    return VTI_OK;
}

int32_t vti_letterbox(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, uint8_t* out, void* stream) {
    if (!c || !frames || !out || H0 < 1 || W0 < 1 || B < 0) return fail(c, VTI_ERR_ARG, "vti_letterbox: bad argument");
    if (int32_t drc = check_device(c, "vti_letterbox")) return drc;
    VTI_HIP(c, launch_letterbox(frames, B, H0, W0, nullptr, out, c->plan.desc.H, c->plan.desc.W, (hipStream_t)stream),
            "letterbox kernel");
    return VTI_OK;
}

}  // extern "C": the calls that take a frame table or a window table are one template over what differs between the two kinds

// ---- batches whose frames differ in size (the frame table) and predicts on a window of each frame (the window table) ----------
static const int32_t kFrameMaxSide = 16384;      // vti_mask_polygons' limit

// What is wrong with one frame of a table for the H x W canvas (nullptr: nothing).  The pack calls run it on their arguments and
// every call that takes a table on the rows of the host table it is given, so each value a kernel forms an address from was
// checked by the host at the call.
static const char* frame_error(int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t offset, int64_t total_bytes) {
    if (H0 < 1 || W0 < 1) return "H0 and W0 must be >= 1";
    if (H0 > kFrameMaxSide || W0 > kFrameMaxSide) return "H0 and W0 must be <= 16384";
    if (offset < 0 || (offset & 15)) return "byte_offset must be >= 0 and a multiple of 16";
    if (offset > total_bytes || 3 * (int64_t)H0 * W0 > total_bytes - offset) return "the frame runs past total_bytes";
    int nh, nw, top, left;
    letterbox_geom(H0, W0, H, W, nh, nw, top, left);
    if (nh < 1 || nw < 1) return "the resized frame would be below 1 px";
    if (top < 0 || left < 0 || top + nh > H || left + nw > W) return "the resized frame does not fit the canvas";
    return nullptr;
}

// What is wrong with one window of an H0 x W0 frame for the H x W canvas (nullptr: nothing); the frame itself passed frame_error.
static const char* window_error(int32_t H, int32_t W, int32_t H0, int32_t W0, int32_t x0, int32_t y0, int32_t w, int32_t h) {
    if (w < 1 || h < 1) return "the window's w and h must be >= 1";
    if (x0 < 0 || y0 < 0 || x0 > W0 - w || y0 > H0 - h) return "the window does not lie inside its frame";
    int nh, nw, top, left;
    letterbox_geom(h, w, H, W, nh, nw, top, left);
    if (nh < 1 || nw < 1) return "the resized window would be below 1 px";
    if (top < 0 || left < 0 || top + nh > H || left + nw > W) return "the resized window does not fit the canvas";
    return nullptr;
}

// What is wrong with the frame a packed row describes: frame_error, and a size above the header's recorded maximum.
static const char* packed_frame_error(const FrameTableHeader& h, int32_t H0, int32_t W0, int64_t offset) {
    const char* e = frame_error(h.H, h.W, H0, W0, offset, h.total_bytes);
    if (!e && (H0 > h.max_H0 || W0 > h.max_W0)) e = "larger than the table's recorded maximum";
    return e;
}

// What differs between the two kinds of table: the row and the magic, the words of the messages, what a pack call takes and
// writes per frame, what is wrong with a packed row, what vti_*_table_info reports beyond the letterbox row, the launchers, and in
// the ragged-mask checks one pointer and one alignment (the frame form crops to dev_xyxy, the window form reads dev_dets in pairs).
struct FrameKind {
    using Row = FrameRow;
    static constexpr int magic = kFrameTableMagic;
    static constexpr bool windowed = false;
    static constexpr int info_ints = 8;
    static constexpr const char *noun = "frame", *packer = "vti_pack_frames";
    static constexpr const char *letterbox_fn = "vti_letterbox_frames", *letterbox_kernel = "letterbox kernel";
    static constexpr const char *scale_boxes_fn = "vti_scale_boxes_frames", *scale_boxes_kernel = "scale_boxes kernel";
    static constexpr const char *masks_fn = "vti_masks_native_frames", *masks_kernel = "native mask kernel (frames)";
    static constexpr const char* predict_fn = "vti_predict_frames_native";
    static constexpr const char* xyxy_required = "dev_xyxy is required (the masks are cropped to the frame-px boxes)";
    static constexpr const char* masks_alignment = "dev_masks and dev_mask_bases must be 8-byte aligned, dev_offsets 4-byte aligned";
    static constexpr const char* no_layout = "a frame of host_table has no native mask layout (slot below 2 GiB)";
    static const FrameRow& letterbox_row(const FrameRow& r) { return r; }
    static void info_tail(const FrameRow&, int32_t*) {}
    static const char* pack_error(int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t offset, int64_t total_bytes, const int32_t*) {
        return frame_error(H, W, H0, W0, offset, total_bytes);
    }
    static void pack_row(int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t offset, const int32_t*, FrameRow& r) {
        frame_row_fill(H, W, H0, W0, offset, r);
    }
    static const char* row_error(const FrameTableHeader& h, const FrameRow& r) { return packed_frame_error(h, r.H0, r.W0, r.offset); }
    static bool masks_pointer_missing(const float* xyxy) { return !xyxy; }
    static bool masks_dets_misaligned(const float*) { return false; }
    static hipError_t letterbox(const uint8_t* frames, int B, const FrameRow* rows, uint8_t* out, int H, int W, hipStream_t st) {
        return launch_letterbox(frames, B, 0, 0, rows, out, H, W, st);
    }
    static hipError_t scale_boxes(const float* dets, const int* counts, int B, int max_det, const vti_desc& d, const FrameRow* rows,
                                  float* xyxy, hipStream_t st) {
        return launch_scale_boxes(dets, counts, B, max_det, d.nm, d.H, d.W, 0, 0, rows, xyxy, st);
    }
    static constexpr auto masks = launch_masks_native_frames;
};
struct WindowKind {
    using Row = WindowRow;
    static constexpr int magic = kWindowTableMagic;
    static constexpr bool windowed = true;       // the pack call takes `windows` and, given a ctx, holds B to its max_batch
    static constexpr int info_ints = 12;
    static constexpr const char *noun = "window", *packer = "vti_pack_windows";
    static constexpr const char *letterbox_fn = "vti_letterbox_windows", *letterbox_kernel = "letterbox kernel (windows)";
    static constexpr const char *scale_boxes_fn = "vti_scale_boxes_windows", *scale_boxes_kernel = "scale_boxes kernel (windows)";
    static constexpr const char *masks_fn = "vti_masks_native_windows", *masks_kernel = "native mask kernel (windows)";
    static constexpr const char* predict_fn = "vti_predict_windows";
    static constexpr const char* xyxy_required = "dev_xyxy is required";
    static constexpr const char* masks_alignment =
        "dev_masks, dev_mask_bases and dev_dets must be 8-byte aligned, dev_offsets 4-byte aligned";
    static constexpr const char* no_layout = "a frame or a window of host_table has no native mask layout (slot below 2 GiB)";
    static const FrameRow& letterbox_row(const WindowRow& w) { return w.crop; }
    static void info_tail(const WindowRow& w, int32_t* v) { v[0] = w.x0; v[1] = w.y0; v[2] = w.H0; v[3] = w.W0; }
    static const char* pack_error(int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t offset, int64_t total_bytes, const int32_t* w) {
        const char* e = frame_error(H, W, H0, W0, offset, total_bytes);
        return e ? e : window_error(H, W, H0, W0, w[0], w[1], w[2], w[3]);
    }
    static void pack_row(int32_t H, int32_t W, int32_t H0, int32_t W0, int64_t offset, const int32_t* w, WindowRow& r) {
        memset(&r, 0, sizeof r);
        frame_row_fill(H, W, w[3], w[2], offset + 3 * ((int64_t)w[1] * W0 + w[0]), r.crop);
        r.frame_offset = offset; r.H0 = H0; r.W0 = W0; r.x0 = w[0]; r.y0 = w[1];
    }
    // the row's frame passes frame_error, its window window_error, and the crop row holds the window's size and first byte (what the
    // kernels form addresses from)
    static const char* row_error(const FrameTableHeader& h, const WindowRow& w) {
        const char* e = packed_frame_error(h, w.H0, w.W0, w.frame_offset);
        if (!e) e = window_error(h.H, h.W, w.H0, w.W0, w.x0, w.y0, w.crop.W0, w.crop.H0);
        if (!e && w.crop.offset != w.frame_offset + 3 * ((int64_t)w.y0 * w.W0 + w.x0)) e = "the window's first byte is not where its origin puts it";
        return e;
    }
    static bool masks_pointer_missing(const float*) { return false; }
    static bool masks_dets_misaligned(const float* dets) { return (uintptr_t)dets & 7; }
    static constexpr auto letterbox = launch_letterbox_windows;
    static hipError_t scale_boxes(const float* dets, const int* counts, int B, int max_det, const vti_desc& d, const WindowRow* rows,
                                  float* xyxy, hipStream_t st) {
        return launch_scale_boxes_windows(dets, counts, B, max_det, d.nm, rows, xyxy, st);
    }
    static hipError_t masks(int dtype, const float* dets, const float*, const int* counts, const void* proto, const WindowRow* rows, int B,
                            int max_det, int Hp, int Wp, int mode, uint8_t* out, long long capacity_bytes, int* offsets,
                            long long* bases, void* ws, hipStream_t st) {
        return launch_masks_native_windows(dtype, dets, counts, proto, rows, B, max_det, Hp, Wp, mode, out, capacity_bytes, offsets, bases,
                                           ws, st);
    }
};

// The header of a host table, row k of it, and the rows of its device copy.
static FrameTableHeader table_header(const void* host_table) { FrameTableHeader h; memcpy(&h, host_table, sizeof h); return h; }
template <class K>
static typename K::Row host_row(const void* host_table, int32_t k) {
    typename K::Row r;
    memcpy(&r, (const char*)host_table + sizeof(FrameTableHeader) + (size_t)k * sizeof r, sizeof r);
    return r;
}
template <class K>
static const typename K::Row* dev_rows(const void* dev_table) {
    return (const typename K::Row*)((const char*)dev_table + sizeof(FrameTableHeader));
}

template <class K>
static int64_t table_bytes(int32_t B) {
    return B < 1 ? 0 : (int64_t)sizeof(FrameTableHeader) + (int64_t)B * (int64_t)sizeof(typename K::Row);
}

// `windows`: four ints (x0, y0, w, h) per frame, for a window table only.
template <class K>
static int32_t pack_table(vti_ctx* c, int32_t H, int32_t W, const int32_t* H0, const int32_t* W0, const int64_t* byte_offset,
                          const int32_t* windows, int32_t B, int64_t total_bytes, void* host_table, size_t nbytes) {
    if (!H0 || !W0 || !byte_offset || (K::windowed && !windows) || !host_table || B < 1)
        return refuse(c, K::packer, "null array or table, or B < 1");
    if (H < 32 || W < 32 || (H & 31) || (W & 31) || total_bytes < 0)
        return refuse(c, K::packer, "the canvas H, W must be multiples of 32, total_bytes >= 0");
    if ((int64_t)nbytes < table_bytes<K>(B)) return refuse(c, K::packer, std::string("table smaller than vti_") + K::noun + "_table_bytes()");
    if (K::windowed && c && B > c->plan.desc.max_batch) return refuse(c, K::packer, "B above the ctx's max_batch");
    auto window = [&](int32_t b) { return K::windowed ? windows + 4 * (size_t)b : nullptr; };
    for (int32_t b = 0; b < B; ++b)
        if (const char* e = K::pack_error(H, W, H0[b], W0[b], byte_offset[b], total_bytes, window(b)))
            return refuse(c, K::packer, "frame " + std::to_string(b) + ": " + e);
    FrameTableHeader h;
    memset(&h, 0, sizeof h);
    h.magic = K::magic; h.B = B; h.H = H; h.W = W; h.total_bytes = total_bytes;
    for (int32_t b = 0; b < B; ++b) {
        typename K::Row r;
        K::pack_row(H, W, H0[b], W0[b], byte_offset[b], window(b), r);
        h.max_H0 = std::max(h.max_H0, H0[b]); h.max_W0 = std::max(h.max_W0, W0[b]);
        memcpy((char*)host_table + sizeof h + (size_t)b * sizeof r, &r, sizeof r);
    }
    memcpy(host_table, &h, sizeof h);
    return VTI_OK;
}

// b = -1: the header.  Else row b: its letterbox row, then what K::info_tail adds, and the doubles (out_f64 may be null).
template <class K>
static int32_t table_info(const void* host_table, int32_t b, int32_t* out_i32, double* out_f64) {
    if (!host_table || !out_i32) return VTI_ERR_ARG;
    const FrameTableHeader h = table_header(host_table);
    if (h.magic != K::magic || h.B < 1 || b < -1 || b >= h.B) return VTI_ERR_ARG;
    int32_t v[K::info_ints] = {h.B, h.H, h.W, h.max_H0, h.max_W0, 0, (int32_t)(h.total_bytes & 0xffffffff), (int32_t)(h.total_bytes >> 32)};
    if (b >= 0) {
        const typename K::Row row = host_row<K>(host_table, b);
        const FrameRow& r = K::letterbox_row(row);
        const int32_t lb[8] = {r.H0, r.W0, r.new_h, r.new_w, r.top, r.left, (int32_t)(r.offset & 0xffffffff), (int32_t)(r.offset >> 32)};
        memcpy(v, lb, sizeof lb);
        K::info_tail(row, v + 8);
        if (out_f64) { out_f64[0] = r.scale_x; out_f64[1] = r.scale_y; out_f64[2] = r.gain; out_f64[3] = r.padx; out_f64[4] = r.pady; }
    }
    memcpy(out_i32, v, sizeof v);
    return VTI_OK;
}

template <class K>
static std::string not_a_table() { return std::string("host_table is not a table of ") + K::packer; }
template <class K>
static std::string packed_for_another(const char* what) { return std::string("the ") + K::noun + " table was packed for another " + what; }

// What is wrong with a packed host table for this ctx (empty: nothing): not a table of K's pack call, packed for another B (B < 0:
// any B >= 1) or another canvas, or a row that no longer passes K::row_error (`frame` then receives its index, else -1).  Fails
// nothing and records nothing: table_check and the host-only size queries share it.  `h` receives the header.
template <class K>
static std::string table_problem(const vti_ctx* c, const void* host_table, int32_t B, FrameTableHeader& h, int32_t& frame) {
    frame = -1;
    h = table_header(host_table);
    if (h.magic != K::magic) return not_a_table<K>();
    if (h.B < 1 || (B >= 0 && h.B != B)) return packed_for_another<K>("B");
    if (h.H != c->plan.desc.H || h.W != c->plan.desc.W) return packed_for_another<K>("canvas (H x W)");
    for (int32_t b = 0; b < h.B; ++b)
        if (const char* e = K::row_error(h, host_row<K>(host_table, b))) { frame = b; return e; }
    return {};
}

// The checks every call makes on its table pair before anything else: the host copy is a packed table of kind K for this ctx's
// canvas and this B whose rows still pass K::row_error, and the device copy is a 16-byte aligned pointer.  `h` receives the header.
template <class K>
static int32_t table_check(const char* fn, vti_ctx* c, const void* host_table, const void* dev_table, int32_t B, FrameTableHeader& h) {
    if (!c) return VTI_ERR_ARG;
    if (!host_table || !dev_table) return refuse(c, fn, std::string("null ") + K::noun + " table (host copy or device copy)");
    if ((uintptr_t)dev_table & 15) return refuse(c, fn, std::string("the device ") + K::noun + " table must be 16-byte aligned");
    if (B < 1) {                            // no table is packed for B < 1 (table_problem reads B < 0 as "any B")
        h = table_header(host_table);
        return refuse(c, fn, h.magic != K::magic ? not_a_table<K>() : packed_for_another<K>("B"));
    }
    int32_t frame;
    const std::string e = table_problem<K>(c, host_table, B, h, frame);
    if (e.empty()) return VTI_OK;
    return refuse(c, fn, frame < 0 ? e : "frame " + std::to_string(frame) + " of host_table: " + e);
}

// The frame-table forms under the names the other families call them by.
static FrameRow table_row(const void* host_table, int32_t k) { return host_row<FrameKind>(host_table, k); }
static const FrameRow* frame_rows(const void* dev_table) { return dev_rows<FrameKind>(dev_table); }
static int32_t frames_check(const char* fn, vti_ctx* c, const void* host_table, const void* dev_table, int32_t B, FrameTableHeader& h) {
    return table_check<FrameKind>(fn, c, host_table, dev_table, B, h);
}

template <class K>
static int32_t letterbox_table(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B, uint8_t* out,
                               void* stream) {
    const char* fn = K::letterbox_fn;
    FrameTableHeader h;
    VTI_TRY(table_check<K>(fn, c, host_table, dev_table, B, h));
    if (!frames || !out) return refuse(c, fn, "null frames or output");
    if (((uintptr_t)frames & 15) || ((uintptr_t)out & 3)) return refuse(c, fn, "dev_frames must be 16-byte aligned, dev_input 4-byte aligned");
    if (B > c->plan.desc.max_batch) return refuse(c, fn, "B above max_batch");
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, K::letterbox(frames, B, dev_rows<K>(dev_table), out, h.H, h.W, (hipStream_t)stream), K::letterbox_kernel);
    return VTI_OK;
}

template <class K>
static int32_t scale_boxes_table(vti_ctx* c, const float* dets, const int32_t* counts, const void* host_table, const void* dev_table,
                                 int32_t B, int32_t max_det, float* xyxy, void* stream) {
    const char* fn = K::scale_boxes_fn;
    FrameTableHeader h;
    VTI_TRY(table_check<K>(fn, c, host_table, dev_table, B, h));
    if (!dets || !counts || !xyxy || max_det < 1 || ((uintptr_t)xyxy & 15))
        return refuse(c, fn, "bad argument (null pointer, max_det < 1 or dev_xyxy not 16-byte aligned)");
    if ((int64_t)B * max_det > INT32_MAX) return refuse(c, fn, "B * max_det out of range");
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, K::scale_boxes(dets, counts, B, max_det, c->plan.desc, dev_rows<K>(dev_table), xyxy, (hipStream_t)stream), K::scale_boxes_kernel);
    return VTI_OK;
}

// The table predicts up to the NMS: the checks on what those stages take, then letterbox -> scored forward -> NMS.
template <class K>
static int32_t predict_table_head(const char* fn, vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table,
                                  int32_t B, int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic,
                                  uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts, const float* xyxy,
                                  void* stream) {
    if (!frames || !input_scratch || ((uintptr_t)frames & 15) || ((uintptr_t)input_scratch & 3))
        return refuse(c, fn, "dev_frames (16-byte aligned) and dev_input_scratch (4-byte aligned) are required");
    if (xyxy && (max_det < 1 || ((uintptr_t)xyxy & 15) || !dets || !counts))
        return refuse(c, fn, "bad argument (max_det < 1, null dets / counts or dev_xyxy not 16-byte aligned)");
    VTI_TRY(check_ready(c, B, fn));
    const vti_desc& d = c->plan.desc;
    VTI_TRY(letterbox_table<K>(c, frames, host_table, dev_table, B, input_scratch, stream));
    float* best = nms_workspace_best(c->ws + c->act_bytes, d.max_batch, c->plan.num_anchors);
    VTI_TRY(vti_forward_scored(c, input_scratch, B, swap_rb, pred, proto, best, stream));
    return vti_nms_scored(c, pred, best, B, conf, iou, max_det, agnostic, dets, counts, stream);
}

// ---- frame-resolution masks through a table: the ragged mask buffer -----------------------------------------------------------
template <class K>
static int64_t mask_native_table_bytes(const vti_ctx* c, const void* host_table, int32_t max_det) {
    if (!c || !host_table || max_det < 1) return 0;
    FrameTableHeader h;
    int32_t frame;
    if (!table_problem<K>(c, host_table, -1, h, frame).empty() || h.B > c->plan.desc.max_batch) return 0;
    const long long n = native_table_bytes<typename K::Row>(host_table, h.H / 4, h.W / 4, max_det, nullptr);
    return n < 0 ? 0 : n;
}

// The argument checks of the ragged-mask calls (everything but the table, which table_check has passed).
template <class K>
static int32_t masks_native_table_check(const char* fn, vti_ctx* c, const float* dets, const float* xyxy, const int32_t* counts,
                                        const void* proto, const void* host_table, int32_t B, int32_t max_det, int32_t mode,
                                        int32_t packing, const uint8_t* masks, int64_t capacity_bytes, const int32_t* offsets,
                                        const int64_t* bases) {
    if (!dets || K::masks_pointer_missing(xyxy) || !counts || !proto || !offsets || !bases || max_det < 1 || capacity_bytes < 0 ||
        (capacity_bytes && !masks))
        return refuse(c, fn, "bad argument (null pointer, max_det < 1 or capacity_bytes < 0)");
    if (mode != VTI_MASK_LOGIT && mode != VTI_MASK_SIGMOID) return refuse(c, fn, "bad mode");
    if (packing == VTI_PACK_U8) return refuse(c, fn, "the ragged mask buffer is bit-packed only (VTI_PACK_BITS)", VTI_ERR_UNSUPPORTED);
    if (packing != VTI_PACK_BITS) return refuse(c, fn, "bad packing");
    if (((uintptr_t)masks & 7) || ((uintptr_t)bases & 7) || ((uintptr_t)offsets & 3) || K::masks_dets_misaligned(dets))
        return refuse(c, fn, K::masks_alignment);
    const vti_desc& d = c->plan.desc;
    if (B > d.max_batch) return refuse(c, fn, "B out of range");
    if (d.nm != 32) return refuse(c, fn, "only nm == 32 prototypes", VTI_ERR_UNSUPPORTED);
    long long tiles = 0;
    if (native_table_bytes<typename K::Row>(host_table, d.H / 4, d.W / 4, max_det, &tiles) < 0) return refuse(c, fn, K::no_layout);
    if (tiles > INT32_MAX || (int64_t)B * max_det > INT32_MAX) return refuse(c, fn, "too many tiles or slots for one call", VTI_ERR_UNSUPPORTED);
    return VTI_OK;
}

// `xyxy`: the frame form's frame-px boxes; the window form recomputes its boxes from dets and takes none.
template <class K>
static int32_t masks_native_table(vti_ctx* c, const float* dets, const float* xyxy, const int32_t* counts, const void* proto,
                                  const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t mode,
                                  int32_t packing, uint8_t* masks, int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases,
                                  void* stream) {
    const char* fn = K::masks_fn;
    FrameTableHeader h;
    VTI_TRY(table_check<K>(fn, c, host_table, dev_table, B, h));
    VTI_TRY(masks_native_table_check<K>(fn, c, dets, xyxy, counts, proto, host_table, B, max_det, mode, packing, masks, capacity_bytes,
                                        offsets, mask_bases));
    if (!c->ws) return refuse(c, fn, "workspace not set", VTI_ERR_STATE);
    const vti_desc& d = c->plan.desc;
    void* mws = c->ws + c->act_bytes + nms_workspace_bytes(d.max_batch, c->plan.num_anchors);
    if (masks_native_frames_workspace_bytes(B) > masks_workspace_bytes(d.max_batch * kMaskSlotsPerFrame, d.H, d.W))
        return refuse(c, fn, "workspace too small", VTI_ERR_NOMEM);
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, K::masks(d.dtype, dets, xyxy, counts, proto, dev_rows<K>(dev_table), B, max_det, d.H / 4, d.W / 4, mode, masks,
                        capacity_bytes, offsets, (long long*)mask_bases, mws, (hipStream_t)stream), K::masks_kernel);
    return VTI_OK;
}

// Letterbox -> scored forward -> NMS -> boxes in frame px -> ragged frame-resolution masks, every check ahead of the first launch.
template <class K>
static int32_t predict_table_native(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                                    int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode,
                                    int32_t packing, uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts,
                                    uint8_t* masks, int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases, float* xyxy,
                                    void* stream) {
    const char* fn = K::predict_fn;
    const int32_t mode = mask_mode & ~VTI_MASK_NATIVE;
    FrameTableHeader h;
    VTI_TRY(table_check<K>(fn, c, host_table, dev_table, B, h));
    if (!xyxy) return refuse(c, fn, K::xyxy_required);
    if (!pred) return refuse(c, fn, "null dev_pred");
    VTI_TRY(masks_native_table_check<K>(fn, c, dets, xyxy, counts, proto, host_table, B, max_det, mode, packing, masks, capacity_bytes,
                                        offsets, mask_bases));
    VTI_TRY(predict_table_head<K>(fn, c, frames, host_table, dev_table, B, swap_rb, conf, iou, max_det, agnostic, input_scratch, pred,
                                  proto, dets, counts, xyxy, stream));
    VTI_TRY(scale_boxes_table<K>(c, dets, counts, host_table, dev_table, B, max_det, xyxy, stream));
    return masks_native_table<K>(c, dets, xyxy, counts, proto, host_table, dev_table, B, max_det, mode, packing, masks, capacity_bytes,
                                 offsets, mask_bases, stream);
}

extern "C" {

int64_t vti_frame_table_bytes(int32_t B) { return table_bytes<FrameKind>(B); }
int64_t vti_window_table_bytes(int32_t B) { return table_bytes<WindowKind>(B); }

int32_t vti_pack_frames(vti_ctx* c, int32_t H, int32_t W, const int32_t* H0, const int32_t* W0, const int64_t* byte_offset, int32_t B,
                        int64_t total_bytes, void* host_table, size_t nbytes) {
    return pack_table<FrameKind>(c, H, W, H0, W0, byte_offset, nullptr, B, total_bytes, host_table, nbytes);
}
int32_t vti_pack_windows(vti_ctx* c, int32_t H, int32_t W, const int32_t* H0, const int32_t* W0, const int64_t* byte_offset,
                         const int32_t* windows, int32_t B, int64_t total_bytes, void* host_table, size_t nbytes) {
    return pack_table<WindowKind>(c, H, W, H0, W0, byte_offset, windows, B, total_bytes, host_table, nbytes);
}

int32_t vti_frame_table_info(const void* host_table, int32_t b, int32_t out_i32[8], double out_f64[5]) {
    return table_info<FrameKind>(host_table, b, out_i32, out_f64);
}
int32_t vti_window_table_info(const void* host_table, int32_t b, int32_t out_i32[12], double out_f64[5]) {
    return table_info<WindowKind>(host_table, b, out_i32, out_f64);
}

int32_t vti_letterbox_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                             uint8_t* out, void* stream) {
    return letterbox_table<FrameKind>(c, frames, host_table, dev_table, B, out, stream);
}
int32_t vti_letterbox_windows(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                              uint8_t* out, void* stream) {
    return letterbox_table<WindowKind>(c, frames, host_table, dev_table, B, out, stream);
}

// The tensors of one forward: the ctx's weights and workspace, the caller's input and outputs.
static Bindings bindings_of(const vti_ctx* c, const void* input, float* pred, void* proto, float* best) {
    return Bindings{c->ws, c->d_wpk, c->d_bias, c->alpha.data(), input, pred, proto, best};
}

static hipError_t launch_record(const LaunchRec& L, hipStream_t st) {
    switch (L.fn) {
    case LAUNCH_STEM_L1: return launch_stem_l1(L.dtype, L.conv, st, L.persistent);
    case LAUNCH_CONV: return launch_conv(L.dtype, L.ks, L.stride, L.nrep, L.mode, L.conv, L.lds, st);
    case LAUNCH_CONVFOLD: return launch_convfold(L.dtype, L.conv, L.lds, st);
    case LAUNCH_CONV_PK_FOLD: return launch_conv_pk_fold(L.dtype, L.conv, L.lds, st);
    case LAUNCH_POOL: return launch_sppf_pool(L.dtype, L.pool, st);
    case LAUNCH_UP2: return launch_upsample2x(L.dtype, L.up2, st);
    case LAUNCH_DECODE: return launch_decode(L.dec, st);
    case LAUNCH_BOX_DECODE: return launch_box_decode(L.dec, st);
    }
    return hipErrorInvalidValue;
}

// Issues one record on a stream.  Diagnostic build, stamp_header != nullptr (the op VTI_STAMP_OP names; "": no header line): a
// launch_conv record is launched once, stamped; stem + layer 1 is stamped and then launched again.
static hipError_t issue(LaunchRec& L, hipStream_t st, const char* stamp_header = nullptr) {
#ifdef VTI_STAMPS
    if (stamp_header && (L.fn == LAUNCH_CONV || L.fn == LAUNCH_STEM_L1)) {
        if (L.fn == LAUNCH_STEM_L1) fprintf(stderr, "[stamps] stem + layer 1: 1: patch staged, 2: stem done, 3: layer-1 MFMAs done, 12: end\n");
        if (stamped_launch(L.conv, launch_workgroups(L), L.fn == LAUNCH_CONV && L.conv.pk != 0, st, *stamp_header ? stamp_header : nullptr,
                           [&] { return launch_record(L, st); }) && L.fn == LAUNCH_CONV)
            return hipSuccess;
    }
#endif
    return launch_record(L, st);
}

// what names an op in a launch error
static const char* launch_what(const LaunchRec& L) {
    switch (L.fn) {
    case LAUNCH_STEM_L1: return "stem + layer 1";
    case LAUNCH_POOL: return "sppf pool";
    case LAUNCH_UP2: return "upsample2x";
    case LAUNCH_DECODE: return "decode";
    case LAUNCH_BOX_DECODE: return "box decode";
    default: return L.name;
    }
}

// One op of the plan (no OP_FORK / OP_JOIN) on a stream: its launch record into L, then the launch.  The body of vti_forward's
// loop, and all that vti_debug_run_op launches.
static int32_t run_op(vti_ctx* c, const Op& op, int32_t B, int32_t swap_rb, const Bindings& bind, hipStream_t st, LaunchRec& L) {
    const Plan& P = c->plan;
    const RunOptions& run = c->opt.run;
    if (const char* e = fill_launch(P, op, B, swap_rb, run, bind, L)) return fail(c, VTI_ERR_UNSUPPORTED, e);
    const bool stamp = L.name && run.stamp_op == L.name;        // diagnostic build only
    VTI_HIP(c, issue(L, st, stamp ? ("[stamps] op " + op_label(P, op)).c_str() : nullptr), launch_what(L));
    return VTI_OK;
}

static int32_t forward_impl(vti_ctx* c, const uint8_t* input, int32_t B, int32_t swap_rb, float* pred, void* proto, float* best, void* stream);

int32_t vti_forward(vti_ctx* c, const uint8_t* input, int32_t B, int32_t swap_rb, float* pred, void* proto, void* stream) {
    return forward_impl(c, input, B, swap_rb, pred, proto, nullptr, stream);
}

int32_t vti_forward_scored(vti_ctx* c, const uint8_t* input, int32_t B, int32_t swap_rb, float* pred, void* proto, float* anchor_best,
                           void* stream) {
    if (!anchor_best) return fail(c, VTI_ERR_ARG, "vti_forward_scored: null pointer");
    return forward_impl(c, input, B, swap_rb, pred, proto, anchor_best, stream);
}

static int32_t forward_impl(vti_ctx* c, const uint8_t* input, int32_t B, int32_t swap_rb, float* pred, void* proto, float* best, void* stream) {
    int32_t rc = check_ready(c, B, "vti_forward");
    if (rc) return rc;
    if (!input || !pred || !proto) return fail(c, VTI_ERR_ARG, "vti_forward: null pointer");
    if (B == 0) return VTI_OK;
    const Plan& P = c->plan;
    hipStream_t main_st = (hipStream_t)stream;
    const RunOptions& run = c->opt.run;
    if (run.list_ops) {        // developer aid: launch order, to label a kernel trace
        int i = 0;
        for (const Op& op : P.ops)
            if (op.kind != OP_FORK && op.kind != OP_JOIN) fprintf(stderr, "[op %2d] lane %d %s\n", i++, op.lane, op_label(P, op).c_str());
    }
    const Bindings bind = bindings_of(c, input, pred, proto, best);
    LaunchRec L;
    for (const Op& op : P.ops) {
        if (op.kind == OP_FORK || op.kind == OP_JOIN) {       // a side lane starts after / is waited for by the caller's stream
            if (!c->multi_stream) continue;
            const bool fork = op.kind == OP_FORK;
            hipEvent_t ev = fork ? c->ev_fork[op.lane] : c->ev_join[op.lane];
            VTI_HIP(c, hipEventRecord(ev, fork ? main_st : c->side[op.lane]), fork ? "fork record" : "join record");
            VTI_HIP(c, hipStreamWaitEvent(fork ? c->side[op.lane] : main_st, ev, 0), fork ? "fork wait" : "join wait");
            continue;
        }
        VTI_TRY(run_op(c, op, B, swap_rb, bind, (c->multi_stream && op.lane > 0) ? c->side[op.lane] : main_st, L));
    }
    // a plan whose class towers do not write pred themselves (VTI_NO_SCATTER ...) derives the pairs from the finished rows
    if (best && !P.pred_scatter)
        VTI_HIP(c, launch_anchor_best(pred, B, P.num_anchors, P.desc.nc, P.desc.nm, best, main_st), "anchor pairs");
    c->last_input = input;
    c->last_proto = proto;
    return VTI_OK;
}

// vti_nms (best == null: the candidate filter scans the class scores) and vti_nms_scored (the (max, class) pairs beside pred)
static int32_t nms_impl(vti_ctx* c, const char* fn, bool scored, const float* pred, const float* best, int32_t B, float conf,
                        double iou, int32_t max_det, int32_t agnostic, float* dets, int32_t* counts, void* stream) {
    if (!c) return VTI_ERR_ARG;
    if (B < 0 || B > c->plan.desc.max_batch) return fail(c, VTI_ERR_ARG, std::string(fn) + ": B out of range");
    if (!c->ws) return fail(c, VTI_ERR_STATE, std::string(fn) + ": workspace not set");
    if (!pred || (scored && !best) || !dets || !counts || max_det < 1) return fail(c, VTI_ERR_ARG, std::string(fn) + ": bad argument");
    if (int32_t drc = check_device(c, fn)) return drc;
    VTI_HIP(c, launch_nms(pred, best, B, c->plan.num_anchors, c->plan.desc.nc, c->plan.desc.nm, conf, iou, max_det, agnostic,
                          dets, counts, c->ws + c->act_bytes, (hipStream_t)stream, c->nms_table), "nms kernel");
    return VTI_OK;
}

// ---- the NMS table: settings per frame and Ultralytics' `classes` filter (host only) ---------------------------------------------
int64_t vti_nms_table_bytes(int32_t n_rows) {
    if (n_rows < 1 || n_rows > VTI_NMS_TABLE_MAX_ROWS) return 0;
    return (int64_t)sizeof(NmsTableHeader) + (int64_t)n_rows * (int64_t)sizeof(NmsRow);
}

// What is wrong with the settings of one packed row (nullptr: nothing); the checks vti_pack_nms_table makes of the struct's numbers.
static const char* nms_settings_error(float conf, double iou, int32_t max_det, int32_t agnostic) {
    if (!(conf >= 0.0f && conf <= 1.0f)) return "conf must be finite and in [0, 1]";
    if (!(iou >= 0.0 && iou <= 1.0)) return "iou must be finite and in [0, 1]";
    if (max_det < 1) return "max_det must be >= 1";
    if (agnostic != 0 && agnostic != 1) return "agnostic must be 0 or 1";
    return nullptr;
}

int32_t vti_pack_nms_table(vti_ctx* c, const vti_nms_params* params, int32_t n_rows, void* host_table, size_t nbytes) {
    const char* fn = "vti_pack_nms_table";
    if (!c) return fail(c, VTI_ERR_ARG, "vti_pack_nms_table: null ctx (the table is packed for its class count)");
    if (!params || !host_table) return refuse(c, fn, "null params or table");
    const int64_t need = vti_nms_table_bytes(n_rows);
    if (!need) return refuse(c, fn, "n_rows must be in 1 .. VTI_NMS_TABLE_MAX_ROWS");
    if ((int64_t)nbytes < need) return refuse(c, fn, "table smaller than vti_nms_table_bytes()");
    const int nc = c->plan.desc.nc;
    char msg[200];
    for (int32_t k = 0; k < n_rows; ++k) {
        const vti_nms_params& p = params[k];
        const char* e = nms_settings_error(p.conf, p.iou, p.max_det, p.agnostic);
        if (!e && p.n_classes < 0) e = "n_classes must be >= 0";
        if (!e && p.n_classes > 0 && !p.classes) e = "classes is NULL but n_classes > 0";
        if (e) {
            snprintf(msg, sizeof msg, "%s: row %d: %s", fn, k, e);
            return fail(c, VTI_ERR_ARG, msg);
        }
        for (int32_t i = 0; i < p.n_classes; ++i)
            if (p.classes[i] < 0 || p.classes[i] >= nc) {
                snprintf(msg, sizeof msg, "%s: row %d: classes[%d] = %d is outside [0, %d)", fn, k, i, p.classes[i], nc);
                return fail(c, VTI_ERR_ARG, msg);
            }
        if (p.n_classes > 0 && nc > VTI_NMS_TABLE_MAX_CLASSES) {
            snprintf(msg, sizeof msg, "%s: row %d: a class set needs a model of at most %d classes (this one has %d)", fn, k,
                     VTI_NMS_TABLE_MAX_CLASSES, nc);
            return fail(c, VTI_ERR_UNSUPPORTED, msg);
        }
    }
    memset(host_table, 0, (size_t)need);
    NmsTableHeader h = {};
    h.magic = kNmsTableMagic; h.n_rows = n_rows; h.nc = nc; h.mask_words = kNmsMaskWords;
    memcpy(host_table, &h, sizeof h);
    for (int32_t k = 0; k < n_rows; ++k) {
        const vti_nms_params& p = params[k];
        NmsRow r = {};
        r.conf = p.conf; r.max_det = p.max_det; r.iou = p.iou; r.agnostic = p.agnostic;
        int named = 0;
        for (int32_t i = 0; i < p.n_classes; ++i) {
            unsigned& w = r.mask[p.classes[i] >> 5];
            const unsigned bit = 1u << (p.classes[i] & 31);
            named += !(w & bit);
            w |= bit;
        }
        if (named > 0 && named < nc) r.filter = 1;
        else memset(r.mask, 0, sizeof r.mask);      // a set that names every class is no set: the same bytes as n_classes = 0
        memcpy((char*)host_table + sizeof h + (size_t)k * sizeof r, &r, sizeof r);
    }
    return VTI_OK;
}

int32_t vti_set_nms_table(vti_ctx* c, const void* host_table, const void* dev_table, int32_t n_rows, const int32_t* dev_row_of_frame) {
    const char* fn = "vti_set_nms_table";
    if (!c) return VTI_ERR_ARG;
    if (!host_table) {          // clear: every NMS of the ctx takes its call's own arguments again
        c->nms_host.clear();
        c->nms_table = NmsTable{};
        return VTI_OK;
    }
    if (!dev_table || ((uintptr_t)dev_table & 15)) return refuse(c, fn, "dev_table is required and must be 16-byte aligned");
    if ((uintptr_t)dev_row_of_frame & 3) return refuse(c, fn, "dev_row_of_frame must be 4-byte aligned");
    const int64_t need = vti_nms_table_bytes(n_rows);
    if (!need) return refuse(c, fn, "n_rows must be in 1 .. VTI_NMS_TABLE_MAX_ROWS");
    NmsTableHeader h;
    memcpy(&h, host_table, sizeof h);
    if (h.magic != kNmsTableMagic || h.mask_words != kNmsMaskWords) return refuse(c, fn, "host_table is not a table of vti_pack_nms_table");
    if (h.n_rows != n_rows) return refuse(c, fn, "n_rows is not the row count host_table was packed with");
    const int nc = c->plan.desc.nc;
    if (h.nc != nc) return refuse(c, fn, "host_table was packed for a model with another class count");
    char msg[200];
    for (int32_t k = 0; k < n_rows; ++k) {
        NmsRow r;
        memcpy(&r, (const char*)host_table + sizeof h + (size_t)k * sizeof r, sizeof r);
        const char* e = nms_settings_error(r.conf, r.iou, r.max_det, r.agnostic);
        if (!e && (r.filter != 0 && r.filter != 1)) e = "damaged class-set flag";
        if (!e && r.filter && nc > VTI_NMS_TABLE_MAX_CLASSES) e = "a class set on a model above VTI_NMS_TABLE_MAX_CLASSES classes";
        int named = 0;
        for (int j = 0; !e && j < 32 * kNmsMaskWords; ++j)
            if ((r.mask[j >> 5] >> (j & 31)) & 1u) {
                if (j >= nc) e = "a class outside [0, nc) in the class set";
                ++named;
            }
        if (!e && (r.filter ? (named < 1 || named >= nc) : named != 0)) e = "class-set flag and mask disagree";
        if (e) {
            snprintf(msg, sizeof msg, "%s: row %d: %s", fn, k, e);
            return fail(c, VTI_ERR_ARG, msg);
        }
    }
    c->nms_host.assign((const unsigned char*)host_table, (const unsigned char*)host_table + need);
    c->nms_table.rows = (const NmsRow*)((const char*)dev_table + sizeof(NmsTableHeader));
    c->nms_table.row_of_frame = dev_row_of_frame;
    c->nms_table.n_rows = n_rows;
    return VTI_OK;
}

int32_t vti_nms_scored(vti_ctx* c, const float* pred, const float* anchor_best, int32_t B, float conf, double iou, int32_t max_det,
                       int32_t agnostic, float* dets, int32_t* counts, void* stream) {
    return nms_impl(c, "vti_nms_scored", true, pred, anchor_best, B, conf, iou, max_det, agnostic, dets, counts, stream);
}

int32_t vti_nms(vti_ctx* c, const float* pred, int32_t B, float conf, double iou, int32_t max_det, int32_t agnostic,
                float* dets, int32_t* counts, void* stream) {
    return nms_impl(c, "vti_nms", false, pred, nullptr, B, conf, iou, max_det, agnostic, dets, counts, stream);
}

int32_t vti_masks(vti_ctx* c, const float* dets, const int32_t* counts, const void* proto, int32_t B, int32_t max_det,
                  int32_t mode, int32_t packing, uint8_t* masks, int32_t capacity, int32_t* offsets, void* stream) {
    if (!c || !dets || !counts || !proto || !offsets || B < 0 || max_det < 1 || capacity < 0 || (capacity && !masks))
        return fail(c, VTI_ERR_ARG, "vti_masks: bad argument");
    if ((mode != VTI_MASK_LOGIT && mode != VTI_MASK_SIGMOID) || (packing != VTI_PACK_U8 && packing != VTI_PACK_BITS))
        return fail(c, VTI_ERR_ARG, "vti_masks: bad mode/packing");
    const vti_desc& d = c->plan.desc;
    if (!c->ws) return fail(c, VTI_ERR_STATE, "vti_masks: workspace not set");
    if (B > d.max_batch) return fail(c, VTI_ERR_ARG, "vti_masks: B out of range");
    if (capacity > d.max_batch * kMaskSlotsPerFrame)
        return fail(c, VTI_ERR_UNSUPPORTED, "vti_masks: capacity above max_batch*512 instances per call");
    void* mws = c->ws + c->act_bytes + nms_workspace_bytes(d.max_batch, c->plan.num_anchors);
    if (int32_t drc = check_device(c, "vti_masks")) return drc;
    VTI_HIP(c, launch_masks(d.dtype, dets, counts, proto, B, max_det, d.nm, d.H / 4, d.W / 4, d.H, d.W, mode, packing, masks,
                            capacity, offsets, mws, (hipStream_t)stream, c->opt.run.mask_wgs_per_cu), "mask kernel");
    return VTI_OK;
}

int32_t vti_mask_native_layout(const vti_ctx* c, int32_t H0, int32_t W0, int32_t packing, int32_t out[6]) {
    vti_ctx* m = const_cast<vti_ctx*>(c);     // the error message slot
    if (!c || !out) return fail(m, VTI_ERR_ARG, "vti_mask_native_layout: bad argument");
    if (packing != VTI_PACK_U8 && packing != VTI_PACK_BITS) return fail(m, VTI_ERR_ARG, "vti_mask_native_layout: bad packing");
    const vti_desc& d = c->plan.desc;
    if (native_mask_layout(d.H / 4, d.W / 4, H0, W0, packing, out))
        return fail(m, VTI_ERR_ARG, "vti_mask_native_layout: bad frame size (H0, W0 >= 1, slot below 2 GiB)");
    return VTI_OK;
}

int32_t vti_masks_native(vti_ctx* c, const float* dets, const float* xyxy, const int32_t* counts, const void* proto, int32_t B,
                         int32_t max_det, int32_t H0, int32_t W0, int32_t mode, int32_t packing, uint8_t* masks, int32_t capacity,
                         int32_t* offsets, void* stream) {
    if (!c || !dets || !xyxy || !counts || !proto || !offsets || B < 0 || max_det < 1 || capacity < 0 || (capacity && !masks))
        return fail(c, VTI_ERR_ARG, "vti_masks_native: bad argument");
    if ((mode != VTI_MASK_LOGIT && mode != VTI_MASK_SIGMOID) || (packing != VTI_PACK_U8 && packing != VTI_PACK_BITS))
        return fail(c, VTI_ERR_ARG, "vti_masks_native: bad mode/packing");
    const vti_desc& d = c->plan.desc;
    int lay[6];
    if (native_mask_layout(d.H / 4, d.W / 4, H0, W0, packing, lay)) return fail(c, VTI_ERR_ARG, "vti_masks_native: bad frame size");
    if (packing == VTI_PACK_BITS && capacity && ((uintptr_t)masks & 7))
        return fail(c, VTI_ERR_ARG, "vti_masks_native: bit-packed masks must be 8-byte aligned");
    if (!c->ws) return fail(c, VTI_ERR_STATE, "vti_masks_native: workspace not set");
    if (B > d.max_batch) return fail(c, VTI_ERR_ARG, "vti_masks_native: B out of range");
    if (capacity > d.max_batch * kMaskSlotsPerFrame)
        return fail(c, VTI_ERR_UNSUPPORTED, "vti_masks_native: capacity above max_batch*512 instances per call");
    if (d.nm != 32) return fail(c, VTI_ERR_UNSUPPORTED, "vti_masks_native: only nm == 32 prototypes");
    void* mws = c->ws + c->act_bytes + nms_workspace_bytes(d.max_batch, c->plan.num_anchors);
    if (int32_t drc = check_device(c, "vti_masks_native")) return drc;
    VTI_HIP(c, launch_masks_native(d.dtype, dets, xyxy, counts, proto, B, max_det, d.H / 4, d.W / 4, H0, W0, mode, packing, masks,
                                   capacity, offsets, mws, (hipStream_t)stream), "native mask kernel");
    return VTI_OK;
}

int32_t vti_scale_boxes(vti_ctx* c, const float* dets, const int32_t* counts, int32_t B, int32_t max_det, int32_t H0,
                        int32_t W0, float* xyxy, void* stream) {
    if (!c || !dets || !counts || !xyxy || B < 0 || max_det < 1 || H0 < 1 || W0 < 1)
        return fail(c, VTI_ERR_ARG, "vti_scale_boxes: bad argument");
    const vti_desc& d = c->plan.desc;
    if (int32_t drc = check_device(c, "vti_scale_boxes")) return drc;
    VTI_HIP(c, launch_scale_boxes(dets, counts, B, max_det, d.nm, d.H, d.W, H0, W0, nullptr, xyxy, (hipStream_t)stream), "scale_boxes kernel");
    return VTI_OK;
}

int32_t vti_scale_boxes_frames(vti_ctx* c, const float* dets, const int32_t* counts, const void* host_table, const void* dev_table,
                               int32_t B, int32_t max_det, float* xyxy, void* stream) {
    return scale_boxes_table<FrameKind>(c, dets, counts, host_table, dev_table, B, max_det, xyxy, stream);
}
int32_t vti_scale_boxes_windows(vti_ctx* c, const float* dets, const int32_t* counts, const void* host_table, const void* dev_table,
                                int32_t B, int32_t max_det, float* xyxy, void* stream) {
    return scale_boxes_table<WindowKind>(c, dets, counts, host_table, dev_table, B, max_det, xyxy, stream);
}

int32_t vti_predict(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, int32_t swap_rb, float conf,
                    double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode, int32_t packing,
                    uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts, uint8_t* masks,
                    int32_t capacity, int32_t* offsets, float* xyxy, void* stream) {
    int32_t rc = check_ready(c, B, "vti_predict");
    if (rc) return rc;
    const vti_desc& d = c->plan.desc;
    const uint8_t* input = frames;
    if (H0 != d.H || W0 != d.W) {
        if (!input_scratch) return fail(c, VTI_ERR_ARG, "vti_predict: frames need letterboxing but dev_input_scratch is NULL");
        rc = vti_letterbox(c, frames, B, H0, W0, input_scratch, stream);
        if (rc) return rc;
        input = input_scratch;
    }
    // the (max score, class) pairs travel from the class towers to the NMS filter through the library's own workspace
    float* best = c->ws ? nms_workspace_best(c->ws + c->act_bytes, d.max_batch, c->plan.num_anchors) : nullptr;
    if (!best) return fail(c, VTI_ERR_STATE, "vti_predict: workspace not set");
    if ((rc = vti_forward_scored(c, input, B, swap_rb, pred, proto, best, stream))) return rc;
    if ((rc = vti_nms_scored(c, pred, best, B, conf, iou, max_det, agnostic, dets, counts, stream))) return rc;
    if (mask_mode & VTI_MASK_NATIVE) {     // frame-resolution masks need the frame-px boxes first
        if (!xyxy) return fail(c, VTI_ERR_ARG, "vti_predict: VTI_MASK_NATIVE needs dev_xyxy");
        if ((rc = vti_scale_boxes(c, dets, counts, B, max_det, H0, W0, xyxy, stream))) return rc;
        return vti_masks_native(c, dets, xyxy, counts, proto, B, max_det, H0, W0, mask_mode & ~VTI_MASK_NATIVE, packing, masks,
                                capacity, offsets, stream);
    }
    if ((rc = vti_masks(c, dets, counts, proto, B, max_det, mask_mode, packing, masks, capacity, offsets, stream))) return rc;
    if (xyxy && (rc = vti_scale_boxes(c, dets, counts, B, max_det, H0, W0, xyxy, stream))) return rc;
    return VTI_OK;
}

// Canvas-size masks for frames of differing sizes; the frame-resolution ones are vti_predict_frames_native's.
int32_t vti_predict_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                           int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode,
                           int32_t packing, uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts,
                           uint8_t* masks, int32_t capacity, int32_t* offsets, float* xyxy, void* stream) {
    const char* fn = "vti_predict_frames";
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, B, h));
    if (mask_mode & VTI_MASK_NATIVE) return refuse(c, fn, "VTI_MASK_NATIVE needs frames of one size (vti_predict)", VTI_ERR_UNSUPPORTED);
    VTI_TRY(predict_table_head<FrameKind>(fn, c, frames, host_table, dev_table, B, swap_rb, conf, iou, max_det, agnostic, input_scratch,
                                          pred, proto, dets, counts, xyxy, stream));
    VTI_TRY(vti_masks(c, dets, counts, proto, B, max_det, mask_mode, packing, masks, capacity, offsets, stream));
    return xyxy ? vti_scale_boxes_frames(c, dets, counts, host_table, dev_table, B, max_det, xyxy, stream) : VTI_OK;
}

// ---- frame-resolution masks for frames of differing sizes, and for a window of each: the ragged mask buffer ------------------
int64_t vti_mask_native_frames_bytes(const vti_ctx* c, const void* host_table, int32_t max_det) {
    return mask_native_table_bytes<FrameKind>(c, host_table, max_det);
}
int64_t vti_mask_native_windows_bytes(const vti_ctx* c, const void* host_table, int32_t max_det) {
    return mask_native_table_bytes<WindowKind>(c, host_table, max_det);
}

int32_t vti_masks_native_frames(vti_ctx* c, const float* dets, const float* xyxy, const int32_t* counts, const void* proto,
                                const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t mode, int32_t packing,
                                uint8_t* masks, int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases, void* stream) {
    return masks_native_table<FrameKind>(c, dets, xyxy, counts, proto, host_table, dev_table, B, max_det, mode, packing, masks,
                                         capacity_bytes, offsets, mask_bases, stream);
}
int32_t vti_masks_native_windows(vti_ctx* c, const float* dets, const int32_t* counts, const void* proto, const void* host_table,
                                 const void* dev_table, int32_t B, int32_t max_det, int32_t mode, int32_t packing, uint8_t* masks,
                                 int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases, void* stream) {
    return masks_native_table<WindowKind>(c, dets, nullptr, counts, proto, host_table, dev_table, B, max_det, mode, packing, masks,
                                          capacity_bytes, offsets, mask_bases, stream);
}

int32_t vti_predict_frames_native(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                                  int32_t swap_rb, float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode,
                                  int32_t packing, uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts,
                                  uint8_t* masks, int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases, float* xyxy,
                                  void* stream) {
    return predict_table_native<FrameKind>(c, frames, host_table, dev_table, B, swap_rb, conf, iou, max_det, agnostic, mask_mode, packing,
                                           input_scratch, pred, proto, dets, counts, masks, capacity_bytes, offsets, mask_bases, xyxy,
                                           stream);
}
int32_t vti_predict_windows(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B, int32_t swap_rb,
                            float conf, double iou, int32_t max_det, int32_t agnostic, int32_t mask_mode, int32_t packing,
                            uint8_t* input_scratch, float* pred, void* proto, float* dets, int32_t* counts, uint8_t* masks,
                            int64_t capacity_bytes, int32_t* offsets, int64_t* mask_bases, float* xyxy, void* stream) {
    return predict_table_native<WindowKind>(c, frames, host_table, dev_table, B, swap_rb, conf, iou, max_det, agnostic, mask_mode, packing,
                                            input_scratch, pred, proto, dets, counts, masks, capacity_bytes, offsets, mask_bases, xyxy,
                                            stream);
}

int32_t vti_mask_to_frame(vti_ctx* c, const uint8_t* masks, int32_t n, int32_t H, int32_t W, int32_t H0, int32_t W0,
                          uint8_t* bitmaps, int32_t* nonzero, void* stream) {
    if (!c || n < 0 || H < 1 || W < 1 || H0 < 1 || W0 < 1 || (n && (!masks || !bitmaps || !nonzero)))
        return fail(c, VTI_ERR_ARG, "vti_mask_to_frame: bad argument");
    if (int32_t drc = check_device(c, "vti_mask_to_frame")) return drc;
    VTI_HIP(c, launch_mask_to_frame(masks, n, H, W, H0, W0, bitmaps, nonzero, (hipStream_t)stream), "mask_to_frame kernel");
    return VTI_OK;
}

int32_t vti_union_envelope(vti_ctx* c, const uint8_t* bitmaps, const int32_t* select, int32_t nsel, int32_t H0, int32_t W0,
                           uint8_t* uni, int32_t* envelope, void* stream) {
    if (!c || nsel < 0 || H0 < 1 || W0 < 1 || !uni || !envelope || (nsel && (!bitmaps || !select)))
        return fail(c, VTI_ERR_ARG, "vti_union_envelope: bad argument");
    if (int32_t drc = check_device(c, "vti_union_envelope")) return drc;
    VTI_HIP(c, launch_union_envelope(bitmaps, select, nsel, H0, W0, uni, envelope, (hipStream_t)stream), "union_envelope kernel");
    return VTI_OK;
}

int32_t vti_mask_stats(vti_ctx* c, const uint8_t* bitmaps, int32_t n, int32_t H0, int32_t W0, int64_t* stats, void* stream) {
    if (!c || n < 0 || H0 < 1 || W0 < 1 || (n && (!bitmaps || !stats)))
        return fail(c, VTI_ERR_ARG, "vti_mask_stats: bad argument");
    if (int32_t drc = check_device(c, "vti_mask_stats")) return drc;
    VTI_HIP(c, launch_mask_stats(bitmaps, n, H0, W0, (long long*)stats, (hipStream_t)stream), "mask_stats kernel");
    return VTI_OK;
}

int32_t vti_mask_stats_bits(vti_ctx* c, const uint8_t* masks_bits, int32_t n, const int32_t* n_live, int32_t H, int32_t W,
                            int32_t H0, int32_t W0, int64_t* stats, void* stream) {
    if (n < 0 || H < 1 || W < 32 || (W & 31) || H0 < 1 || W0 < 1 || (n && (!masks_bits || !stats)))
        return fail(c, VTI_ERR_ARG, "vti_mask_stats_bits: bad argument (W must be a multiple of 32)");
    if (int32_t drc = check_device(c, "vti_mask_stats_bits")) return drc;
    VTI_HIP(c, launch_mask_stats_bits(masks_bits, n, n_live, H, W, H0, W0, (long long*)stats, (hipStream_t)stream), "mask_stats_bits kernel");
    return VTI_OK;
}

int32_t vti_envelope_bits(vti_ctx* c, const uint8_t* masks_bits, const int32_t* offsets, const float* dets, int32_t B,
                          int32_t max_det, int32_t capacity, int32_t cls, int32_t H0, int32_t W0, int32_t* envelope, void* stream) {
    if (!c || B < 0 || max_det < 1 || capacity < 0 || H0 < 1 || W0 < 1 || (B && (!masks_bits || !offsets || !dets || !envelope)))
        return fail(c, VTI_ERR_ARG, "vti_envelope_bits: bad argument");
    const vti_desc& d = c->plan.desc;
    if (int32_t drc = check_device(c, "vti_envelope_bits")) return drc;
    VTI_HIP(c, launch_envelope_bits(masks_bits, offsets, dets, B, max_det, d.nm, capacity, cls, d.H, d.W, H0, W0, envelope,
                                    (hipStream_t)stream), "envelope_bits kernel");
    return VTI_OK;
}

int32_t vti_pixels_to_world(vti_ctx* c, const double* uv, int32_t n, const double* K, const double* dist, const double* R,
                            const double* t, double* xyz, int32_t* valid, void* stream) {
    if (n < 0 || !K || !dist || !R || !t || (n && (!uv || !xyz || !valid)))
        return fail(c, VTI_ERR_ARG, "vti_pixels_to_world: bad argument");
    VTI_HIP(c, launch_pixels_to_world(uv, n, K, dist, R, t, xyz, valid, (hipStream_t)stream), "pixels_to_world kernel");
    return VTI_OK;
}

int32_t vti_kmeans1d2(vti_ctx* c, const double* values, const int32_t* counts, int32_t B, int32_t max_n, int32_t max_iters,
                      int32_t* labels, double* centers, void* stream) {
    if (B < 0 || max_n < 1 || max_n > 1024 || max_iters < 0 || (B && (!values || !counts || !labels || !centers)))
        return fail(c, VTI_ERR_ARG, "vti_kmeans1d2: bad argument (max_n <= 1024)");
    VTI_HIP(c, launch_kmeans1d2(values, counts, B, max_n, max_iters, labels, centers, (hipStream_t)stream), "kmeans1d2 kernel");
    return VTI_OK;
}

int64_t vti_measure_scratch_bytes(const vti_ctx* c, int32_t B, int32_t capacity, int32_t W0) {
    if (!c || B < 0 || capacity < 0 || W0 < 1) return 0;
    size_t off[3], total;
    measure_scratch_layout(B, capacity, W0, off, total);
    return (int64_t)total;
}

// ---- argument checks that several entry points make: each returns 0, or refuse()'s status with the message "<fn>: <what>" -----
// Mask rows are read with 16-byte loads, native (frame-size) rows with 8-byte loads.
static int32_t mask_align_check(const char* fn, vti_ctx* c, const uint8_t* masks, int32_t native) {
    if ((uintptr_t)masks & (native ? 7 : 15))
        return refuse(c, fn, native ? "native masks must be 8-byte aligned" : "masks must be 16-byte aligned");
    return VTI_OK;
}

// The caller's scratch: a 256-byte aligned pointer (`need_ptr` = 0: not looked at) to at least `need` bytes, the answer of `query`.
static int32_t scratch_check(const char* fn, vti_ctx* c, const void* scratch, size_t scratch_bytes, int64_t need, const char* query,
                             bool need_ptr = true) {
    if (need_ptr && (!scratch || ((uintptr_t)scratch & 255))) return refuse(c, fn, "scratch must be a 256-byte aligned device pointer");
    if ((int64_t)scratch_bytes < need) return refuse(c, fn, (std::string("scratch smaller than ") + query).c_str());
    return VTI_OK;
}

// What both measurement families check of the output set, the result rows and the scratch.  `limit`: the status for a max_det or a
// letterbox size beyond what the kernels serve (include/vti.h: VTI_ERR_UNSUPPORTED in the measure family, VTI_ERR_ARG in the checker).
static int32_t measure_args_check(const char* fn, vti_ctx* c, int32_t limit, const OutputSet& o, int32_t H0, int32_t W0,
                                  const MeasureResult& r) {
    if (o.B < 0 || o.max_det < 1 || o.capacity < 0 || H0 < 1 || W0 < 1 || (o.native != 0 && o.native != 1))
        return refuse(c, fn, "bad shape (B, capacity >= 0; max_det, H0, W0 >= 1; native 0 or 1)");
    if (o.max_det > VTI_MEASURE_MAX_DET) return refuse(c, fn, "max_det above VTI_MEASURE_MAX_DET", limit);
    if (o.B && (!o.dets || !o.xyxy || !o.counts || !o.offsets || !r.frame_f64 || !r.frame_i32 || (o.capacity && !o.masks)))
        return refuse(c, fn, "null pointer");
    VTI_TRY(mask_align_check(fn, c, o.capacity ? o.masks : nullptr, o.native));
    if (!o.native && (size_t)(4 * c->plan.desc.W + 2 * c->plan.desc.H) * 4 > 60 * 1024)
        return refuse(c, fn, "letterbox size too large for the resize tables", limit);
    if ((int64_t)o.B * W0 > INT32_MAX) return refuse(c, fn, "B * W0 out of range");
    return scratch_check(fn, c, r.scratch, r.scratch_bytes, vti_measure_scratch_bytes(c, o.B, o.capacity, W0),
                         "vti_measure_scratch_bytes()", o.B != 0);
}

// The camera table and the per-frame camera index of the table forms.
static int32_t camera_table_check(const char* fn, vti_ctx* c, const CameraChoice& cams) {
    if (!c || !cams.table || !cams.cam_of_frame) return refuse(c, fn, "null ctx, camera table or camera index");
    if (cams.n_cams < 1) return refuse(c, fn, "n_cams must be >= 1");
    if (((uintptr_t)cams.table & 15) || ((uintptr_t)cams.cam_of_frame & 3))
        return refuse(c, fn, "the camera table must be 16-byte aligned, the index 4-byte aligned");
    return VTI_OK;
}

}  // extern "C": the code of the two measurement families is a template over what differs between them

// ---- vti_measure* (process_frame's record) and vti_measure_checker* (the stitch-distance checker's): one implementation -------
struct MeasureFamily {
    using Params = vti_measure_params;
    static constexpr auto error = measure_params_error;
    static constexpr auto pack = measure_pack_camera;
    static constexpr auto launch = launch_measure;
    static constexpr int32_t limit = VTI_ERR_UNSUPPORTED;
    static constexpr const char* one_size = "native masks need frames of one size (vti_measure_cameras)";
    static constexpr const char* kernels = "measure kernels";
};
struct CheckerFamily {
    using Params = vti_checker_params;
    static constexpr auto error = settings_error<vti_checker_params>;
    static constexpr auto pack = checker_pack;
    static constexpr auto launch = launch_measure_checker;
    static constexpr int32_t limit = VTI_ERR_ARG;
    static constexpr const char* one_size = "native masks need frames of one size (vti_measure_checker_cameras)";
    static constexpr const char* kernels = "measure_checker kernels";
};

// Exactly one of p and cams is given; with fs.rows (the rows of a device frame table, already checked against its host copy) fs.H0 and
// fs.W0 are the table's largest ones.  o.bases (with fs.rows and native = 1 only, the *_frames_native calls): the masks are
// vti_masks_native_frames' ragged rows.  Every check comes before the first HIP call.
template <class F>
static int32_t measure_impl(const char* fn, vti_ctx* c, const typename F::Params* p, const CameraChoice& cams, const OutputSet& o,
                            const FrameSizes& fs, const MeasureResult& r, void* stream) {
    if (fs.rows && o.native == 1 && !o.bases) return refuse(c, fn, F::one_size, VTI_ERR_UNSUPPORTED);
    if (o.bases && (o.capacity_bytes < 0 || ((uintptr_t)o.bases & 7)))
        return refuse(c, fn, "capacity_bytes must be >= 0, dev_mask_bases 8-byte aligned");
    if (p)
        if (const char* e = F::error(*p)) return refuse(c, fn, e);
    VTI_TRY(measure_args_check(fn, c, F::limit, o, fs.H0, fs.W0, r));
    if (o.B == 0) return VTI_OK;
    VTI_TRY(check_device(c, fn));
    const vti_desc& d = c->plan.desc;
    VTI_HIP(c, F::launch(p, cams, o, Canvas{d.nm, d.H, d.W}, fs, r, (hipStream_t)stream), F::kernels);
    return VTI_OK;
}

template <class F>
static int32_t measure_one(const char* fn, vti_ctx* c, const typename F::Params* p, const OutputSet& o, int32_t H0, int32_t W0,
                           const MeasureResult& r, void* stream) {
    if (!c || !p) return refuse(c, fn, "null ctx or params");
    return measure_impl<F>(fn, c, p, CameraChoice{}, o, FrameSizes{H0, W0, nullptr}, r, stream);
}

template <class F>
static int32_t pack_cameras(const char* fn, vti_ctx* c, const typename F::Params* params, int32_t n_cams, void* host_table,
                            size_t nbytes) {
    if (!params || n_cams < 1 || !host_table) return refuse(c, fn, "null list or table, or n_cams < 1");
    if ((int64_t)nbytes < vti_measure_cameras_bytes(n_cams)) return refuse(c, fn, "table smaller than vti_measure_cameras_bytes()");
    for (int32_t k = 0; k < n_cams; ++k)
        if (const char* e = F::error(params[k])) {
            char msg[200];
            snprintf(msg, sizeof msg, "camera %d: %s", k, e);
            return refuse(c, fn, msg);
        }
    for (int32_t k = 0; k < n_cams; ++k) F::pack(params[k], (char*)host_table + (size_t)k * measure_camera_row_bytes());
    return VTI_OK;
}

template <class F>
static int32_t measure_cameras(const char* fn, vti_ctx* c, const CameraChoice& cams, const OutputSet& o, int32_t H0, int32_t W0,
                               const MeasureResult& r, void* stream) {
    VTI_TRY(camera_table_check(fn, c, cams));
    return measure_impl<F>(fn, c, nullptr, cams, o, FrameSizes{H0, W0, nullptr}, r, stream);
}

template <class F>
static int32_t measure_frames(const char* fn, vti_ctx* c, const CameraChoice& cams, const OutputSet& o, const void* host_table,
                              const void* dev_table, const MeasureResult& r, void* stream) {
    VTI_TRY(camera_table_check(fn, c, cams));
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, o.B, h));
    return measure_impl<F>(fn, c, nullptr, cams, o, FrameSizes{h.max_H0, h.max_W0, frame_rows(dev_table)}, r, stream);
}

template <class F>
static int32_t measure_frames_native(const char* fn, vti_ctx* c, const CameraChoice& cams, const OutputSet& o, const void* host_table,
                                     const void* dev_table, const MeasureResult& r, void* stream) {
    VTI_TRY(camera_table_check(fn, c, cams));
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, o.B, h));
    if (!o.bases) return refuse(c, fn, "null dev_mask_bases");
    if (o.capacity_bytes < 0) return refuse(c, fn, "capacity_bytes must be >= 0");
    if (native_table_bytes<FrameRow>(host_table, c->plan.desc.H / 4, c->plan.desc.W / 4, 1, nullptr) < 0)
        return refuse(c, fn, "a frame of host_table has no native mask layout (slot below 2 GiB)");
    return measure_impl<F>(fn, c, nullptr, cams, o, FrameSizes{h.max_H0, h.max_W0, frame_rows(dev_table)}, r, stream);
}

extern "C" {

int64_t vti_measure_cameras_bytes(int32_t n_cams) {
    return n_cams < 1 ? 0 : (int64_t)n_cams * (int64_t)measure_camera_row_bytes();
}

int32_t vti_measure(vti_ctx* c, const vti_measure_params* p, const uint8_t* masks, int32_t native, const float* dets,
                    const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t B, int32_t max_det, int32_t capacity,
                    int32_t H0, int32_t W0, void* scratch, size_t scratch_bytes, double* frame_f64, int32_t* frame_i32,
                    double* stitch_f64, int32_t* stitch_i32, void* stream) {
    return measure_one<MeasureFamily>("vti_measure", c, p, {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
                                      H0, W0, {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_checker(vti_ctx* c, const vti_checker_params* p, const uint8_t* masks, int32_t native, const float* dets,
                            const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t B, int32_t max_det,
                            int32_t capacity, int32_t H0, int32_t W0, void* scratch, size_t scratch_bytes, double* frame_f64,
                            int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32, void* stream) {
    return measure_one<CheckerFamily>("vti_measure_checker", c, p,
                                      {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0}, H0, W0,
                                      {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_pack_cameras(vti_ctx* c, const vti_measure_params* params, int32_t n_cams, void* host_table, size_t nbytes) {
    return pack_cameras<MeasureFamily>("vti_measure_pack_cameras", c, params, n_cams, host_table, nbytes);
}

int32_t vti_checker_pack_cameras(vti_ctx* c, const vti_checker_params* params, int32_t n_cams, void* host_table, size_t nbytes) {
    return pack_cameras<CheckerFamily>("vti_checker_pack_cameras", c, params, n_cams, host_table, nbytes);
}

int32_t vti_measure_cameras(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                            int32_t native, const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t B,
                            int32_t max_det, int32_t capacity, int32_t H0, int32_t W0, void* scratch, size_t scratch_bytes,
                            double* frame_f64, int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32, void* stream) {
    return measure_cameras<MeasureFamily>("vti_measure_cameras", c, {cameras, n_cams, cam_of_frame},
                                          {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0}, H0, W0,
                                          {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_checker_cameras(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                    int32_t native, const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets,
                                    int32_t B, int32_t max_det, int32_t capacity, int32_t H0, int32_t W0, void* scratch,
                                    size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32,
                                    void* stream) {
    return measure_cameras<CheckerFamily>("vti_measure_checker_cameras", c, {cameras, n_cams, cam_of_frame},
                                          {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0}, H0, W0,
                                          {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_frames(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                           int32_t native, const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets,
                           const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t capacity, void* scratch,
                           size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32,
                           void* stream) {
    return measure_frames<MeasureFamily>("vti_measure_frames", c, {cameras, n_cams, cam_of_frame},
                                         {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0}, host_table,
                                         dev_table, {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_checker_frames(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                   int32_t native, const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets,
                                   const void* host_table, const void* dev_table, int32_t B, int32_t max_det, int32_t capacity,
                                   void* scratch, size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64,
                                   int32_t* stitch_i32, void* stream) {
    return measure_frames<CheckerFamily>("vti_measure_checker_frames", c, {cameras, n_cams, cam_of_frame},
                                         {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0}, host_table,
                                         dev_table, {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_frames_native(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                  const int64_t* mask_bases, int64_t capacity_bytes, const float* dets, const float* xyxy,
                                  const int32_t* counts, const int32_t* offsets, const void* host_table, const void* dev_table, int32_t B,
                                  int32_t max_det, int32_t capacity, void* scratch, size_t scratch_bytes, double* frame_f64,
                                  int32_t* frame_i32, double* stitch_f64, int32_t* stitch_i32, void* stream) {
    return measure_frames_native<MeasureFamily>(
        "vti_measure_frames_native", c, {cameras, n_cams, cam_of_frame},
        {masks, 1, dets, xyxy, counts, offsets, B, max_det, capacity, (const long long*)mask_bases, capacity_bytes}, host_table,
        dev_table, {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

int32_t vti_measure_checker_frames_native(vti_ctx* c, const void* cameras, int32_t n_cams, const int32_t* cam_of_frame,
                                          const uint8_t* masks, const int64_t* mask_bases, int64_t capacity_bytes, const float* dets,
                                          const float* xyxy, const int32_t* counts, const int32_t* offsets, const void* host_table,
                                          const void* dev_table, int32_t B, int32_t max_det, int32_t capacity, void* scratch,
                                          size_t scratch_bytes, double* frame_f64, int32_t* frame_i32, double* stitch_f64,
                                          int32_t* stitch_i32, void* stream) {
    return measure_frames_native<CheckerFamily>(
        "vti_measure_checker_frames_native", c, {cameras, n_cams, cam_of_frame},
        {masks, 1, dets, xyxy, counts, offsets, B, max_det, capacity, (const long long*)mask_bases, capacity_bytes}, host_table,
        dev_table, {scratch, scratch_bytes, frame_f64, frame_i32, stitch_f64, stitch_i32}, stream);
}

static bool poly_sizes_ok(int32_t H, int32_t W, int32_t row_bytes) {
    return H >= 1 && W >= 1 && H <= 16384 && W <= 16384 && (int64_t)H * W <= (int64_t)1 << 26 && row_bytes >= 1 &&
           (int64_t)row_bytes * 8 >= W;
}

int64_t vti_mask_polygons_scratch_bytes(const vti_ctx* c, int32_t H, int32_t W, int32_t row_bytes) {
    if (!c || !poly_sizes_ok(H, W, row_bytes)) return 0;
    PolyLayout L;
    mask_polygons_layout(H, W, row_bytes, L);
    return (int64_t)L.total;
}

int32_t vti_mask_polygons(vti_ctx* c, const uint8_t* masks, int32_t n, const int32_t* n_live, int32_t H, int32_t W, int32_t row_bytes,
                          int32_t H0, int32_t W0, int32_t strategy, void* scratch, size_t scratch_bytes, int32_t* offsets,
                          float* points, int64_t max_points, void* stream) {
    // every check comes before the first HIP call
    if (!c) return fail(c, VTI_ERR_ARG, "vti_mask_polygons: null ctx");
    if (n < 0 || !poly_sizes_ok(H, W, row_bytes) || H0 < 1 || W0 < 1 || max_points < 0)
        return fail(c, VTI_ERR_ARG, "vti_mask_polygons: bad size (n, max_points >= 0; 1 <= H, W <= 16384, H * W <= 2^26; "
                                    "row_bytes * 8 >= W; H0, W0 >= 1)");
    if (strategy != VTI_POLY_LARGEST && strategy != VTI_POLY_CONCAT)
        return fail(c, VTI_ERR_ARG, "vti_mask_polygons: strategy must be VTI_POLY_LARGEST or VTI_POLY_CONCAT");
    if (!offsets || (n && !masks) || (max_points && !points)) return fail(c, VTI_ERR_ARG, "vti_mask_polygons: null pointer");
    VTI_TRY(scratch_check("vti_mask_polygons", c, scratch, scratch_bytes, vti_mask_polygons_scratch_bytes(c, H, W, row_bytes),
                          "vti_mask_polygons_scratch_bytes()"));
    VTI_TRY(check_device(c, "vti_mask_polygons"));
    VTI_HIP(c, launch_mask_polygons(masks, n, n_live, H, W, row_bytes, H0, W0, strategy, scratch, offsets, points,
                                    (long long)max_points, (hipStream_t)stream), "mask_polygons kernels");
    return VTI_OK;
}

// ---- the polygons of a batch whose frames differ in size: vti_mask_polygons on the slots of a frame table -------------------------
// The scratch layout for the frames of a validated host table: the canvas for letterbox masks, else every frame's own size.  Returns
// the first frame vti_mask_polygons' size limit refuses (native only; the table allows more), or -1.
static int32_t poly_frames_layout(const vti_ctx* c, const void* host_table, const FrameTableHeader& h, int32_t native, PolyLayout& L) {
    if (!native) {
        mask_polygons_layout(c->plan.desc.H, c->plan.desc.W, c->plan.desc.W / 8, L);
        return -1;
    }
    std::vector<int> H0(h.B), W0(h.B);
    for (int32_t b = 0; b < h.B; ++b) {
        const FrameRow r = table_row(host_table, b);
        if (!poly_sizes_ok(r.H0, r.W0, 8 * ((r.W0 + 63) / 64))) return b;
        H0[b] = r.H0; W0[b] = r.W0;
    }
    mask_polygons_layout_frames(H0.data(), W0.data(), h.B, L);
    return -1;
}

int64_t vti_mask_polygons_frames_scratch_bytes(const vti_ctx* c, const void* host_table, int32_t native) {
    if (!c || !host_table || (native != 0 && native != 1)) return 0;
    FrameTableHeader h;
    int32_t frame;
    if (!table_problem<FrameKind>(c, host_table, -1, h, frame).empty() || h.B > c->plan.desc.max_batch) return 0;
    PolyLayout L;
    if (!poly_sizes_ok(h.H, h.W, h.W / 8) || poly_frames_layout(c, host_table, h, native, L) >= 0) return 0;
    return (int64_t)L.total;
}

int32_t vti_mask_polygons_frames(vti_ctx* c, const uint8_t* masks, int32_t native, const int64_t* mask_bases, int64_t capacity_bytes,
                                 const int32_t* offsets, const void* host_table, const void* dev_table, int32_t B, int32_t capacity,
                                 int32_t strategy, void* scratch, size_t scratch_bytes, int32_t* point_offsets, float* points,
                                 int64_t max_points, void* stream) {
    const char* fn = "vti_mask_polygons_frames";
    // every check comes before the first HIP call
    if (!c) return refuse(c, fn, "null ctx");
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, B, h));
    if (B > c->plan.desc.max_batch) return refuse(c, fn, "B above max_batch");
    if (native != 0 && native != 1) return refuse(c, fn, "native must be 0 or 1");
    if (!native && mask_bases) return refuse(c, fn, "dev_mask_bases must be NULL with native = 0 (letterbox masks have one slot size)");
    if (native && !mask_bases) return refuse(c, fn, "null dev_mask_bases (native = 1: the ragged rows of vti_masks_native_frames)");
    if (capacity_bytes < 0) return refuse(c, fn, "capacity_bytes must be >= 0");
    if (capacity < 0 || max_points < 0) return refuse(c, fn, "capacity and max_points must be >= 0");
    if (strategy != VTI_POLY_LARGEST && strategy != VTI_POLY_CONCAT)
        return refuse(c, fn, "strategy must be VTI_POLY_LARGEST or VTI_POLY_CONCAT");
    if (!offsets || !point_offsets || (capacity && !masks) || (max_points && !points)) return refuse(c, fn, "null pointer");
    VTI_TRY(mask_align_check(fn, c, capacity ? masks : nullptr, native));
    if (((uintptr_t)mask_bases & 7) || ((uintptr_t)offsets & 3) || ((uintptr_t)point_offsets & 3) || ((uintptr_t)points & 3))
        return refuse(c, fn, "dev_mask_bases must be 8-byte aligned, dev_offsets, dev_point_offsets and dev_points 4-byte aligned");
    if (!poly_sizes_ok(h.H, h.W, h.W / 8)) return refuse(c, fn, "the canvas is above vti_mask_polygons' limit (H * W <= 2^26)");
    PolyLayout L;
    const int32_t big = poly_frames_layout(c, host_table, h, native, L);
    if (big >= 0) {
        char msg[160];
        snprintf(msg, sizeof msg, "frame %d of host_table: H0 * W0 above 2^26 (vti_mask_polygons' limit)", big);
        return refuse(c, fn, msg);
    }
    VTI_TRY(scratch_check(fn, c, scratch, scratch_bytes, (int64_t)L.total, "vti_mask_polygons_frames_scratch_bytes()"));
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, launch_mask_polygons_frames(masks, (const long long*)mask_bases, capacity_bytes, offsets, frame_rows(dev_table), B, capacity,
                                           c->plan.desc.H, c->plan.desc.W, L, strategy, scratch, point_offsets, points,
                                           (long long)max_points, (hipStream_t)stream), "mask_polygons kernels (frames)");
    return VTI_OK;
}

static bool annotate_sizes_ok(int32_t n_sel, int32_t max_det, int32_t H0, int32_t W0, int32_t max_points) {
    return n_sel >= 1 && max_det >= 1 && max_det <= VTI_MEASURE_MAX_DET && H0 >= 1 && W0 >= 1 && H0 <= 8192 && W0 <= 8192 &&
           max_points >= 0 && (int64_t)n_sel * H0 * W0 * 3 <= (int64_t)1 << 40;
}

int64_t vti_annotate_scratch_bytes(const vti_ctx* c, int32_t n_sel, int32_t max_det, int32_t H0, int32_t W0, int32_t max_points) {
    if (!c || !annotate_sizes_ok(n_sel, max_det, H0, W0, max_points)) return 0;
    AnnotateLayout L;
    annotate_layout(n_sel, max_det, H0, W0, max_points, L);
    return (int64_t)L.total;
}

// Every host_select[k] is a frame of the batch (select_at: entry k alone).
static int32_t select_at(const char* fn, vti_ctx* c, const int32_t* host_select, int32_t k, int32_t B) {
    if (host_select[k] >= 0 && host_select[k] < B) return VTI_OK;
    char msg[120];
    snprintf(msg, sizeof msg, "host_select[%d] = %d is outside [0, %d)", k, host_select[k], B);
    return refuse(c, fn, msg);
}
static int32_t select_check(const char* fn, vti_ctx* c, const int32_t* host_select, int32_t n_sel, int32_t B) {
    for (int32_t k = 0; k < n_sel; ++k)
        VTI_TRY(select_at(fn, c, host_select, k, B));
    return VTI_OK;
}

// The measurement rows a picture is drawn from, and the status it reports.
static int32_t meas_rows_check(const char* fn, vti_ctx* c, const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                               const int32_t* status) {
    if (((uintptr_t)stitch_f64 & 7) || ((uintptr_t)stitch_i32 & 3) || ((uintptr_t)frame_i32 & 3) || ((uintptr_t)status & 3))
        return refuse(c, fn, "misaligned measurement rows or status");
    return VTI_OK;
}

// One walk over the selection of a *_frames drawing call: every host_select[k] is a frame of the batch, at most 8192 x 8192 and of
// the size of row k of the out table.  `s` receives the largest H0, W0 and pixel count, and from `in_lds(c, row, slot_words)`, the
// call's layout of one selected frame, which tracers serve the selection and the words of its largest native mask slot.
struct Selection { int32_t mh = 0, mw = 0; long long max_px = 0, max_slot_words = 1; bool any_lds = false, any_global = false; };
static int32_t selection_walk(const char* fn, vti_ctx* c, const void* host_table, const void* host_out_table, const int32_t* host_select,
                              int32_t n_sel, int32_t B, int32_t max_det, int32_t max_points, Selection& s,
                              bool (*in_lds)(const vti_ctx*, const FrameRow&, long long& slot_words)) {
    char msg[200];
    for (int32_t k = 0; k < n_sel; ++k) {
        VTI_TRY(select_at(fn, c, host_select, k, B));
        const int32_t b = host_select[k];
        const FrameRow ri = table_row(host_table, b), ro = table_row(host_out_table, k);
        if (ri.H0 > 8192 || ri.W0 > 8192) {
            snprintf(msg, sizeof msg, "frame %d (host_select[%d]) is %d x %d: H0, W0 must be <= 8192", b, k, ri.H0, ri.W0);
            return refuse(c, fn, msg);
        }
        if (ro.H0 != ri.H0 || ro.W0 != ri.W0) {
            snprintf(msg, sizeof msg, "row %d of the out table is %d x %d, frame host_select[%d] = %d is %d x %d", k, ro.H0, ro.W0, k, b,
                     ri.H0, ri.W0);
            return refuse(c, fn, msg);
        }
        s.mh = std::max(s.mh, ri.H0); s.mw = std::max(s.mw, ri.W0);
        s.max_px = std::max(s.max_px, (long long)ri.H0 * ri.W0);
        long long slot_words = 1;
        (in_lds(c, ri, slot_words) ? s.any_lds : s.any_global) = true;
        s.max_slot_words = std::max(s.max_slot_words, slot_words);
    }
    if (!annotate_sizes_ok(n_sel, max_det, s.mh, s.mw, max_points)) return refuse(c, fn, "the selection is too large");
    return VTI_OK;
}

// ---- vti_annotate (process_frame's picture) and vti_annotate_checker (the stitch-distance checker's) ---------------------------
// The one-struct call of the checker passes p, every other form a camera table.  `checker`: the prep kernel is the checker's.
struct AnnotateCall {
    const char* fn; bool checker; const vti_checker_params* p; const uint8_t* frames;
    // the *_frames forms: the host tables and what selection_walk() found (then H0, W0 below are s->mh, s->mw)
    const void* host_table; const void* host_out_table; Selection* s;
    bool ragged;                // the *_frames_native forms: the masks are the ragged rows (o.native is 1, o.bases given)
};

// Every check of the drawing calls but those of the frame tables themselves, in the order each entry point has always made them, and
// all before the first HIP call.  Uniform forms: H0, W0 are the call's; the *_frames forms set them from the selection.
static int32_t annotate_check(const AnnotateCall& a, vti_ctx* c, int32_t& H0, int32_t& W0, const CameraChoice& cams, const OutputSet& o,
                              const DrawInputs& d) {
    const char* fn = a.fn;
    const vti_desc& desc = c->plan.desc;
    const bool bad_canvas = a.checker && !o.native && ((desc.W & 31) || (size_t)(4 * desc.W + 2 * desc.H) * 4 > 60 * 1024);
    const char* unsuitable = "letterbox size unsuitable for the resize tables";
    // which masks the kernels may read: the ragged rows are cut by capacity_bytes, every other set by the slot count
    const bool reads_masks = a.ragged ? o.capacity_bytes > 0 : o.capacity != 0;
    if (a.s) {
        if (o.capacity < 0 || cams.n_cams < 1 || (!a.ragged && o.native != 0) || o.max_det < 1 || o.max_det > VTI_MEASURE_MAX_DET || d.max_points < 0)
            return refuse(c, fn, "bad size (n_cams >= 1; capacity, max_points >= 0; 1 <= max_det <= VTI_MEASURE_MAX_DET; native 0)");
    } else if (o.B < 1 || o.capacity < 0 || (!a.p && cams.n_cams < 1) || (o.native != 0 && o.native != 1) ||
               !annotate_sizes_ok(d.n_sel, o.max_det, H0, W0, d.max_points))
        return refuse(c, fn, a.p ? "bad size (B, n_sel >= 1; capacity, max_points >= 0; 1 <= max_det <= VTI_MEASURE_MAX_DET; "
                                   "1 <= H0, W0 <= 8192; native 0 or 1)"
                                 : "bad size (B, n_sel, n_cams >= 1; capacity, max_points >= 0; 1 <= max_det <= VTI_MEASURE_MAX_DET; "
                                   "1 <= H0, W0 <= 8192; native 0 or 1)");
    if (!a.frames || (!a.p && !cams.table) || !o.dets || !o.xyxy || !o.counts || !o.offsets || !d.frame_i32 || !d.stitch_f64 ||
        !d.stitch_i32 || !d.host_select || !d.dev_select || !d.out || !d.status || (reads_masks && !o.masks))
        return refuse(c, fn, "null pointer");
    if (a.p)
        if (const char* e = settings_error(*a.p)) return refuse(c, fn, e);
    if (a.s) {
        VTI_TRY(selection_walk(fn, c, a.host_table, a.host_out_table, d.host_select, d.n_sel, o.B, o.max_det, d.max_points, *a.s,
                               [](const vti_ctx*, const FrameRow& r, long long&) {
                                   AnnotateLayout one;                   // the frame's own bitmap: which tracer serves it
                                   annotate_layout(1, 1, r.H0, r.W0, 0, one);
                                   return one.in_lds;
                               }));
        H0 = a.s->mh; W0 = a.s->mw;
        if (((uintptr_t)a.frames & 15) || ((uintptr_t)d.out & 15)) return refuse(c, fn, "dev_frames and dev_out must be 16-byte aligned");
    } else
        VTI_TRY(select_check(fn, c, d.host_select, d.n_sel, o.B));
    if (a.p) {
        if ((uintptr_t)d.dev_select & 3) return refuse(c, fn, "the selection must be 4-byte aligned");
    } else if (((uintptr_t)cams.table & 15) || ((uintptr_t)cams.cam_of_frame & 3) || ((uintptr_t)d.dev_select & 3))
        return refuse(c, fn, "the camera table must be 16-byte aligned, the index arrays 4-byte aligned");
    VTI_TRY(mask_align_check(fn, c, reads_masks ? o.masks : nullptr, o.native));
    if (!a.s && bad_canvas) return refuse(c, fn, unsuitable);
    VTI_TRY(meas_rows_check(fn, c, d.frame_i32, d.stitch_f64, d.stitch_i32, d.status));
    VTI_TRY(scratch_check(fn, c, d.scratch, d.scratch_bytes, vti_annotate_scratch_bytes(c, d.n_sel, o.max_det, H0, W0, d.max_points),
                          a.s ? "vti_annotate_frames_scratch_bytes()" : "vti_annotate_scratch_bytes()"));
    if (a.s && bad_canvas) return refuse(c, fn, unsuitable);
    return VTI_OK;
}

// The checks above, then the launches: launch_annotate or launch_annotate_checker.  fr: the device tables of the *_frames forms.
static int32_t annotate_impl(const AnnotateCall& a, vti_ctx* c, int32_t H0, int32_t W0, const CameraChoice& cams, const OutputSet& o,
                             const DrawInputs& d, void* stream, AnnotateFrames* fr = nullptr) {
    VTI_TRY(annotate_check(a, c, H0, W0, cams, o, d));
    VTI_TRY(check_device(c, a.fn));
    const Canvas cv{c->plan.desc.nm, c->plan.desc.H, c->plan.desc.W};
    if (fr) { fr->any_lds = a.s->any_lds; fr->any_global = a.s->any_global; fr->max_px = a.s->max_px; }
    if (a.checker)
        VTI_HIP(c, launch_annotate_checker(a.p, a.frames, H0, W0, cams, o, cv, d, (hipStream_t)stream, fr), "annotate_checker kernels");
    else
        VTI_HIP(c, launch_annotate(a.frames, H0, W0, cams, o, cv, d, (hipStream_t)stream, fr), "annotate kernels");
    return VTI_OK;
}

int32_t vti_annotate(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, const void* cameras, int32_t n_cams,
                     const int32_t* cam_of_frame, const uint8_t* masks, int32_t native, const float* dets, const float* xyxy,
                     const int32_t* counts, const int32_t* offsets, int32_t max_det, int32_t capacity, const int32_t* frame_i32,
                     const double* stitch_f64, const int32_t* stitch_i32, const int32_t* host_select, const int32_t* dev_select,
                     int32_t n_sel, int32_t max_points, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes,
                     void* stream) {
    if (!c) return refuse(c, "vti_annotate", "null ctx");
    return annotate_impl({"vti_annotate", false, nullptr, frames}, c, H0, W0, {cameras, n_cams, cam_of_frame},
                         {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
                         {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes},
                         stream);
}

int32_t vti_annotate_checker(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, const vti_checker_params* p,
                             const uint8_t* masks, int32_t native, const float* dets, const float* xyxy, const int32_t* counts,
                             const int32_t* offsets, int32_t max_det, int32_t capacity, const int32_t* frame_i32,
                             const double* stitch_f64, const int32_t* stitch_i32, const int32_t* host_select, const int32_t* dev_select,
                             int32_t n_sel, int32_t max_points, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes,
                             void* stream) {
    if (!c || !p) return refuse(c, "vti_annotate_checker", "null ctx or params");
    return annotate_impl({"vti_annotate_checker", true, p, frames}, c, H0, W0, {},
                         {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
                         {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes},
                         stream);
}

int32_t vti_annotate_checker_cameras(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, const void* cameras,
                                     int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks, int32_t native,
                                     const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets,
                                     int32_t max_det, int32_t capacity, const int32_t* frame_i32, const double* stitch_f64,
                                     const int32_t* stitch_i32, const int32_t* host_select, const int32_t* dev_select, int32_t n_sel,
                                     int32_t max_points, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes,
                                     void* stream) {
    if (!c) return refuse(c, "vti_annotate_checker_cameras", "null ctx");
    return annotate_impl({"vti_annotate_checker_cameras", true, nullptr, frames}, c, H0, W0, {cameras, n_cams, cam_of_frame},
                         {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
                         {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes},
                         stream);
}

// ---- vti_overlay: the model-check viewer's picture ---------------------------------------------------------------------------
int64_t vti_overlay_scratch_bytes(const vti_ctx* c, int32_t n_sel, int32_t max_det, int32_t H0, int32_t W0, int32_t max_points) {
    if (!c || !annotate_sizes_ok(n_sel, max_det, H0, W0, max_points)) return 0;
    OverlayLayout L;
    overlay_layout(n_sel, max_det, H0, W0, c->plan.desc.H, c->plan.desc.W, max_points, L);
    return (int64_t)L.total;
}

// What vti_overlay and vti_overlay_frames check alike: the mode with its picture, the palette, the blend weights, and the alignment of
// the rows the kernels index.
static int32_t overlay_args_check(const char* fn, vti_ctx* c, int32_t mode, const uint8_t* annotated, int32_t n_colours, float alpha,
                                  float beta, const int32_t* dev_select, const int32_t* counts, const int32_t* offsets,
                                  const int32_t* status, const float* dets, const float* xyxy, const int32_t* plates) {
    if (mode != VTI_OVERLAY_DRAW && mode != VTI_OVERLAY_BLEND && mode != VTI_OVERLAY_BOTH)
        return refuse(c, fn, "mode must be VTI_OVERLAY_DRAW, VTI_OVERLAY_BLEND or VTI_OVERLAY_BOTH");
    if (n_colours < 1 || n_colours > 16) return refuse(c, fn, "n_colours must be 1 .. 16");
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return refuse(c, fn, "alpha and beta must be finite");
    if ((annotated != nullptr) != (mode == VTI_OVERLAY_BLEND))
        return refuse(c, fn, "dev_annotated must be given with VTI_OVERLAY_BLEND and only then");
    if (((uintptr_t)dev_select & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)offsets & 3) || ((uintptr_t)status & 3) ||
        ((uintptr_t)dets & 3) || ((uintptr_t)xyxy & 3))
        return refuse(c, fn, "the index arrays, rows and status must be 4-byte aligned");
    if (plates && ((uintptr_t)plates & 15)) return refuse(c, fn, "dev_plates must be 16-byte aligned");
    return VTI_OK;
}

int32_t vti_overlay(vti_ctx* c, const uint8_t* frames, int32_t B, int32_t H0, int32_t W0, const uint8_t* masks, int32_t native,
                    const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t max_det,
                    int32_t capacity, const int32_t* plates, const uint8_t* host_palette, int32_t n_colours, float alpha, float beta,
                    const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t mode, const uint8_t* annotated,
                    int32_t max_points, uint8_t* out, int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_overlay";
    if (!c) return refuse(c, fn, "null ctx");
    if (B < 1 || capacity < 0 || (native != 0 && native != 1) || !annotate_sizes_ok(n_sel, max_det, H0, W0, max_points))
        return refuse(c, fn, "bad size (B, n_sel >= 1; capacity, max_points >= 0; 1 <= max_det <= VTI_MEASURE_MAX_DET; "
                             "1 <= H0, W0 <= 8192; native 0 or 1)");
    if (!frames || !dets || !xyxy || !counts || !offsets || !host_palette || !host_select || !dev_select || !out || !status ||
        (capacity && !masks))
        return refuse(c, fn, "null pointer");
    VTI_TRY(overlay_args_check(fn, c, mode, annotated, n_colours, alpha, beta, dev_select, counts, offsets, status, dets, xyxy, plates));
    VTI_TRY(select_check(fn, c, host_select, n_sel, B));
    VTI_TRY(mask_align_check(fn, c, capacity ? masks : nullptr, native));
    VTI_TRY(scratch_check(fn, c, scratch, scratch_bytes, vti_overlay_scratch_bytes(c, n_sel, max_det, H0, W0, max_points),
                          "vti_overlay_scratch_bytes()"));
    VTI_TRY(check_device(c, fn));
    const vti_desc& d = c->plan.desc;
    VTI_HIP(c, launch_overlay(frames, B, H0, W0, masks, native, dets, xyxy, counts, offsets, max_det, d.nm, capacity, d.H, d.W, plates,
                              host_palette, n_colours, alpha, beta, dev_select, n_sel, mode, annotated, max_points, out, status, scratch,
                              (hipStream_t)stream), "overlay kernels");
    return VTI_OK;
}

// ---- vti_annotate and vti_overlay for frames of differing sizes --------------------------------------------------------------
// The rows and the largest H0 and W0 of a host out table (of the rows themselves: the header's maxima are only an upper bound);
// 0 rows when it is no table of vti_pack_frames.
static int32_t out_table_maxima(const void* host_out_table, int32_t& mh, int32_t& mw) {
    mh = mw = 0;
    if (!host_out_table) return 0;
    const FrameTableHeader h = table_header(host_out_table);
    if (h.magic != kFrameTableMagic || h.B < 1) return 0;
    for (int32_t k = 0; k < h.B; ++k) {
        const FrameRow r = table_row(host_out_table, k);
        mh = std::max(mh, r.H0); mw = std::max(mw, r.W0);
    }
    return h.B;
}

int64_t vti_annotate_frames_scratch_bytes(const vti_ctx* c, const void* host_out_table, int32_t max_det, int32_t max_points) {
    int32_t mh, mw;
    const int32_t n = out_table_maxima(host_out_table, mh, mw);
    return n ? vti_annotate_scratch_bytes(c, n, max_det, mh, mw, max_points) : 0;
}

int64_t vti_overlay_frames_scratch_bytes(const vti_ctx* c, const void* host_out_table, int32_t max_det, int32_t max_points) {
    int32_t mh, mw;
    const int32_t n = out_table_maxima(host_out_table, mh, mw);
    return n ? vti_overlay_scratch_bytes(c, n, max_det, mh, mw, max_points) : 0;
}

// vti_annotate_frames and vti_annotate_checker_frames (checker: the table is the checker's, the prep kernel the checker's own): the
// two frame tables, then annotate_impl's checks and launches
// one_size == nullptr: the *_frames_native forms (o.native is 1 and o.bases, o.capacity_bytes are the caller's)
static int32_t annotate_frames_impl(const char* fn, const char* out_fn, const char* one_size, bool checker, vti_ctx* c,
                                    const uint8_t* frames, const void* host_table, const void* dev_table, const void* host_out_table,
                                    const void* dev_out_table, const CameraChoice& cams, const OutputSet& o, const DrawInputs& d,
                                    void* stream) {
    // every check comes before the first HIP call
    if (!c) return refuse(c, fn, "null ctx");
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, o.B, h));
    if (d.n_sel < 1) return refuse(c, fn, "n_sel must be >= 1");
    VTI_TRY(frames_check(out_fn, c, host_out_table, dev_out_table, d.n_sel, h));
    const bool ragged = one_size == nullptr;
    if (ragged) {
        if (!o.bases) return refuse(c, fn, "null dev_mask_bases");
        if ((uintptr_t)o.bases & 7) return refuse(c, fn, "dev_mask_bases must be 8-byte aligned");
        if (o.capacity_bytes < 0) return refuse(c, fn, "capacity_bytes must be >= 0");
    } else if (o.native == 1)
        return refuse(c, fn, one_size, VTI_ERR_UNSUPPORTED);
    Selection s;
    AnnotateFrames fr{frame_rows(dev_table), frame_rows(dev_out_table), false, false, 0};
    return annotate_impl({fn, checker, nullptr, frames, host_table, host_out_table, &s, ragged}, c, 0, 0, cams, o, d, stream, &fr);
}

int32_t vti_annotate_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                            const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks, int32_t native,
                            const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t max_det,
                            int32_t capacity, const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                            const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t max_points,
                            const void* host_out_table, const void* dev_out_table, uint8_t* out, int32_t* status, void* scratch,
                            size_t scratch_bytes, void* stream) {
    return annotate_frames_impl(
        "vti_annotate_frames", "vti_annotate_frames (out table)", "native masks need frames of one size (vti_annotate)", false, c, frames,
        host_table, dev_table, host_out_table, dev_out_table, {cameras, n_cams, cam_of_frame},
        {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
        {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes}, stream);
}

int32_t vti_annotate_checker_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                                    const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                    int32_t native, const float* dets, const float* xyxy, const int32_t* counts, const int32_t* offsets,
                                    int32_t max_det, int32_t capacity, const int32_t* frame_i32, const double* stitch_f64,
                                    const int32_t* stitch_i32, const int32_t* host_select, const int32_t* dev_select, int32_t n_sel,
                                    int32_t max_points, const void* host_out_table, const void* dev_out_table, uint8_t* out,
                                    int32_t* status, void* scratch, size_t scratch_bytes, void* stream) {
    return annotate_frames_impl(
        "vti_annotate_checker_frames", "vti_annotate_checker_frames (out table)",
        "native masks need frames of one size (vti_annotate_checker_cameras)", true, c, frames, host_table, dev_table, host_out_table,
        dev_out_table, {cameras, n_cams, cam_of_frame}, {masks, native, dets, xyxy, counts, offsets, B, max_det, capacity, nullptr, 0},
        {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes}, stream);
}

int32_t vti_annotate_frames_native(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                                   const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                   const int64_t* mask_bases, int64_t capacity_bytes, const float* dets, const float* xyxy,
                                   const int32_t* counts, const int32_t* offsets, int32_t max_det, int32_t capacity,
                                   const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                                   const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t max_points,
                                   const void* host_out_table, const void* dev_out_table, uint8_t* out, int32_t* status, void* scratch,
                                   size_t scratch_bytes, void* stream) {
    return annotate_frames_impl(
        "vti_annotate_frames_native", "vti_annotate_frames_native (out table)", nullptr, false, c, frames, host_table, dev_table,
        host_out_table, dev_out_table, {cameras, n_cams, cam_of_frame},
        {masks, 1, dets, xyxy, counts, offsets, B, max_det, capacity, (const long long*)mask_bases, capacity_bytes},
        {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes}, stream);
}

int32_t vti_annotate_checker_frames_native(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                                           const void* cameras, int32_t n_cams, const int32_t* cam_of_frame, const uint8_t* masks,
                                           const int64_t* mask_bases, int64_t capacity_bytes, const float* dets, const float* xyxy,
                                           const int32_t* counts, const int32_t* offsets, int32_t max_det, int32_t capacity,
                                           const int32_t* frame_i32, const double* stitch_f64, const int32_t* stitch_i32,
                                           const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t max_points,
                                           const void* host_out_table, const void* dev_out_table, uint8_t* out, int32_t* status,
                                           void* scratch, size_t scratch_bytes, void* stream) {
    return annotate_frames_impl(
        "vti_annotate_checker_frames_native", "vti_annotate_checker_frames_native (out table)", nullptr, true, c, frames, host_table,
        dev_table, host_out_table, dev_out_table, {cameras, n_cams, cam_of_frame},
        {masks, 1, dets, xyxy, counts, offsets, B, max_det, capacity, (const long long*)mask_bases, capacity_bytes},
        {frame_i32, stitch_f64, stitch_i32, host_select, dev_select, n_sel, max_points, out, status, scratch, scratch_bytes}, stream);
}

int32_t vti_overlay_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t B,
                           const uint8_t* masks, int32_t native, const int64_t* mask_bases, int64_t capacity_bytes, const float* dets,
                           const float* xyxy, const int32_t* counts, const int32_t* offsets, int32_t max_det, int32_t capacity,
                           const int32_t* plates, const uint8_t* host_palette, int32_t n_colours, float alpha, float beta,
                           const int32_t* host_select, const int32_t* dev_select, int32_t n_sel, int32_t mode, const uint8_t* annotated,
                           int32_t max_points, const void* host_out_table, const void* dev_out_table, uint8_t* out, int32_t* status,
                           void* scratch, size_t scratch_bytes, void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_overlay_frames";
    if (!c) return refuse(c, fn, "null ctx");
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, B, h));
    if (n_sel < 1) return refuse(c, fn, "n_sel must be >= 1");
    VTI_TRY(frames_check("vti_overlay_frames (out table)", c, host_out_table, dev_out_table, n_sel, h));
    if (capacity < 0 || (native != 0 && native != 1) || max_det < 1 || max_det > VTI_MEASURE_MAX_DET || max_points < 0)
        return refuse(c, fn, "bad size (capacity, max_points >= 0; 1 <= max_det <= VTI_MEASURE_MAX_DET; native 0 or 1)");
    if (!native && mask_bases) return refuse(c, fn, "dev_mask_bases must be NULL with letterbox masks (native = 0)");
    if (native && !mask_bases) return refuse(c, fn, "native masks need dev_mask_bases (vti_masks_native_frames)");
    if (capacity_bytes < 0) return refuse(c, fn, "capacity_bytes must be >= 0");
    const bool need_masks = capacity > 0 && (!native || capacity_bytes > 0);
    if (!frames || !dets || !xyxy || !counts || !offsets || !host_palette || !host_select || !dev_select || !out || !status ||
        (need_masks && !masks))
        return refuse(c, fn, "null pointer");
    VTI_TRY(overlay_args_check(fn, c, mode, annotated, n_colours, alpha, beta, dev_select, counts, offsets, status, dets, xyxy, plates));
    Selection s;
    VTI_TRY(selection_walk(fn, c, host_table, host_out_table, host_select, n_sel, B, max_det, max_points, s,
                           [](const vti_ctx* c, const FrameRow& r, long long& slot_words) {
                               OverlayLayout one;                    // the frame's own bitmap: which tracer serves it, and the words of its native slot
                               overlay_layout(1, 1, r.H0, r.W0, c->plan.desc.H, c->plan.desc.W, 0, one);
                               slot_words = (long long)r.H0 * 2 * one.WW;
                               return one.in_lds;
                           }));
    if (((uintptr_t)frames & 15) || ((uintptr_t)out & 15) || ((uintptr_t)annotated & 15))
        return refuse(c, fn, "dev_frames, dev_out and dev_annotated must be 16-byte aligned");
    if (mask_bases && ((uintptr_t)mask_bases & 7)) return refuse(c, fn, "dev_mask_bases must be 8-byte aligned");
    VTI_TRY(mask_align_check(fn, c, need_masks ? masks : nullptr, native));
    VTI_TRY(scratch_check(fn, c, scratch, scratch_bytes, vti_overlay_scratch_bytes(c, n_sel, max_det, s.mh, s.mw, max_points),
                          "vti_overlay_frames_scratch_bytes()"));
    VTI_TRY(check_device(c, fn));
    const vti_desc& d = c->plan.desc;
    const OverlayFrames fr{frame_rows(dev_table), frame_rows(dev_out_table), (const long long*)mask_bases, capacity_bytes,
                           s.max_slot_words, s.any_lds, s.any_global, s.max_px};
    VTI_HIP(c, launch_overlay(frames, B, s.mh, s.mw, masks, native, dets, xyxy, counts, offsets, max_det, d.nm, capacity, d.H, d.W, plates,
                              host_palette, n_colours, alpha, beta, dev_select, n_sel, mode, annotated, max_points, out, status, scratch,
                              (hipStream_t)stream, &fr), "overlay kernels");
    return VTI_OK;
}

int64_t vti_encode_jpeg_scratch_bytes(const vti_ctx* c, int32_t n, int32_t H0, int32_t W0) {
    JpegLayout L;
    if (!c || !encode_jpeg_layout(n, H0, W0, L)) return 0;
    return (int64_t)L.total;
}

int64_t vti_encode_jpeg_max_bytes(int32_t n, int32_t H0, int32_t W0) {
    JpegLayout L;
    if (!encode_jpeg_layout(n, H0, W0, L)) return 0;
    return (int64_t)n * L.max_file;
}

// What the two encode calls check alike: the settings, the pointers and the scratch (`need` bytes, the answer of `query`).
static int32_t jpeg_args_check(const char* fn, vti_ctx* c, const uint8_t* frames, int32_t rgb, int32_t quality, const void* scratch,
                               size_t scratch_bytes, int64_t need, const char* query, const int64_t* offsets, const uint8_t* out,
                               int64_t max_bytes) {
    if (quality < 1 || quality > 100 || (rgb != 0 && rgb != 1) || max_bytes < 0)
        return refuse(c, fn, "1 <= quality <= 100, rgb 0 or 1, max_bytes >= 0");
    if (!frames || !offsets || (max_bytes && !out)) return refuse(c, fn, "null pointer");
    if ((uintptr_t)offsets & 7) return refuse(c, fn, "dev_byte_offsets must be 8-byte aligned");
    return scratch_check(fn, c, scratch, scratch_bytes, need, query);
}

int32_t vti_encode_jpeg(vti_ctx* c, const uint8_t* frames, int32_t n, int32_t H0, int32_t W0, int32_t rgb, int32_t quality,
                        void* scratch, size_t scratch_bytes, int64_t* offsets, uint8_t* out, int64_t max_bytes, void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_encode_jpeg";
    if (!c) return refuse(c, fn, "null ctx");
    JpegLayout L;
    if (!encode_jpeg_layout(n, H0, W0, L))
        return refuse(c, fn, "bad size (n >= 1; 1 <= H0, W0 <= 8192; n * ceil(H0/16) * ceil(W0/16) <= 2^28)");
    VTI_TRY(jpeg_args_check(fn, c, frames, rgb, quality, scratch, scratch_bytes, (int64_t)L.total,
                            "vti_encode_jpeg_scratch_bytes()", offsets, out, max_bytes));
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, launch_encode_jpeg(frames, n, H0, W0, rgb, quality, scratch, (long long*)offsets, out, (long long)max_bytes,
                                  (hipStream_t)stream), "encode_jpeg kernels");
    return VTI_OK;
}

// ---- vti_encode_jpeg for frames of differing sizes -------------------------------------------------------------------------
// The header and rows of a host frame table, as far as they can be checked without a ctx: nullptr, or what is wrong.
static const char* jpeg_table_error(const void* host_table, JpegFramesLayout& L) {
    if (!host_table) return "null frame table";
    const FrameTableHeader h = table_header(host_table);
    if (h.magic != kFrameTableMagic || h.B < 1) return "host_table is not a table of vti_pack_frames";
    if (!encode_jpeg_frames_layout(host_table, L)) return "a frame is outside 1 <= H0, W0 <= 8192, or the batch has more than 2^28 MCUs";
    return nullptr;
}

int64_t vti_encode_jpeg_frames_scratch_bytes(const vti_ctx* c, const void* host_table) {
    JpegFramesLayout L;
    if (!c || jpeg_table_error(host_table, L)) return 0;
    return (int64_t)L.total;
}

int64_t vti_encode_jpeg_frames_max_bytes(const void* host_table) {
    JpegFramesLayout L;
    if (jpeg_table_error(host_table, L)) return 0;
    return (int64_t)L.max_bytes;
}

int32_t vti_encode_jpeg_frames(vti_ctx* c, const uint8_t* frames, const void* host_table, const void* dev_table, int32_t n, int32_t rgb,
                               int32_t quality, void* scratch, size_t scratch_bytes, int64_t* offsets, uint8_t* out, int64_t max_bytes,
                               void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_encode_jpeg_frames";
    if (!c) return refuse(c, fn, "null ctx");
    FrameTableHeader h;
    VTI_TRY(frames_check(fn, c, host_table, dev_table, n, h));
    JpegFramesLayout L;
    if (const char* e = jpeg_table_error(host_table, L)) return refuse(c, fn, e);
    VTI_TRY(jpeg_args_check(fn, c, frames, rgb, quality, scratch, scratch_bytes, (int64_t)L.total,
                            "vti_encode_jpeg_frames_scratch_bytes()", offsets, out, max_bytes));
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, launch_encode_jpeg_frames(frames, host_table, frame_rows(dev_table), rgb, quality, scratch, (long long*)offsets, out,
                                         (long long)max_bytes, (hipStream_t)stream), "encode_jpeg_frames kernels");
    return VTI_OK;
}

// ---- the text of the annotated pictures: the stamp table, vti_stamp, vti_stamp_frames -------------------------------------------
int64_t vti_stamp_table_bytes(int32_t n_pictures, int32_t n_stamps) {
    if (n_pictures < 1 || n_pictures > VTI_STAMP_MAX_PICTURES || n_stamps < 0 || n_stamps > VTI_STAMP_MAX_TOTAL) return 0;
    return (int64_t)sizeof(StampHeader) + (int64_t)n_pictures * (int64_t)sizeof(StampPicture) + (int64_t)n_stamps * (int64_t)sizeof(StampRec);
}

// What is wrong with one stamp of a picture of H0 x W0 and a bit buffer of n_words words (nullptr: nothing).  vti_pack_stamps runs it
// on its arguments, vti_stamp and vti_stamp_frames on every record of the host table they are given.
static const char* stamp_error(int32_t H0, int32_t W0, const StampRec& r, int64_t n_words) {
    if (r.w < 1 || r.h < 1) return "w and h must be >= 1";
    if (r.x < 0 || r.y < 0 || r.x > W0 - r.w || r.y > H0 - r.h) return "the rectangle is not inside its picture";
    if (r.pitch < (r.w + 31) / 32) return "pitch must be >= ceil(w / 32)";
    if (r.pitch > VTI_STAMP_MAX_PITCH) return "pitch must be <= VTI_STAMP_MAX_PITCH";
    if (r.offset < 0 || r.offset > n_words || (int64_t)r.h * r.pitch > n_words - r.offset) return "its rows run past n_words (or word_offset < 0)";
    return nullptr;
}

static bool stamp_picture_ok(int32_t H0, int32_t W0) { return H0 >= 1 && W0 >= 1 && H0 <= kStampMaxSide && W0 <= kStampMaxSide; }

int32_t vti_pack_stamps(vti_ctx* c, const int32_t* H0, const int32_t* W0, int32_t n_pictures, const vti_stamp_desc* stamps,
                        int32_t n_stamps, int64_t n_words, void* host_table, size_t nbytes) {
    const char* fn = "vti_pack_stamps";
    char msg[200];
    if (!H0 || !W0 || !host_table || (n_stamps > 0 && !stamps)) return refuse(c, fn, "null array or table");
    if (n_pictures < 1 || n_pictures > VTI_STAMP_MAX_PICTURES) return refuse(c, fn, "1 <= n_pictures <= VTI_STAMP_MAX_PICTURES");
    if (n_stamps < 0 || n_stamps > VTI_STAMP_MAX_TOTAL) return refuse(c, fn, "0 <= n_stamps <= VTI_STAMP_MAX_TOTAL");
    if (n_words < 0 || n_words > kStampMaxWords) return refuse(c, fn, "0 <= n_words <= 2^40");
    if ((int64_t)nbytes < vti_stamp_table_bytes(n_pictures, n_stamps)) return refuse(c, fn, "table smaller than vti_stamp_table_bytes()");
    for (int32_t k = 0; k < n_pictures; ++k)
        if (!stamp_picture_ok(H0[k], W0[k])) {
            snprintf(msg, sizeof msg, "%s: picture %d: 1 <= H0, W0 <= 8192", fn, k);
            return fail(c, VTI_ERR_ARG, msg);
        }
    StampHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kStampTableMagic; h.n_pictures = n_pictures; h.n_stamps = n_stamps; h.n_words = n_words;
    char* pics = (char*)host_table + sizeof h;
    char* recs = pics + (size_t)n_pictures * sizeof(StampPicture);
    int32_t k = 0, begin = 0;               // the picture whose range is open, and where it began
    auto close = [&](int32_t end) {
        const StampPicture p{H0[k], W0[k], begin, end};
        memcpy(pics + (size_t)k * sizeof p, &p, sizeof p);
        ++k; begin = end;
    };
    for (int32_t i = 0; i < n_stamps; ++i) {
        const vti_stamp_desc& s = stamps[i];
        auto bad = [&](const char* what) { snprintf(msg, sizeof msg, "%s: stamp %d: %s", fn, i, what); return fail(c, VTI_ERR_ARG, msg); };
        if (s.picture < 0 || s.picture >= n_pictures) return bad("picture outside [0, n_pictures)");
        if (s.picture < k) return bad("picture must not decrease along the array");
        while (k < s.picture) close(i);
        StampRec r;
        memset(&r, 0, sizeof r);
        r.offset = s.word_offset; r.x = s.x; r.y = s.y; r.w = s.w; r.h = s.h; r.pitch = s.pitch;
        r.colour = (unsigned)s.bgr[0] | (unsigned)s.bgr[1] << 8 | (unsigned)s.bgr[2] << 16;
        if (const char* e = stamp_error(H0[k], W0[k], r, n_words)) return bad(e);
        if (i - begin >= VTI_STAMP_MAX_PER_PICTURE) return bad("more than VTI_STAMP_MAX_PER_PICTURE stamps in its picture");
        memcpy(recs + (size_t)i * sizeof r, &r, sizeof r);
    }
    while (k < n_pictures) close(n_stamps);
    memcpy(host_table, &h, sizeof h);
    return VTI_OK;
}

// The checks vti_stamp and vti_stamp_frames make on their stamp table pair and bit buffer: the host copy is a table of
// vti_pack_stamps for n pictures and this n_words whose ranges and records still pass, picture k having the size of row k of the
// (checked) host frame table, or H0 x W0 when there is none.
static int32_t stamps_check(const char* fn, vti_ctx* c, const void* host_table, const void* dev_table, const uint32_t* bits, int32_t n,
                            int64_t n_words, StampHeader& h, int32_t H0, int32_t W0, const void* host_frame_table) {
    char msg[240];
    if (!host_table || !dev_table) return refuse(c, fn, "null stamp table (host copy or device copy)");
    if ((uintptr_t)dev_table & 15) return refuse(c, fn, "the device stamp table must be 16-byte aligned");
    if ((uintptr_t)bits & 3) return refuse(c, fn, "dev_bits must be 4-byte aligned");
    memcpy(&h, host_table, sizeof h);
    if (h.magic != kStampTableMagic) return refuse(c, fn, "host_table is not a table of vti_pack_stamps");
    if (h.n_pictures != n) return refuse(c, fn, "the stamp table was packed for another number of pictures");
    if (h.n_stamps < 0 || h.n_stamps > VTI_STAMP_MAX_TOTAL || h.n_words < 0 || h.n_words > kStampMaxWords)
        return refuse(c, fn, "host_table is not a table of vti_pack_stamps");
    if (h.n_words != n_words) return refuse(c, fn, "the stamp table was packed for another n_words");
    if (h.n_stamps > 0 && !bits) return refuse(c, fn, "null dev_bits");
    const char* pics = (const char*)host_table + sizeof h;
    const char* recs = pics + (size_t)n * sizeof(StampPicture);
    int32_t at = 0;
    for (int32_t k = 0; k < n; ++k) {
        StampPicture p;
        memcpy(&p, pics + (size_t)k * sizeof p, sizeof p);
        if (host_frame_table) {
            const FrameRow fr = table_row(host_frame_table, k);
            H0 = fr.H0; W0 = fr.W0;
        }
        if (p.H0 != H0 || p.W0 != W0) {
            snprintf(msg, sizeof msg, "%s: picture %d of the stamp table is %d x %d, the call's is %d x %d", fn, k, p.H0, p.W0, H0, W0);
            return fail(c, VTI_ERR_ARG, msg);
        }
        if (p.begin != at || p.end < p.begin || p.end > h.n_stamps || p.end - p.begin > VTI_STAMP_MAX_PER_PICTURE) {
            snprintf(msg, sizeof msg, "%s: picture %d of host_table: its range of stamps is not the one vti_pack_stamps wrote", fn, k);
            return fail(c, VTI_ERR_ARG, msg);
        }
        for (int32_t i = p.begin; i < p.end; ++i) {
            StampRec r;
            memcpy(&r, recs + (size_t)i * sizeof r, sizeof r);
            if (const char* e = stamp_error(H0, W0, r, n_words)) {
                snprintf(msg, sizeof msg, "%s: stamp %d of host_table: %s", fn, i, e);
                return fail(c, VTI_ERR_ARG, msg);
            }
        }
        at = p.end;
    }
    if (at != h.n_stamps) return refuse(c, fn, "host_table: the pictures' ranges do not cover its stamps");
    return VTI_OK;
}

int32_t vti_stamp(vti_ctx* c, uint8_t* pictures, int32_t n, int32_t H0, int32_t W0, const void* host_table, const void* dev_table,
                  const uint32_t* bits, int64_t n_words, void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_stamp";
    if (!c) return refuse(c, fn, "null ctx");
    if (n < 1 || n > VTI_STAMP_MAX_PICTURES || !stamp_picture_ok(H0, W0))
        return refuse(c, fn, "bad size (1 <= n <= VTI_STAMP_MAX_PICTURES; 1 <= H0, W0 <= 8192)");
    if (!pictures) return refuse(c, fn, "null pointer");
    StampHeader h;
    VTI_TRY(stamps_check(fn, c, host_table, dev_table, bits, n, n_words, h, H0, W0, nullptr));
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, launch_stamp(pictures, n, H0, W0, nullptr, 0, (long long)H0 * W0, dev_table, h.n_stamps, bits, n_words, (hipStream_t)stream),
            "stamp kernel");
    return VTI_OK;
}

int32_t vti_stamp_frames(vti_ctx* c, uint8_t* buf, const void* host_frame_table, const void* dev_frame_table, int32_t n,
                         const void* host_table, const void* dev_table, const uint32_t* bits, int64_t n_words, void* stream) {
    // every check comes before the first HIP call
    const char* fn = "vti_stamp_frames";
    if (!c) return refuse(c, fn, "null ctx");
    FrameTableHeader fh;
    VTI_TRY(frames_check(fn, c, host_frame_table, dev_frame_table, n, fh));
    if (n > VTI_STAMP_MAX_PICTURES) return refuse(c, fn, "bad size (1 <= n <= VTI_STAMP_MAX_PICTURES)");
    if (!buf) return refuse(c, fn, "null pointer");
    if ((uintptr_t)buf & 15) return refuse(c, fn, "dev_buf must be 16-byte aligned");
    long long max_px = 0;
    for (int32_t k = 0; k < n; ++k) {
        const FrameRow r = table_row(host_frame_table, k);
        if (!stamp_picture_ok(r.H0, r.W0)) {
            char msg[200];
            snprintf(msg, sizeof msg, "%s: frame %d is %d x %d; a stamped picture is at most 8192 x 8192", fn, k, r.H0, r.W0);
            return fail(c, VTI_ERR_ARG, msg);
        }
        max_px = std::max(max_px, (long long)r.H0 * r.W0);
    }
    StampHeader h;
    VTI_TRY(stamps_check(fn, c, host_table, dev_table, bits, n, n_words, h, 0, 0, host_frame_table));
    VTI_TRY(check_device(c, fn));
    VTI_HIP(c, launch_stamp(buf, n, std::min(fh.max_H0, kStampMaxSide), std::min(fh.max_W0, kStampMaxSide), frame_rows(dev_frame_table),
                            fh.total_bytes, max_px, dev_table, h.n_stamps, bits, n_words, (hipStream_t)stream), "stamp kernel");
    return VTI_OK;
}

int64_t vti_decode_jpeg_table_bytes(int32_t n) {
    return n < 1 || n > kJpegDecMaxFiles ? 0 : (int64_t)sizeof(JpegDecHeader) + (int64_t)n * (int64_t)sizeof(JpegDecRow);
}

int32_t vti_decode_jpeg_plan(vti_ctx* c, const uint8_t* files, const int64_t* file_offsets, int32_t n, int32_t segment_bytes,
                             int32_t layout, void* host_table, size_t nbytes, int32_t* out_H0, int32_t* out_W0, int64_t* out_byte_offsets,
                             int64_t* out_scratch_bytes) {
    auto bad = [&](const std::string& what) { return fail(c, VTI_ERR_ARG, what); };
    if (n < 1 || n > kJpegDecMaxFiles) return bad("vti_decode_jpeg_plan: 1 <= n <= 4096");
    if (!files || !file_offsets || !host_table || !out_H0 || !out_W0 || !out_byte_offsets || !out_scratch_bytes)
        return bad("vti_decode_jpeg_plan: null pointer");
    if (layout != 0 && layout != 1) return bad("vti_decode_jpeg_plan: layout 0 (frames at multiples of 16 bytes) or 1 (dense)");
    if (segment_bytes == 0) segment_bytes = kJpegDecDefaultSegment;
    if (segment_bytes < 16 || segment_bytes > 4096 || (segment_bytes & (segment_bytes - 1)))
        return bad("vti_decode_jpeg_plan: segment_bytes must be 0 or a power of two from 16 to 4096");
    if ((int64_t)nbytes < vti_decode_jpeg_table_bytes(n)) return bad("vti_decode_jpeg_plan: table smaller than vti_decode_jpeg_table_bytes()");
    if (file_offsets[0] < 0) return bad("vti_decode_jpeg_plan: host_file_offsets[0] < 0");
    for (int32_t k = 0; k < n; ++k)
        if (file_offsets[k + 1] < file_offsets[k]) return bad("vti_decode_jpeg_plan: host_file_offsets must ascend (file " + std::to_string(k) + ")");
    JpegDecHeader H;
    memset(&H, 0, sizeof H);
    H.magic = kJpegDecMagic;
    H.n = n;
    H.layout = layout;
    H.seg_bytes = segment_bytes;
    H.files_bytes = file_offsets[n];
    std::vector<JpegDecRow> rows((size_t)n);
    size_t scratch_at = 0;
    long long out_at = 0;
    for (int32_t k = 0; k < n; ++k) {
        JpegDecRow& R = rows[(size_t)k];
        std::string why;
        const int rc = decode_jpeg_parse(files + file_offsets[k], file_offsets[k + 1] - file_offsets[k], R, why);
        if (rc) return fail(c, rc, "vti_decode_jpeg_plan: file " + std::to_string(k) + ": " + why);
        if (layout == 1 && (R.H0 != rows[0].H0 || R.W0 != rows[0].W0))
            return bad("vti_decode_jpeg_plan: file " + std::to_string(k) + ": layout 1 (dense) needs files of one size");
        R.file_off = file_offsets[k];
        R.scan_start += R.file_off;
        R.scan_end += R.file_off;
        R.seg_bytes = segment_bytes;
        R.nseg = (int)std::max<long long>(1, (R.scan_end - R.scan_start + segment_bytes - 1) / segment_bytes);
        scratch_at = decode_jpeg_scratch_of(R, scratch_at);
        R.out_off = out_at;
        out_H0[k] = R.H0;
        out_W0[k] = R.W0;
        out_byte_offsets[k] = out_at;
        out_at += 3LL * R.H0 * R.W0;
        if (layout == 0) out_at = (out_at + 15) & ~15LL;
    }
    if (layout == 0) out_at = std::max<long long>(out_at, 16);
    out_byte_offsets[n] = out_at;
    H.out_bytes = out_at;
    H.scratch_bytes = (long long)scratch_at;
    *out_scratch_bytes = H.scratch_bytes;
    memcpy(host_table, &H, sizeof H);
    memcpy((uint8_t*)host_table + sizeof H, rows.data(), (size_t)n * sizeof(JpegDecRow));
    return VTI_OK;
}

int32_t vti_decode_jpeg(vti_ctx* c, const uint8_t* files, const void* host_table, const void* dev_table, int32_t n, int32_t rgb,
                        uint8_t* out, int64_t out_bytes, int32_t* info, void* scratch, size_t scratch_bytes, void* stream) {
    // every check comes before the first HIP call
    auto bad = [&](const std::string& what) { return fail(c, VTI_ERR_ARG, what); };
    if (!c) return bad("vti_decode_jpeg: null ctx");
    if (n < 1 || n > kJpegDecMaxFiles) return bad("vti_decode_jpeg: 1 <= n <= 4096");
    if (rgb != 0 && rgb != 1) return bad("vti_decode_jpeg: rgb 0 or 1");
    if (!files || !host_table || !dev_table || !out || !info) return bad("vti_decode_jpeg: null pointer");
    if (((uintptr_t)dev_table & 15) || ((uintptr_t)info & 3)) return bad("vti_decode_jpeg: dev_table must be 16-byte aligned, dev_info 4-byte aligned");
    JpegDecHeader H;
    memcpy(&H, host_table, sizeof H);
    if (H.magic != kJpegDecMagic || H.n != n || (H.layout != 0 && H.layout != 1) || H.files_bytes < 0 || H.out_bytes < 0 || H.scratch_bytes < 0)
        return bad("vti_decode_jpeg: host_table is not a descriptor table of vti_decode_jpeg_plan for n files");
    if (out_bytes < H.out_bytes) return bad("vti_decode_jpeg: dev_out smaller than out_byte_offsets[n]");
    VTI_TRY(scratch_check("vti_decode_jpeg", c, scratch, scratch_bytes, H.scratch_bytes, "the plan's scratch_bytes"));
    size_t scratch_at = 0;
    long long out_at = 0;
    for (int32_t k = 0; k < n; ++k) {
        JpegDecRow R;
        memcpy(&R, (const uint8_t*)host_table + sizeof H + (size_t)k * sizeof R, sizeof R);
        std::string why;
        if (!decode_jpeg_row_ok(R, H, scratch_at, why) || R.out_off < out_at)
            return bad("vti_decode_jpeg: row " + std::to_string(k) + " of the table is invalid (" + (why.empty() ? "frames overlap" : why) + ")");
        out_at = R.out_off + 3LL * R.H0 * R.W0;
    }
    VTI_TRY(check_device(c, "vti_decode_jpeg"));
    VTI_HIP(c, launch_decode_jpeg(files, host_table, dev_table, n, rgb, out, info, scratch, (hipStream_t)stream), "decode_jpeg kernels");
    return VTI_OK;
}

// ---- raw camera frames -> BGR / RGB ----------------------------------------------------------------------------------------------
int64_t vti_raw_frame_bytes(int32_t fmt, int32_t H0, int32_t W0) { return raw::frame_bytes(fmt, H0, W0); }

static const char* raw_frame_error(int32_t fmt, int32_t H0, int32_t W0) {
    if (fmt < 0 || fmt >= kRawFormats) return "fmt must be one of VTI_RAW_YUYV .. VTI_RAW_YV12";
    if (H0 < 2 || W0 < 2 || H0 > kRawMaxSide || W0 > kRawMaxSide) return "H0 and W0 must be in 2..8192";
    if (W0 & 1) return "W0 must be even";
    if (raw::fmt_420(fmt) && (H0 & 1)) return "H0 must be even for a 4:2:0 format";
    return nullptr;
}

int32_t vti_convert_raw(vti_ctx* c, const uint8_t* raw_buf, int32_t fmt, int32_t B, int32_t H0, int32_t W0, int32_t rgb, uint8_t* frames,
                        void* stream) {
    // every check comes before the first HIP call
    auto bad = [&](const std::string& what) { return fail(c, VTI_ERR_ARG, what); };
    if (!c) return bad("vti_convert_raw: null ctx");
    if (const char* e = raw_frame_error(fmt, H0, W0)) return bad(std::string("vti_convert_raw: ") + e);
    if (B < 1 || B > kRawMaxFrames) return bad("vti_convert_raw: 1 <= B <= 4096");
    if (rgb != 0 && rgb != 1) return bad("vti_convert_raw: rgb 0 or 1");
    if (!raw_buf || !frames) return bad("vti_convert_raw: null pointer");
    if (int32_t drc = check_device(c, "vti_convert_raw")) return drc;
    VTI_HIP(c, launch_convert_raw(raw_buf, fmt, B, H0, W0, rgb, frames, (hipStream_t)stream), "convert_raw kernel");
    return VTI_OK;
}

int64_t vti_raw_table_bytes(int32_t n) {
    return n < 1 || n > kRawMaxFrames ? 0 : (int64_t)sizeof(RawTableHeader) + (int64_t)n * (int64_t)sizeof(RawRow);
}

int32_t vti_pack_raw_frames(vti_ctx* c, const int32_t* H0, const int32_t* W0, const int32_t* fmt, int32_t n, void* host_raw_table,
                            size_t nbytes, int64_t* out_raw_offsets) {
    auto bad = [&](const std::string& what) { return fail(c, VTI_ERR_ARG, what); };
    if (n < 1 || n > kRawMaxFrames) return bad("vti_pack_raw_frames: 1 <= n <= 4096");
    if (!H0 || !W0 || !fmt || !host_raw_table || !out_raw_offsets) return bad("vti_pack_raw_frames: null pointer");
    if ((int64_t)nbytes < vti_raw_table_bytes(n)) return bad("vti_pack_raw_frames: table smaller than vti_raw_table_bytes()");
    for (int32_t k = 0; k < n; ++k)
        if (const char* e = raw_frame_error(fmt[k], H0[k], W0[k]))
            return bad("vti_pack_raw_frames: frame " + std::to_string(k) + ": " + e);
    long long at = 0;
    for (int32_t k = 0; k < n; ++k) {
        RawRow r;
        memset(&r, 0, sizeof r);
        r.raw_off = at;
        r.raw_len = raw::frame_bytes(fmt[k], H0[k], W0[k]);
        r.H0 = H0[k]; r.W0 = W0[k]; r.fmt = fmt[k];
        memcpy((char*)host_raw_table + sizeof(RawTableHeader) + (size_t)k * sizeof r, &r, sizeof r);
        out_raw_offsets[k] = at;
        at = (at + r.raw_len + 15) & ~15LL;
    }
    out_raw_offsets[n] = at;
    RawTableHeader h;
    memset(&h, 0, sizeof h);
    h.magic = kRawTableMagic; h.n = n; h.raw_bytes = at;
    memcpy(host_raw_table, &h, sizeof h);
    return VTI_OK;
}

int32_t vti_convert_raw_frames(vti_ctx* c, const uint8_t* raw_buf, int64_t raw_bytes, const void* host_raw_table, const void* dev_raw_table,
                               const void* host_frame_table, const void* dev_frame_table, int32_t n, int32_t rgb, uint8_t* out,
                               int64_t out_bytes, void* stream) {
    // every check comes before the first HIP call
    auto bad = [&](const std::string& what) { return fail(c, VTI_ERR_ARG, what); };
    if (!c) return bad("vti_convert_raw_frames: null ctx");
    if (n < 1 || n > kRawMaxFrames) return bad("vti_convert_raw_frames: 1 <= n <= 4096");
    if (rgb != 0 && rgb != 1) return bad("vti_convert_raw_frames: rgb 0 or 1");
    if (!raw_buf || !host_raw_table || !dev_raw_table || !out) return bad("vti_convert_raw_frames: null pointer");
    if ((uintptr_t)dev_raw_table & 15) return bad("vti_convert_raw_frames: dev_raw_table must be 16-byte aligned");
    FrameTableHeader fh;
    if (int32_t rc = frames_check("vti_convert_raw_frames", c, host_frame_table, dev_frame_table, n, fh)) return rc;
    RawTableHeader h;
    memcpy(&h, host_raw_table, sizeof h);
    if (h.magic != kRawTableMagic || h.n != n || h.raw_bytes < 0)
        return bad("vti_convert_raw_frames: host_raw_table is not a table of vti_pack_raw_frames for n frames");
    if (raw_bytes < h.raw_bytes) return bad("vti_convert_raw_frames: raw_bytes smaller than out_raw_offsets[n]");
    if (out_bytes < fh.total_bytes) return bad("vti_convert_raw_frames: out_bytes smaller than the frame table's total_bytes");
    long long at = 0;
    int max_items = 1;
    for (int32_t b = 0; b < n; ++b) {
        RawRow r;
        memcpy(&r, (const char*)host_raw_table + sizeof h + (size_t)b * sizeof r, sizeof r);
        const char* e = raw_frame_error(r.fmt, r.H0, r.W0);
        if (!e && r.raw_len != raw::frame_bytes(r.fmt, r.H0, r.W0)) e = "raw_len is not the frame's size";
        if (!e && (r.raw_off < at || (r.raw_off & 15))) e = "raw offsets must ascend without overlap, each a multiple of 16";
        if (!e && (r.raw_off > h.raw_bytes || r.raw_len > h.raw_bytes - r.raw_off)) e = "the raw frame runs past the table's raw_bytes";
        if (e) return bad("vti_convert_raw_frames: row " + std::to_string(b) + " of host_raw_table is invalid (" + e + ")");
        const FrameRow f = table_row(host_frame_table, b);
        if (f.H0 != r.H0 || f.W0 != r.W0)
            return bad("vti_convert_raw_frames: frame " + std::to_string(b) + ": the raw table says " + std::to_string(r.H0) + "x" +
                       std::to_string(r.W0) + ", the frame table " + std::to_string(f.H0) + "x" + std::to_string(f.W0));
        at = r.raw_off + r.raw_len;
        max_items = std::max(max_items, raw::items_of(r.fmt, r.H0, r.W0));
    }
    if (int32_t drc = check_device(c, "vti_convert_raw_frames")) return drc;
    VTI_HIP(c, launch_convert_raw_frames(raw_buf, dev_raw_table, frame_rows(dev_frame_table), n, max_items, rgb, out, (hipStream_t)stream),
            "convert_raw_frames kernel");
    return VTI_OK;
}

// Where conv i's output lives, for vti_debug_conv_output and its inverse (one set of refusals): the view, its storage
// (elem: 1 f32, 2 h2 pairs, 0 fp16) and the buffer's address.
static int32_t conv_output_view(vti_ctx* c, const char* fn, int32_t i, int32_t B, const void* user, const View*& v, int& elem, void*& ptr) {
    int32_t rc = check_ready(c, B, fn);
    if (rc) return rc;
    if (i < 0 || i >= (int32_t)c->plan.convs.size() || !user) return refuse(c, fn, "bad argument");
    v = &c->plan.conv_out[i];
    if (v->buf < 0) return refuse(c, fn, "this conv is fused into the next one; its output is never materialised", VTI_ERR_UNSUPPORTED);
    const Buf& b = c->plan.bufs[v->buf];
    ptr = buf_ptr(c->plan, bindings_of(c, c->last_input, nullptr, c->last_proto, nullptr), v->buf);
    if (!ptr) return refuse(c, fn, "run vti_forward first", VTI_ERR_STATE);
    elem = (b.elem == EL_F32 || (b.elem == EL_T && c->plan.desc.dtype == VTI_F32)) ? 1
           : (b.elem == EL_T && c->plan.desc.dtype == VTI_H2) ? 2 : 0;      // 2: h2 pairs
    return VTI_OK;
}

int32_t vti_debug_conv_output(vti_ctx* c, int32_t i, int32_t B, float* out, void* stream) {
    const View* v; int elem; void* src;
    VTI_TRY(conv_output_view(c, "vti_debug_conv_output", i, B, out, v, elem, src));
    const Buf& b = c->plan.bufs[v->buf];
    VTI_HIP(c, launch_debug_nchw(elem, src, B, b.H, b.W, v->C, b.C, v->coff, out, (hipStream_t)stream), "debug copy");
    return VTI_OK;
}

int32_t vti_debug_set_conv_output(vti_ctx* c, int32_t i, int32_t B, const float* in, void* stream) {
    const View* v; int elem; void* dst;
    VTI_TRY(conv_output_view(c, "vti_debug_set_conv_output", i, B, in, v, elem, dst));
    const Buf& b = c->plan.bufs[v->buf];
    VTI_HIP(c, launch_debug_set_nchw(elem, in, B, b.H, b.W, v->C, b.C, v->coff, dst, (hipStream_t)stream), "debug copy");
    return VTI_OK;
}

int32_t vti_debug_run_op(vti_ctx* c, int32_t i, const uint8_t* input, int32_t B, int32_t swap_rb, float* pred, void* proto, float* best,
                         int32_t* out_convs, void* stream) {
    const char* fn = "vti_debug_run_op";
    if (!c) return VTI_ERR_ARG;
    const Plan& P = c->plan;
    if (i < 0 || i >= (int32_t)P.convs.size()) return refuse(c, fn, "i out of range (0..vti_num_convs - 1)");
    if (B < 1 || B > P.desc.max_batch) return refuse(c, fn, "B out of range (1..max_batch)");
    const Op* op = nullptr;
    for (const Op& o : P.ops)
        if ((o.kind == OP_CONV || o.kind == OP_CONV0) && (o.conv == i || o.fused == i || o.pair == i || o.tail == i || o.fold == i || o.fused_l1 == i))
            op = &o;
    if (!op) return refuse(c, fn, "no op of the plan computes this conv", VTI_ERR_UNSUPPORTED);
    // the convs of the op in execution order
    const int32_t order[4] = {op->fold >= 0 ? op->fold : op->conv, op->fold >= 0 ? op->conv : op->fused_l1 >= 0 ? op->fused_l1 : op->pair,
                              op->tail, op->fused};
    if (out_convs) {
        int n = 0;
        for (int k = 0; k < 4; ++k) out_convs[k] = -1;
        for (int k = 0; k < 4; ++k) if (order[k] >= 0) out_convs[n++] = order[k];
    }
    auto writes = [&](const View& v) { return v.buf >= 0 && v.buf == P.proto_buf_c; };
    if (op->kind == OP_CONV0 && !input) return refuse(c, fn, "dev_input is null and the op is the stem");
    if (op->pred_mode && !pred) return refuse(c, fn, "dev_pred is null and the op writes pred");
    if ((writes(op->out) || writes(op->out2)) && !proto) return refuse(c, fn, "dev_proto is null and the op writes proto");
    VTI_TRY(check_ready(c, B, fn));
    LaunchRec L;
    VTI_TRY(run_op(c, *op, B, swap_rb, bindings_of(c, input, pred, proto, best), (hipStream_t)stream, L));
    if (input) c->last_input = input;      // vti_debug_conv_output reads what the op wrote
    if (proto) c->last_proto = proto;
    return VTI_OK;
}

int32_t vti_debug_conv2d(int32_t dtype, const void* dev_in, int32_t B, int32_t H, int32_t W, int32_t in_ld, int32_t in_coff,
                         int32_t c1, const float* host_w, const float* host_b, int32_t c2, int32_t k, int32_t s, int32_t kind,
                         const void* dev_res, int32_t res_ld, int32_t res_coff, void* dev_out, int32_t out_ld, int32_t out_coff,
                         int32_t out_f32, int32_t swap_rb, int32_t tile_h, int32_t tile_w, int32_t waves_n, int32_t nrep,
                         int32_t iters, float* ms_out, int32_t* cfg_out, void* stream) {
    if (!dev_in || !host_w || !host_b || !dev_out || B < 1 || H < 1 || W < 1 || c1 < 1 || c2 < 1 || iters < 1)
        return fail(nullptr, VTI_ERR_ARG, "vti_debug_conv2d: bad argument");
    if ((dtype != VTI_F16 && dtype != VTI_F32 && dtype != VTI_H2) || (kind < 0 || kind > 2))
        return fail(nullptr, VTI_ERR_ARG, "vti_debug_conv2d: bad dtype/kind");
    const bool conv0 = (c1 == 3);   // u8 HWC3 input, the stem conv
    if (conv0 ? !(k == 3 && s == 2 && kind == 0) : (c1 % 16 != 0))
        return fail(nullptr, VTI_ERR_ARG, "vti_debug_conv2d: c1 must be 3 (stem) or a multiple of 16");
    if (!((k == 1 && s == 1) || (k == 3 && (s == 1 || s == 2)) || (kind == 2 && k == 2 && s == 2)))
        return fail(nullptr, VTI_ERR_ARG, "vti_debug_conv2d: unsupported kernel/stride");
    ConvRow r;
    r.name = "debug"; r.c1 = c1; r.c2 = c2; r.k = k; r.s = s; r.kind = kind; r.h_in = H; r.w_in = W;
    if (kind == 2) { r.h_out = 2 * H; r.w_out = 2 * W; }
    else { r.h_out = (H + 2 * (k / 2) - k) / s + 1; r.w_out = (W + 2 * (k / 2) - k) / s + 1; }
    const Options opt = options_from_env();       // no context here: the switches are read once per call
    ConvCfg g;
    choose_conv_cfg(opt.plan, dtype, r, conv0, B, g, tile_h, tile_w, waves_n, nrep);
    if (g.TH == 0) return fail(nullptr, VTI_ERR_ARG, "vti_debug_conv2d: no launch configuration fits");
    if (cfg_out) { cfg_out[0] = g.TH; cfg_out[1] = g.TW; cfg_out[2] = g.WN; cfg_out[3] = g.NREP; cfg_out[4] = (int32_t)g.lds * (g.pk ? -1 : 1); }   // negative LDS size = persistent kernel
    std::vector<uint8_t> wpk(packed_conv_bytes(r, conv0, g));
    std::vector<float> bias((size_t)g.ntiles_n * 16);
    float alpha = 1.f;
    pack_conv(dtype, r, conv0, g, host_w, host_b, wpk.data(), bias.data(), 0, &alpha);
    void* d_w = nullptr; float* d_b = nullptr;
    hipStream_t st = (hipStream_t)stream;
    VTI_HIP(nullptr, hipMalloc(&d_w, wpk.size()), "hipMalloc");
    hipError_t e = hipMalloc((void**)&d_b, bias.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_w, wpk.data(), wpk.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) {
        LaunchRec L;
        conv_record(opt.run, dtype, r, g, B, dev_in, in_ld, in_coff, dev_out, out_ld, out_coff, dev_res, res_ld, res_coff, d_w, d_b, alpha,
                    out_f32 != 0, swap_rb, L);
#ifdef VTI_STAMPS
        // diagnostic build: one stamped launch after a warm-up (caches, icache), medians of the phase intervals to stderr
        (void)issue(L, st);
        (void)issue(L, st, "");
#endif
        e = issue(L, st);   // warm-up / the checked run
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        for (int i = 1; i < iters && e == hipSuccess; ++i) e = issue(L, st);
        if (e == hipSuccess) e = hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        float ms = 0.f;
        if (e == hipSuccess && iters > 1) e = hipEventElapsedTime(&ms, e0, e1);
        if (ms_out) *ms_out = iters > 1 ? ms / (iters - 1) : 0.f;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(d_w);
    if (d_b) (void)hipFree(d_b);
    if (e != hipSuccess) return hip_fail(nullptr, e, "vti_debug_conv2d");
    return VTI_OK;
}

// ---- the non-GEMM kernels one at a time: every check on the host, then the one launch ----
int32_t vti_debug_sppf_pool(int32_t dtype, const void* dev_in, void* dev_out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t ld,
                            int32_t in_coff, int32_t out_coff, int32_t* path_out, void* stream) {
    auto bad = [](const std::string& m) { return fail(nullptr, VTI_ERR_ARG, "vti_debug_sppf_pool: " + m); };
    if (dtype != VTI_F16 && dtype != VTI_F32 && dtype != VTI_H2) return bad("bad dtype");
    if (!dev_in || !dev_out) return bad("null pointer");
    if (((uintptr_t)dev_in | (uintptr_t)dev_out) & 15) return bad("dev_in and dev_out must be 16-byte aligned");
    if (B < 1 || H < 1 || W < 1) return bad("B, H and W must be >= 1");
    const int vec = dtype == VTI_F16 ? 8 : 4, esize = 16 / vec;
    std::string e = slice_error("in", C, ld, in_coff, vec);
    if (e.empty() && (int64_t)3 * C > ld) e = "out: 3 C channels do not fit in ld = " + std::to_string(ld);
    if (e.empty()) e = slice_error("out", 3 * C, ld, out_coff, vec);
    if (!e.empty()) return bad(e);
    const int64_t elems = (int64_t)B * H * W * ld;
    if (elems > INT32_MAX) return bad("more than 2^31 - 1 elements");
    if (dev_in == dev_out) {
        if (in_coff < out_coff + 3 * C && out_coff < in_coff + C) return bad("the in and out slices overlap in the one buffer");
    } else if (ranges_overlap(dev_in, elems * esize, dev_out, elems * esize)) {
        return bad("dev_in and dev_out must be one buffer or two that do not overlap");
    }
    PoolParams p;
    p.in = dev_in; p.out = dev_out; p.B = B; p.H = H; p.W = W; p.C = C; p.ld = ld; p.in_coff = in_coff; p.out_coff = out_coff;
    if (path_out) *path_out = sppf_pool_path(dtype, H, W, C);
    const hipError_t he = launch_sppf_pool(dtype, p, (hipStream_t)stream);
    if (he != hipSuccess) return hip_fail(nullptr, he, "vti_debug_sppf_pool");
    return VTI_OK;
}

int32_t vti_debug_upsample2x(int32_t dtype, const void* dev_in, void* dev_out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_ld,
                             int32_t in_coff, int32_t out_ld, int32_t out_coff, void* stream) {
    auto bad = [](const std::string& m) { return fail(nullptr, VTI_ERR_ARG, "vti_debug_upsample2x: " + m); };
    if (dtype != VTI_F16 && dtype != VTI_F32 && dtype != VTI_H2) return bad("bad dtype");
    if (!dev_in || !dev_out) return bad("null pointer");
    if (((uintptr_t)dev_in | (uintptr_t)dev_out) & 15) return bad("dev_in and dev_out must be 16-byte aligned");
    if (B < 1 || H < 1 || W < 1) return bad("B, H and W must be >= 1");
    const int vec = dtype == VTI_F16 ? 8 : 4, esize = 16 / vec;
    std::string e = slice_error("in", C, in_ld, in_coff, vec);
    if (e.empty()) e = slice_error("out", C, out_ld, out_coff, vec);
    if (!e.empty()) return bad(e);
    const int64_t in_elems = (int64_t)B * H * W * in_ld, out_elems = (int64_t)B * H * W * 4 * out_ld;
    if (in_elems > INT32_MAX || out_elems > INT32_MAX) return bad("more than 2^31 - 1 elements");
    if (ranges_overlap(dev_in, in_elems * esize, dev_out, out_elems * esize)) return bad("dev_in and dev_out overlap");
    Up2Params p;
    p.in = dev_in; p.out = dev_out; p.B = B; p.H = H; p.W = W; p.C = C; p.in_ld = in_ld; p.in_coff = in_coff; p.out_ld = out_ld; p.out_coff = out_coff;
    const hipError_t he = launch_upsample2x(dtype, p, (hipStream_t)stream);
    if (he != hipSuccess) return hip_fail(nullptr, he, "vti_debug_upsample2x");
    return VTI_OK;
}

int32_t vti_debug_decode(int32_t box_only, const float* const* dev_box, const float* const* dev_cls, const float* const* dev_mc,
                         const int32_t* H, const int32_t* W, const int32_t* stride, int32_t B, int32_t nc, int32_t nm, float* dev_pred,
                         void* stream) {
    auto bad = [](const std::string& m) { return fail(nullptr, VTI_ERR_ARG, "vti_debug_decode: " + m); };
    if (box_only != 0 && box_only != 1) return bad("box_only must be 0 or 1");
    if (!dev_box || !H || !W || !stride || !dev_pred || (!box_only && (!dev_cls || !dev_mc))) return bad("null pointer");
    if (B < 1 || nc < 1 || nm < 1) return bad("B, nc and nm must be >= 1");
    if (!box_only && nc + (int64_t)nm > VTI_DECODE_MAX_CHANNELS)
        return bad("nc + nm = " + std::to_string(nc + (int64_t)nm) + " is above VTI_DECODE_MAX_CHANNELS = " +
                   std::to_string(VTI_DECODE_MAX_CHANNELS) + ", the most the full decode kernel takes");
    DecodeParams p;
    int64_t A = 0;
    uintptr_t align = (uintptr_t)dev_pred;
    for (int l = 0; l < 3; ++l) {
        if (H[l] < 1 || W[l] < 1 || stride[l] < 1) return bad("level " + std::to_string(l) + ": H, W and stride must be >= 1");
        if (!dev_box[l] || (!box_only && (!dev_cls[l] || !dev_mc[l]))) return bad("level " + std::to_string(l) + ": null pointer");
        p.box[l] = dev_box[l]; p.cls[l] = box_only ? nullptr : dev_cls[l]; p.mc[l] = box_only ? nullptr : dev_mc[l];
        align |= (uintptr_t)p.box[l] | (uintptr_t)p.cls[l] | (uintptr_t)p.mc[l];
        p.H[l] = H[l]; p.W[l] = W[l]; p.stride[l] = stride[l]; p.a0[l] = (int)A;
        A += (int64_t)H[l] * W[l];
        if (A > INT32_MAX) return bad("more than 2^31 - 1 values in pred");
    }
    if (align & 3) return bad("every pointer must be 4-byte aligned");
    if ((int64_t)B * A * (4 + (int64_t)nc + nm) > INT32_MAX || (int64_t)B * A * 64 > INT32_MAX) return bad("more than 2^31 - 1 values in pred");
    p.B = B; p.A = (int)A; p.nc = nc; p.nm = nm; p.reg_max = 16; p.pred = dev_pred;
    const hipError_t he = box_only ? launch_box_decode(p, (hipStream_t)stream) : launch_decode(p, (hipStream_t)stream);
    if (he != hipSuccess) return hip_fail(nullptr, he, "vti_debug_decode");
    return VTI_OK;
}

}  // extern "C"
