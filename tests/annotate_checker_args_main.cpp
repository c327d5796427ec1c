// Stand-alone program (its own main; never loaded into Python): calls every argument check of vti_annotate_checker with fake device
// pointers that are never dereferenced and expects VTI_ERR_ARG with a message that names the function and the argument; then a few
// refusals of vti_measure_checker and vti_overlay_frames, which make the same checks through the same helpers (the selection walk of
// vti_overlay_frames reads two host tables).  Every call is refused, so none reaches a HIP call and the program may run anywhere.
// Built with -fsanitize=address,undefined and linked against libvti.so by tests/test_annotate_checker_abi.py; prints
// "ok <number of refusals>" and returns 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vti.h"

struct Call {
    vti_ctx* ctx;
    const uint8_t* frames; int32_t B, H0, W0;
    const vti_checker_params* params;
    const uint8_t* masks; int32_t native;
    const float* dets; const float* xyxy; const int32_t* counts; const int32_t* offsets;
    int32_t max_det, capacity;
    const int32_t* frame_i32; const double* stitch_f64; const int32_t* stitch_i32;
    const int32_t* host_select; const int32_t* dev_select; int32_t n_sel, max_points;
    uint8_t* out; int32_t* status; void* scratch; size_t scratch_bytes;
};

static int32_t run(const Call& c) {
    return vti_annotate_checker(c.ctx, c.frames, c.B, c.H0, c.W0, c.params, c.masks, c.native, c.dets, c.xyxy, c.counts, c.offsets,
                                c.max_det, c.capacity, c.frame_i32, c.stitch_f64, c.stitch_i32, c.host_select, c.dev_select, c.n_sel,
                                c.max_points, c.out, c.status, c.scratch, c.scratch_bytes, nullptr);
}

static int failures = 0, refusals = 0;

// rc is VTI_ERR_ARG and the message of ctx (if any) begins with "<fn>:" and holds needle (if any)
static void expect(int32_t rc, vti_ctx* ctx, const char* fn, const char* what, const char* needle) {
    const char* msg = ctx ? vti_last_error(ctx) : "";
    const size_t n = strlen(fn);
    const bool ok = rc == VTI_ERR_ARG && (!ctx || (strncmp(msg, fn, n) == 0 && msg[n] == ':' && (!needle || strstr(msg, needle))));
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s: rc %d, message \"%s\"\n", what, rc, msg); }
    ++refusals;
}

static void refused(const Call& c, const char* what, const char* needle) { expect(run(c), c.ctx, "vti_annotate_checker", what, needle); }

int main() {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = 'n'; d.nc = 2; d.nm = 32; d.reg_max = 16; d.H = 736; d.W = 960; d.max_batch = 4; d.dtype = 0;
    vti_ctx* ctx = nullptr;
    if (vti_create(&d, &ctx) != VTI_OK || !ctx) { fprintf(stderr, "vti_create failed\n"); return 2; }

    vti_checker_params p;
    memset(&p, 0, sizeof p);
    p.K[0] = p.K[4] = 1000.0; p.K[2] = 640.0; p.K[5] = 480.0; p.K[8] = 1.0;
    p.R[0] = p.R[4] = p.R[8] = 1.0; p.t[2] = 1.0;
    p.max_px_distance = 150.0; p.stitch_id = 0; p.fabric_id = 1; p.min_stitches = 3; p.envelope_neighborhood = 3;
    p.kmeans_iters = 10; p.frame_buffer = 8;

    const int32_t B = 4, H0 = 960, W0 = 1280, max_det = 200, n_sel = 3, max_points = 4096;
    const int64_t need = vti_annotate_scratch_bytes(ctx, n_sel, max_det, H0, W0, max_points);
    if (need <= 0) { fprintf(stderr, "vti_annotate_scratch_bytes gave %lld\n", (long long)need); return 2; }
    std::vector<int32_t> sel = {3, 0, 3};           // exactly n_sel entries on the heap: a read past them is the sanitizer's to report
    void* const one = (void*)(uintptr_t)4096;       // fake device pointers, never dereferenced
    void* const ws = (void*)(uintptr_t)(1 << 20);
    const Call good = {ctx, (const uint8_t*)one, B, H0, W0, &p, (const uint8_t*)one, 0, (const float*)one, (const float*)one,
                       (const int32_t*)one, (const int32_t*)one, max_det, 800, (const int32_t*)one, (const double*)one,
                       (const int32_t*)one, sel.data(), (const int32_t*)one, n_sel, max_points, (uint8_t*)one, (int32_t*)one, ws,
                       (size_t)need};
    Call c;
#define REFUSED(change, needle) do { c = good; change; refused(c, #change, needle); } while (0)
    REFUSED(c.ctx = nullptr, nullptr);
    REFUSED(c.params = nullptr, "null");
    REFUSED(c.frames = nullptr, "null pointer");
    REFUSED(c.masks = nullptr, "null pointer");
    REFUSED(c.dets = nullptr, "null pointer");
    REFUSED(c.xyxy = nullptr, "null pointer");
    REFUSED(c.counts = nullptr, "null pointer");
    REFUSED(c.offsets = nullptr, "null pointer");
    REFUSED(c.frame_i32 = nullptr, "null pointer");
    REFUSED(c.stitch_f64 = nullptr, "null pointer");
    REFUSED(c.stitch_i32 = nullptr, "null pointer");
    REFUSED(c.host_select = nullptr, "null pointer");
    REFUSED(c.dev_select = nullptr, "null pointer");
    REFUSED(c.out = nullptr, "null pointer");
    REFUSED(c.status = nullptr, "null pointer");
    REFUSED(c.scratch = nullptr, "scratch");
    REFUSED(c.n_sel = 0, "bad size");
    REFUSED(c.n_sel = -2, "bad size");
    REFUSED(c.B = 0, "bad size");
    REFUSED(c.capacity = -1, "bad size");
    REFUSED(c.native = 2, "bad size");
    REFUSED(c.max_det = 0, "bad size");
    REFUSED(c.max_det = VTI_MEASURE_MAX_DET + 1, "VTI_MEASURE_MAX_DET");
    REFUSED(c.H0 = 8193, "8192");
    REFUSED(c.W0 = 0, "bad size");
    REFUSED(c.max_points = -1, "bad size");
    std::vector<int32_t> low = {0, -1, 1}, high = {0, 1, B};
    REFUSED(c.host_select = low.data(), "host_select[1] = -1");
    REFUSED(c.host_select = high.data(), "host_select[2] = 4");
    REFUSED(c.dev_select = (const int32_t*)(uintptr_t)(4096 + 2), "aligned");
    REFUSED(c.masks = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte");
    REFUSED((c.native = 1, c.masks = (const uint8_t*)(uintptr_t)(4096 + 4)), "8-byte");
    REFUSED(c.stitch_f64 = (const double*)(uintptr_t)(4096 + 4), "misaligned");
    REFUSED(c.scratch = (void*)(uintptr_t)((1 << 20) + 64), "256-byte aligned");
    REFUSED(c.scratch_bytes = (size_t)need - 1, "scratch smaller");
    vti_checker_params q;
#define BAD_PARAMS(change, needle) do { q = p; change; c = good; c.params = &q; refused(c, #change, needle); } while (0)
    BAD_PARAMS(q.fabric_id = q.stitch_id, "stitch_id and fabric_id");
    BAD_PARAMS(q.stitch_id = -1, "stitch_id and fabric_id");
    BAD_PARAMS(q.envelope_neighborhood = 65, "envelope_neighborhood");
    BAD_PARAMS(q.envelope_neighborhood = -1, "envelope_neighborhood");
    BAD_PARAMS(q.min_stitches = 0, "bad setting");
    BAD_PARAMS(q.drop_empty = 2, "bad setting");
    BAD_PARAMS(q.frame_buffer = 0, "bad setting");
    BAD_PARAMS(q.max_px_distance = __builtin_nan(""), "NaN");

    // vti_measure_checker: the measurement's checks of the same settings, masks and scratch
    const int64_t mneed = vti_measure_scratch_bytes(ctx, B, 800, W0);
    auto measure = [&](const vti_checker_params* pp, const void* masks, int32_t md, void* scratch, size_t nbytes) {
        return vti_measure_checker(ctx, pp, (const uint8_t*)masks, 0, (const float*)one, (const float*)one, (const int32_t*)one,
                                   (const int32_t*)one, B, md, 800, H0, W0, scratch, nbytes, (double*)one, (int32_t*)one, (double*)one,
                                   (int32_t*)one, nullptr);
    };
    q = p; q.frame_buffer = 0;
    expect(measure(&q, one, max_det, ws, (size_t)mneed), ctx, "vti_measure_checker", "frame_buffer = 0", "bad setting");
    expect(measure(&p, (void*)(uintptr_t)(4096 + 8), max_det, ws, (size_t)mneed), ctx, "vti_measure_checker", "masks + 8", "16-byte");
    expect(measure(&p, one, VTI_MEASURE_MAX_DET + 1, ws, (size_t)mneed), ctx, "vti_measure_checker", "max_det", "VTI_MEASURE_MAX_DET");
    expect(measure(&p, one, max_det, ws, (size_t)mneed - 1), ctx, "vti_measure_checker", "short scratch", "scratch smaller");

    // vti_overlay_frames: the walk over the selection reads host_select and a row of each host table per entry
    const int32_t fh[4] = {960, 481, 720, 1080}, fw[4] = {1280, 333, 960, 1920};
    std::vector<int32_t> oh, ow;
    for (int32_t b : sel) { oh.push_back(fh[b]); ow.push_back(fw[b]); }
    auto pack = [&](const int32_t* h, const int32_t* w, int32_t n, std::vector<uint8_t>& table) {
        std::vector<int64_t> at;
        int64_t total = 0;
        for (int32_t k = 0; k < n; ++k) { at.push_back(total); total = (total + 3LL * h[k] * w[k] + 15) & ~15LL; }
        table.resize((size_t)vti_frame_table_bytes(n));     // exactly the table's bytes on the heap
        return vti_pack_frames(ctx, d.H, d.W, h, w, at.data(), n, total, table.data(), table.size());
    };
    std::vector<uint8_t> t_in, t_out;
    if (pack(fh, fw, 4, t_in) != VTI_OK || pack(oh.data(), ow.data(), n_sel, t_out) != VTI_OK) { fprintf(stderr, "vti_pack_frames failed\n"); return 2; }
    const int64_t oneed = vti_overlay_frames_scratch_bytes(ctx, t_out.data(), max_det, max_points);
    if (oneed <= 0) { fprintf(stderr, "vti_overlay_frames_scratch_bytes gave %lld\n", (long long)oneed); return 2; }
    const uint8_t palette[18] = {0};
    auto overlay = [&](const int32_t* hsel, const void* masks, size_t nbytes) {
        return vti_overlay_frames(ctx, (const uint8_t*)one, t_in.data(), one, B, (const uint8_t*)masks, 0, nullptr, 0, (const float*)one,
                                  (const float*)one, (const int32_t*)one, (const int32_t*)one, max_det, 800, nullptr, palette, 6, 0.3f, 0.7f,
                                  hsel, (const int32_t*)one, n_sel, VTI_OVERLAY_BOTH, nullptr, max_points, t_out.data(), one, (uint8_t*)one,
                                  (int32_t*)one, ws, nbytes, nullptr);
    };
    std::vector<int32_t> past = {3, 0, B}, other = {3, 1, 3};
    expect(overlay(past.data(), one, (size_t)oneed), ctx, "vti_overlay_frames", "host_select[2] = B", "host_select[2] = 4");
    expect(overlay(other.data(), one, (size_t)oneed), ctx, "vti_overlay_frames", "frame 1 for row 1", "row 1 of the out table");
    expect(overlay(sel.data(), (void*)(uintptr_t)(4096 + 8), (size_t)oneed), ctx, "vti_overlay_frames", "masks + 8", "16-byte");
    expect(overlay(sel.data(), one, (size_t)oneed - 1), ctx, "vti_overlay_frames", "short scratch", "scratch smaller");

    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", refusals);
    return 0;
}
