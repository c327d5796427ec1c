// Stand-alone program (its own main; never loaded into Python): repeats the refusals of the stitch-distance checker's rig forms --
// vti_checker_pack_cameras, vti_measure_checker_cameras / _frames / _frames_native, vti_annotate_checker_cameras / _frames -- with
// fake device pointers that are never dereferenced, and expects the status and a message that begins with the function's name and
// names the argument.  The table walks read the host tables row by row and the packer writes exactly the table's bytes: both are
// heap blocks of exactly that size, so a read or write past them is the sanitizer's to report.  Every call is refused, so none
// reaches a HIP call and the program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so by
// tests/test_checker_rig_abi.py; prints "ok <number of refusals>" and returns 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vti.h"

static int failures = 0, refusals = 0;

// rc is `want` and the message of ctx begins with "<fn>" and holds needle (if any)
static void expect(int32_t rc, int32_t want, vti_ctx* ctx, const char* fn, const char* what, const char* needle) {
    const char* msg = vti_last_error(ctx);
    const bool ok = rc == want && strncmp(msg, fn, strlen(fn)) == 0 && (!needle || strstr(msg, needle));
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s %s: rc %d, message \"%s\"\n", fn, what, rc, msg); }
    ++refusals;
}

struct Measure {            // the arguments the three measurement calls share
    const void* cameras; int32_t n_cams; const int32_t* index; const uint8_t* masks; int32_t native;
    const int64_t* bases; int64_t capacity_bytes;
    const float* dets; const void* host_table; const void* dev_table; int32_t B, max_det, capacity;
    void* scratch; size_t scratch_bytes; double* frame_f64;
};

struct Picture {            // the arguments the two drawing calls share
    const uint8_t* frames; const void* host_table; const void* dev_table; int32_t B, H0, W0;
    const void* cameras; int32_t n_cams; const int32_t* index; const uint8_t* masks; int32_t native;
    const float* dets; int32_t max_det, capacity; const double* stitch_f64;
    const int32_t* host_select; const int32_t* dev_select; int32_t n_sel, max_points;
    const void* host_out_table; const void* dev_out_table; uint8_t* out; void* scratch; size_t scratch_bytes;
};

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

    // ---- the packer: exactly n rows are read and exactly the table's bytes written
    const int32_t n_cams = 3;
    const size_t row = (size_t)vti_measure_cameras_bytes(1);
    std::vector<vti_checker_params> list(n_cams, p);
    list[1].stitch_id = 1; list[1].fabric_id = 0; list[2].drop_empty = 1;
    std::vector<uint8_t> t1(row * n_cams, 0xA5), t2(row * n_cams, 0x5A);
    if (vti_checker_pack_cameras(ctx, list.data(), n_cams, t1.data(), t1.size()) != VTI_OK ||
        vti_checker_pack_cameras(ctx, list.data(), n_cams, t2.data(), t2.size()) != VTI_OK || t1 != t2) {
        fprintf(stderr, "vti_checker_pack_cameras: not deterministic\n");
        return 2;
    }
    const char* pk = "vti_checker_pack_cameras:";
    expect(vti_checker_pack_cameras(ctx, nullptr, n_cams, t1.data(), t1.size()), VTI_ERR_ARG, ctx, pk, "null list", "null list");
    expect(vti_checker_pack_cameras(ctx, list.data(), n_cams, nullptr, t1.size()), VTI_ERR_ARG, ctx, pk, "null table", "null list or table");
    expect(vti_checker_pack_cameras(ctx, list.data(), 0, t1.data(), t1.size()), VTI_ERR_ARG, ctx, pk, "n_cams 0", "n_cams < 1");
    expect(vti_checker_pack_cameras(ctx, list.data(), n_cams, t1.data(), t1.size() - 1), VTI_ERR_ARG, ctx, pk, "short table",
           "vti_measure_cameras_bytes");
    for (int32_t k = 0; k < n_cams; ++k) {
        char where[32];
        snprintf(where, sizeof where, "camera %d:", k);
        std::vector<vti_checker_params> bad = list;
        bad[k].envelope_neighborhood = 65;
        expect(vti_checker_pack_cameras(ctx, bad.data(), n_cams, t2.data(), t2.size()), VTI_ERR_ARG, ctx, pk, "neighbourhood 65", where);
        bad = list; bad[k].fabric_id = bad[k].stitch_id;
        expect(vti_checker_pack_cameras(ctx, bad.data(), n_cams, t2.data(), t2.size()), VTI_ERR_ARG, ctx, pk, "equal ids", where);
        bad = list; bad[k].min_stitches = 0;
        expect(vti_checker_pack_cameras(ctx, bad.data(), n_cams, t2.data(), t2.size()), VTI_ERR_ARG, ctx, pk, "min_stitches 0", where);
        bad = list; bad[k].frame_buffer = 0;
        expect(vti_checker_pack_cameras(ctx, bad.data(), n_cams, t2.data(), t2.size()), VTI_ERR_ARG, ctx, pk, "frame_buffer 0", where);
        bad = list; bad[k].max_px_distance = __builtin_nan("");
        expect(vti_checker_pack_cameras(ctx, bad.data(), n_cams, t2.data(), t2.size()), VTI_ERR_ARG, ctx, pk, "NaN", where);
    }
    if (t1 != t2) { fprintf(stderr, "a refused pack wrote into the table\n"); return 2; }

    // ---- the frame tables: exactly their bytes on the heap
    const int32_t B = 4, max_det = 200, capacity = 800, n_sel = 3, max_points = 4096;
    const int32_t fh[4] = {960, 481, 720, 1080}, fw[4] = {1280, 333, 960, 1920};
    std::vector<int32_t> sel = {3, 0, 3}, oh, ow;
    for (int32_t b : sel) { oh.push_back(fh[b]); ow.push_back(fw[b]); }
    auto pack = [&](const int32_t* h, const int32_t* w, int32_t n, std::vector<uint8_t>& table) {
        std::vector<int64_t> at;
        int64_t total = 0;
        for (int32_t k = 0; k < n; ++k) { at.push_back(total); total = (total + 3LL * h[k] * w[k] + 15) & ~15LL; }
        table.resize((size_t)vti_frame_table_bytes(n));
        return vti_pack_frames(ctx, d.H, d.W, h, w, at.data(), n, total, table.data(), table.size());
    };
    std::vector<uint8_t> t_in, t_out, t_three;
    if (pack(fh, fw, 4, t_in) != VTI_OK || pack(oh.data(), ow.data(), n_sel, t_out) != VTI_OK || pack(fh, fw, 3, t_three) != VTI_OK) {
        fprintf(stderr, "vti_pack_frames failed\n");
        return 2;
    }
    std::vector<uint8_t> t_bad = t_in;
    t_bad[64 + 2 * 64] = 1;                         // row 2's byte offset is no longer a multiple of 16

    void* const one = (void*)(uintptr_t)4096;       // fake device pointers, never dereferenced
    void* const ws = (void*)(uintptr_t)(1 << 20);
    const float* const f = (const float*)one;
    const int32_t* const i = (const int32_t*)one;

    // ---- the three measurement calls
    const int64_t mneed = vti_measure_scratch_bytes(ctx, B, capacity, 1920);
    const Measure mgood = {one, n_cams, i, (const uint8_t*)one, 0, (const int64_t*)one, 1 << 20, f, t_in.data(), one, B, max_det, capacity,
                           ws, (size_t)mneed, (double*)one};
    auto cameras = [&](const Measure& m) {
        return vti_measure_checker_cameras(ctx, m.cameras, m.n_cams, m.index, m.masks, m.native, m.dets, f, i, i, m.B, m.max_det, m.capacity,
                                           1080, 1920, m.scratch, m.scratch_bytes, m.frame_f64, (int32_t*)one, nullptr, nullptr, nullptr);
    };
    auto frames = [&](const Measure& m) {
        return vti_measure_checker_frames(ctx, m.cameras, m.n_cams, m.index, m.masks, m.native, m.dets, f, i, i, m.host_table, m.dev_table,
                                          m.B, m.max_det, m.capacity, m.scratch, m.scratch_bytes, m.frame_f64, (int32_t*)one, nullptr,
                                          nullptr, nullptr);
    };
    auto ragged = [&](const Measure& m) {
        return vti_measure_checker_frames_native(ctx, m.cameras, m.n_cams, m.index, m.masks, m.bases, m.capacity_bytes, m.dets, f, i, i,
                                                 m.host_table, m.dev_table, m.B, m.max_det, m.capacity, m.scratch, m.scratch_bytes,
                                                 m.frame_f64, (int32_t*)one, nullptr, nullptr, nullptr);
    };
    Measure m;
#define MEASURE(call, fn, change, needle) do { m = mgood; change; expect(call(m), VTI_ERR_ARG, ctx, fn, #change, needle); } while (0)
#define EVERY_MEASURE(change, needle) do { MEASURE(cameras, "vti_measure_checker_cameras:", change, needle); \
                                            MEASURE(frames, "vti_measure_checker_frames:", change, needle); \
                                            MEASURE(ragged, "vti_measure_checker_frames_native:", change, needle); } while (0)
    EVERY_MEASURE(m.cameras = nullptr, "null ctx, camera table or camera index");
    EVERY_MEASURE(m.index = nullptr, "null ctx, camera table or camera index");
    EVERY_MEASURE(m.n_cams = 0, "n_cams");
    EVERY_MEASURE(m.cameras = (void*)(uintptr_t)(4096 + 8), "16-byte aligned");
    EVERY_MEASURE(m.index = (const int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    EVERY_MEASURE(m.max_det = VTI_MEASURE_MAX_DET + 1, "VTI_MEASURE_MAX_DET");
    EVERY_MEASURE(m.max_det = 0, "bad shape");
    EVERY_MEASURE(m.dets = nullptr, "null pointer");
    EVERY_MEASURE(m.masks = nullptr, "null pointer");
    EVERY_MEASURE(m.frame_f64 = nullptr, "null pointer");
    EVERY_MEASURE(m.scratch = (void*)(uintptr_t)((1 << 20) + 64), "256-byte aligned");
    EVERY_MEASURE(m.scratch_bytes = (size_t)mneed - 1, "scratch smaller");
    MEASURE(cameras, "vti_measure_checker_cameras:", m.masks = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte");
    MEASURE(cameras, "vti_measure_checker_cameras:", (m.native = 1, m.masks = (const uint8_t*)(uintptr_t)(4096 + 4)), "8-byte");
    MEASURE(cameras, "vti_measure_checker_cameras:", m.native = 2, "bad shape");
    MEASURE(frames, "vti_measure_checker_frames:", m.masks = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte");
    MEASURE(ragged, "vti_measure_checker_frames_native:", m.masks = (const uint8_t*)(uintptr_t)(4096 + 4), "8-byte");
    MEASURE(ragged, "vti_measure_checker_frames_native:", m.bases = nullptr, "null dev_mask_bases");
    MEASURE(ragged, "vti_measure_checker_frames_native:", m.bases = (const int64_t*)(uintptr_t)(4096 + 4), "8-byte aligned");
    MEASURE(ragged, "vti_measure_checker_frames_native:", m.capacity_bytes = -1, "capacity_bytes");
#define EITHER_TABLE(change, needle) do { MEASURE(frames, "vti_measure_checker_frames:", change, needle); \
                                           MEASURE(ragged, "vti_measure_checker_frames_native:", change, needle); } while (0)
    EITHER_TABLE(m.host_table = nullptr, nullptr);
    EITHER_TABLE(m.dev_table = nullptr, nullptr);
    EITHER_TABLE(m.host_table = t_three.data(), "another B");
    EITHER_TABLE(m.host_table = t_bad.data(), "frame 2 of host_table");
    m = mgood; m.native = 1;
    expect(frames(m), VTI_ERR_UNSUPPORTED, ctx, "vti_measure_checker_frames:", "native = 1", "native masks need frames of one size");

    // ---- the two drawing calls
    const int64_t need_c = vti_annotate_scratch_bytes(ctx, n_sel, max_det, 960, 1280, max_points);
    const int64_t need_f = vti_annotate_frames_scratch_bytes(ctx, t_out.data(), max_det, max_points);
    if (need_c <= 0 || need_f <= 0) { fprintf(stderr, "scratch queries gave %lld, %lld\n", (long long)need_c, (long long)need_f); return 2; }
    const Picture pgood = {(const uint8_t*)one, t_in.data(), one, B, 960, 1280, one, n_cams, i, (const uint8_t*)one, 0, f, max_det, capacity,
                           (const double*)one, sel.data(), i, n_sel, max_points, t_out.data(), one, (uint8_t*)one, ws, 0};
    auto draw_cameras = [&](Picture q) {
        if (!q.scratch_bytes) q.scratch_bytes = (size_t)need_c;
        return vti_annotate_checker_cameras(ctx, q.frames, q.B, q.H0, q.W0, q.cameras, q.n_cams, q.index, q.masks, q.native, q.dets, f, i, i,
                                            q.max_det, q.capacity, i, q.stitch_f64, i, q.host_select, q.dev_select, q.n_sel, q.max_points,
                                            q.out, (int32_t*)one, q.scratch, q.scratch_bytes, nullptr);
    };
    auto draw_frames = [&](Picture q) {
        if (!q.scratch_bytes) q.scratch_bytes = (size_t)need_f;
        return vti_annotate_checker_frames(ctx, q.frames, q.host_table, q.dev_table, q.B, q.cameras, q.n_cams, q.index, q.masks, q.native,
                                           q.dets, f, i, i, q.max_det, q.capacity, i, q.stitch_f64, i, q.host_select, q.dev_select, q.n_sel,
                                           q.max_points, q.host_out_table, q.dev_out_table, q.out, (int32_t*)one, q.scratch,
                                           q.scratch_bytes, nullptr);
    };
    Picture q;
#define PICTURE(call, fn, change, needle) do { q = pgood; change; expect(call(q), VTI_ERR_ARG, ctx, fn, #change, needle); } while (0)
#define BOTH_PICTURES(change, needle) do { PICTURE(draw_cameras, "vti_annotate_checker_cameras:", change, needle); \
                                            PICTURE(draw_frames, "vti_annotate_checker_frames:", change, needle); } while (0)
    std::vector<int32_t> low = {3, -1, 3}, high = {3, 0, B}, other = {3, 1, 3};
    BOTH_PICTURES(q.frames = nullptr, "null pointer");
    BOTH_PICTURES(q.cameras = nullptr, "null pointer");
    BOTH_PICTURES(q.masks = nullptr, "null pointer");
    BOTH_PICTURES(q.dets = nullptr, "null pointer");
    BOTH_PICTURES(q.stitch_f64 = nullptr, "null pointer");
    BOTH_PICTURES(q.host_select = nullptr, "null pointer");
    BOTH_PICTURES(q.dev_select = nullptr, "null pointer");
    BOTH_PICTURES(q.out = nullptr, "null pointer");
    BOTH_PICTURES(q.n_cams = 0, "bad size");
    BOTH_PICTURES(q.max_det = VTI_MEASURE_MAX_DET + 1, "bad size");
    BOTH_PICTURES(q.capacity = -1, "bad size");
    BOTH_PICTURES(q.max_points = -1, "bad size");
    BOTH_PICTURES(q.native = 2, "bad size");
    BOTH_PICTURES(q.host_select = low.data(), "host_select[1] = -1");
    BOTH_PICTURES(q.host_select = high.data(), "host_select[2] = 4");
    BOTH_PICTURES(q.cameras = (void*)(uintptr_t)(4096 + 8), "16-byte aligned");
    BOTH_PICTURES(q.index = (const int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    BOTH_PICTURES(q.masks = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte");
    BOTH_PICTURES(q.stitch_f64 = (const double*)(uintptr_t)(4096 + 4), "misaligned");
    BOTH_PICTURES(q.scratch = (void*)(uintptr_t)((1 << 20) + 64), "256-byte aligned");
    PICTURE(draw_cameras, "vti_annotate_checker_cameras:", q.scratch_bytes = (size_t)need_c - 1, "scratch smaller");
    PICTURE(draw_cameras, "vti_annotate_checker_cameras:", q.H0 = 8193, "8192");
    PICTURE(draw_cameras, "vti_annotate_checker_cameras:", q.n_sel = 0, "bad size");
    PICTURE(draw_cameras, "vti_annotate_checker_cameras:", (q.native = 1, q.masks = (const uint8_t*)(uintptr_t)(4096 + 4)), "8-byte");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.scratch_bytes = (size_t)need_f - 1, "scratch smaller");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.host_table = t_three.data(), "another B");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.host_table = t_bad.data(), "frame 2 of host_table");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.dev_table = nullptr, nullptr);
    PICTURE(draw_frames, "vti_annotate_checker_frames (out table):", q.host_out_table = t_in.data(), "another B");
    PICTURE(draw_frames, "vti_annotate_checker_frames (out table):", q.dev_out_table = nullptr, nullptr);
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.n_sel = 0, "n_sel");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.host_select = other.data(), "row 1 of the out table");
    PICTURE(draw_frames, "vti_annotate_checker_frames:", q.frames = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte aligned");
    q = pgood; q.native = 1;
    expect(draw_frames(q), VTI_ERR_UNSUPPORTED, ctx, "vti_annotate_checker_frames:", "native = 1", "native masks need frames of one size");

    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", refusals);
    return 0;
}
