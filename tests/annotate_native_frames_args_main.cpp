// Stand-alone program (its own main; never loaded into Python): repeats the refusals of vti_annotate_frames_native and
// vti_annotate_checker_frames_native with fake device pointers that are never dereferenced, and expects the status and a message that
// begins with the function's name and names the argument.  The table and selection walks read the host tables and the selection row
// by row: all are heap blocks of exactly their size, so a read past them is the sanitizer's to report.  Every call is refused, so none
// reaches a HIP call and the program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so by
// tests/test_annotate_native_frames_abi.py; prints "ok <number of refusals>" and returns 0 when everything held.
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

struct Picture {            // the arguments of the two calls
    vti_ctx* ctx; const uint8_t* frames; const void* host_table; const void* dev_table; int32_t B;
    const void* cameras; int32_t n_cams; const int32_t* index; const uint8_t* masks; const int64_t* bases; int64_t capacity_bytes;
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

    // ---- the frame tables: exactly their bytes on the heap
    const int32_t B = 4, max_det = 200, capacity = 800, n_sel = 3, max_points = 4096, n_cams = 2;
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
    const int32_t wh[4] = {960, 8200, 720, 1080}, ww[4] = {1280, 480, 960, 1920};      // frame 1 above the raster's limit
    const int32_t woh[3] = {1080, 8200, 1080}, wow[3] = {1920, 480, 1920};
    std::vector<uint8_t> t_in, t_out, t_three, t_wide, t_wide_out;
    if (pack(fh, fw, 4, t_in) != VTI_OK || pack(oh.data(), ow.data(), n_sel, t_out) != VTI_OK || pack(fh, fw, 3, t_three) != VTI_OK ||
        pack(wh, ww, 4, t_wide) != VTI_OK || pack(woh, wow, 3, t_wide_out) != VTI_OK) {
        fprintf(stderr, "vti_pack_frames failed\n");
        return 2;
    }
    std::vector<uint8_t> t_bad = t_in;
    t_bad[64 + 2 * 64] = 1;                         // row 2's byte offset is no longer a multiple of 16

    void* const one = (void*)(uintptr_t)4096;       // fake device pointers, never dereferenced
    void* const ws = (void*)(uintptr_t)(1 << 20);
    const float* const f = (const float*)one;
    const int32_t* const i = (const int32_t*)one;

    const int64_t need = vti_annotate_frames_scratch_bytes(ctx, t_out.data(), max_det, max_points);
    if (need <= 0) { fprintf(stderr, "the scratch query gave %lld\n", (long long)need); return 2; }
    const Picture good = {ctx, (const uint8_t*)one, t_in.data(), one, B, one, n_cams, i, (const uint8_t*)one, (const int64_t*)one, 1 << 20,
                          f, max_det, capacity, (const double*)one, sel.data(), i, n_sel, max_points, t_out.data(), one, (uint8_t*)one,
                          ws, (size_t)need};
    auto draw = [&](const Picture& q) {
        return vti_annotate_frames_native(q.ctx, q.frames, q.host_table, q.dev_table, q.B, q.cameras, q.n_cams, q.index, q.masks, q.bases,
                                          q.capacity_bytes, q.dets, f, i, i, q.max_det, q.capacity, i, q.stitch_f64, i, q.host_select,
                                          q.dev_select, q.n_sel, q.max_points, q.host_out_table, q.dev_out_table, q.out, (int32_t*)one,
                                          q.scratch, q.scratch_bytes, nullptr);
    };
    auto draw_checker = [&](const Picture& q) {
        return vti_annotate_checker_frames_native(q.ctx, q.frames, q.host_table, q.dev_table, q.B, q.cameras, q.n_cams, q.index, q.masks,
                                                  q.bases, q.capacity_bytes, q.dets, f, i, i, q.max_det, q.capacity, i, q.stitch_f64, i,
                                                  q.host_select, q.dev_select, q.n_sel, q.max_points, q.host_out_table, q.dev_out_table,
                                                  q.out, (int32_t*)one, q.scratch, q.scratch_bytes, nullptr);
    };
    Picture q;
#define PICTURE(call, fn, change, needle) do { q = good; change; expect(call(q), VTI_ERR_ARG, ctx, fn, #change, needle); } while (0)
#define BOTH(change, needle) do { PICTURE(draw, "vti_annotate_frames_native:", change, needle); \
                                   PICTURE(draw_checker, "vti_annotate_checker_frames_native:", change, needle); } while (0)
#define BOTH_OUT(change, needle) do { PICTURE(draw, "vti_annotate_frames_native (out table):", change, needle); \
                                       PICTURE(draw_checker, "vti_annotate_checker_frames_native (out table):", change, needle); } while (0)
    std::vector<int32_t> low = {3, -1, 3}, high = {3, 0, B}, other = {3, 1, 3};
    // a null ctx: the message goes to the library's own slot
    q = good; q.ctx = nullptr;
    expect(draw(q), VTI_ERR_ARG, nullptr, "vti_annotate_frames_native:", "null ctx", "null ctx");
    expect(draw_checker(q), VTI_ERR_ARG, nullptr, "vti_annotate_checker_frames_native:", "null ctx", "null ctx");
    // the ragged rows
    BOTH(q.bases = nullptr, "null dev_mask_bases");
    BOTH(q.bases = (const int64_t*)(uintptr_t)(4096 + 4), "dev_mask_bases must be 8-byte aligned");
    BOTH(q.capacity_bytes = -1, "capacity_bytes must be >= 0");
    BOTH(q.masks = nullptr, "null pointer");                                            // capacity_bytes > 0 needs the masks
    BOTH((q.masks = nullptr, q.capacity = 0), "null pointer");                          // ... whatever `capacity` says
    BOTH(q.masks = (const uint8_t*)(uintptr_t)(4096 + 4), "native masks must be 8-byte aligned");
    // vti_annotate_frames' refusals through the new names
    BOTH(q.frames = nullptr, "null pointer");
    BOTH(q.cameras = nullptr, "null pointer");
    BOTH(q.dets = nullptr, "null pointer");
    BOTH(q.stitch_f64 = nullptr, "null pointer");
    BOTH(q.host_select = nullptr, "null pointer");
    BOTH(q.dev_select = nullptr, "null pointer");
    BOTH(q.out = nullptr, "null pointer");
    BOTH(q.n_cams = 0, "bad size");
    BOTH(q.max_det = VTI_MEASURE_MAX_DET + 1, "bad size");
    BOTH(q.max_det = 0, "bad size");
    BOTH(q.capacity = -1, "bad size");
    BOTH(q.max_points = -1, "bad size");
    BOTH(q.host_select = low.data(), "host_select[1] = -1");
    BOTH(q.host_select = high.data(), "host_select[2] = 4");
    BOTH(q.host_select = other.data(), "row 1 of the out table");
    BOTH((q.host_table = t_wide.data(), q.host_out_table = t_wide_out.data(), q.host_select = other.data(), q.scratch_bytes = (size_t)1 << 40),
         "8192");
    BOTH(q.cameras = (void*)(uintptr_t)(4096 + 8), "16-byte aligned");
    BOTH(q.index = (const int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    BOTH(q.dev_select = (const int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    BOTH(q.stitch_f64 = (const double*)(uintptr_t)(4096 + 4), "misaligned");
    BOTH(q.frames = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte aligned");
    BOTH(q.out = (uint8_t*)(uintptr_t)(4096 + 8), "16-byte aligned");
    BOTH(q.scratch = nullptr, "256-byte aligned");
    BOTH(q.scratch = (void*)(uintptr_t)((1 << 20) + 64), "256-byte aligned");
    BOTH(q.scratch_bytes = (size_t)need - 1, "scratch smaller than vti_annotate_frames_scratch_bytes()");
    BOTH(q.host_table = nullptr, nullptr);
    BOTH(q.dev_table = nullptr, nullptr);
    BOTH(q.dev_table = (void*)(uintptr_t)(4096 + 8), nullptr);
    BOTH(q.host_table = t_three.data(), "another B");
    BOTH(q.B = 3, "another B");
    BOTH(q.host_table = t_bad.data(), "frame 2 of host_table");
    BOTH(q.n_sel = 0, "n_sel");
    BOTH_OUT(q.host_out_table = nullptr, nullptr);
    BOTH_OUT(q.dev_out_table = nullptr, nullptr);
    BOTH_OUT(q.host_out_table = t_in.data(), "another B");

    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", refusals);
    return 0;
}
