// Stand-alone program (its own main; never loaded into Python): repeats the refusals of vti_mask_polygons_frames and the zero
// answers of vti_mask_polygons_frames_scratch_bytes with fake device pointers that are never dereferenced, and expects the status
// and a message that begins with the function's name and names the argument.  The table walks read the host tables row by row:
// they are heap blocks of exactly the table's size, so a read past them is the sanitizer's to report.  Every call is refused, so
// none reaches a HIP call and the program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so
// by tests/test_polygons_frames_abi.py; prints "ok <number of refusals>" and returns 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vti.h"

static int failures = 0, refusals = 0;

// rc is VTI_ERR_ARG and the message of ctx begins with the function's name and holds needle (if any)
static void expect(int32_t rc, vti_ctx* ctx, const char* what, const char* needle) {
    const char* fn = "vti_mask_polygons_frames:";
    const char* msg = vti_last_error(ctx);
    const bool ok = rc == VTI_ERR_ARG && strncmp(msg, fn, strlen(fn)) == 0 && (!needle || strstr(msg, needle));
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s: rc %d, message \"%s\"\n", what, rc, msg); }
    ++refusals;
}

static void expect_zero(int64_t got, const char* what) {
    if (got != 0) { ++failures; fprintf(stderr, "FAIL scratch query, %s: %lld\n", what, (long long)got); }
    ++refusals;
}

struct Args {
    const uint8_t* masks; int32_t native; const int64_t* bases; int64_t capacity_bytes; const int32_t* offsets;
    const void* host_table; const void* dev_table; int32_t B, capacity, strategy; void* scratch; size_t scratch_bytes;
    int32_t* point_offsets; float* points; int64_t max_points;
};

int main() {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = 'n'; d.nc = 2; d.nm = 32; d.reg_max = 16; d.H = 736; d.W = 960; d.max_batch = 4; d.dtype = 0;
    vti_ctx* ctx = nullptr;
    if (vti_create(&d, &ctx) != VTI_OK || !ctx) { fprintf(stderr, "vti_create failed\n"); return 2; }
    vti_desc d64 = d;
    d64.H = 64; d64.W = 96;
    vti_ctx* other = nullptr;
    if (vti_create(&d64, &other) != VTI_OK || !other) { fprintf(stderr, "vti_create failed\n"); return 2; }

    // ---- the frame tables: exactly their bytes on the heap
    const int32_t B = 4, capacity = 20;
    const int32_t fh[4] = {960, 481, 720, 1080}, fw[4] = {1280, 333, 960, 1920};
    const int32_t bh[4] = {960, 481, 8200, 1080}, bw[4] = {1280, 333, 8200, 1920};      // frame 2: above 2^26 pixels
    auto pack = [&](vti_ctx* c, int32_t H, int32_t W, const int32_t* h, const int32_t* w, int32_t n, std::vector<uint8_t>& table) {
        std::vector<int64_t> at;
        int64_t total = 0;
        for (int32_t k = 0; k < n; ++k) { at.push_back(total); total = (total + 3LL * h[k] * w[k] + 15) & ~15LL; }
        table.resize((size_t)vti_frame_table_bytes(n));
        return vti_pack_frames(c, H, W, h, w, at.data(), n, total, table.data(), table.size());
    };
    std::vector<uint8_t> t_in, t_three, t_big, t_other;
    if (pack(ctx, d.H, d.W, fh, fw, 4, t_in) != VTI_OK || pack(ctx, d.H, d.W, fh, fw, 3, t_three) != VTI_OK ||
        pack(ctx, d.H, d.W, bh, bw, 4, t_big) != VTI_OK || pack(other, d64.H, d64.W, fh, fw, 4, t_other) != VTI_OK) {
        fprintf(stderr, "vti_pack_frames failed\n");
        return 2;
    }
    std::vector<uint8_t> t_bad = t_in, t_junk(t_in.size(), 0xA5);
    t_bad[64 + 2 * 64] = 1;                         // row 2's byte offset is no longer a multiple of 16

    // ---- the size query: the two good answers, then every zero
    const int64_t need0 = vti_mask_polygons_frames_scratch_bytes(ctx, t_in.data(), 0);
    const int64_t need1 = vti_mask_polygons_frames_scratch_bytes(ctx, t_in.data(), 1);
    if (need0 != vti_mask_polygons_scratch_bytes(ctx, d.H, d.W, d.W / 8) || need1 != vti_mask_polygons_scratch_bytes(ctx, 1080, 1920, 240)) {
        fprintf(stderr, "scratch queries gave %lld, %lld\n", (long long)need0, (long long)need1);
        return 2;
    }
    expect_zero(vti_mask_polygons_frames_scratch_bytes(nullptr, t_in.data(), 0), "null ctx");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, nullptr, 0), "null table");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, t_in.data(), 2), "native 2");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, t_junk.data(), 1), "junk");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, t_other.data(), 0), "another canvas");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, t_bad.data(), 1), "a bad row");
    expect_zero(vti_mask_polygons_frames_scratch_bytes(ctx, t_big.data(), 1), "a frame above 2^26 pixels");

    // ---- the call
    void* const one = (void*)(uintptr_t)4096;       // fake device pointers, never dereferenced
    void* const ws = (void*)(uintptr_t)(1 << 20);
    const Args good[2] = {
        {(const uint8_t*)one, 0, nullptr, 0, (const int32_t*)one, t_in.data(), one, B, capacity, VTI_POLY_LARGEST, ws, (size_t)need0,
         (int32_t*)one, (float*)one, 100},
        {(const uint8_t*)one, 1, (const int64_t*)one, 1 << 20, (const int32_t*)one, t_in.data(), one, B, capacity, VTI_POLY_CONCAT, ws,
         (size_t)need1, (int32_t*)one, (float*)one, 100}};
    auto call = [&](const Args& a) {
        return vti_mask_polygons_frames(ctx, a.masks, a.native, a.bases, a.capacity_bytes, a.offsets, a.host_table, a.dev_table, a.B,
                                        a.capacity, a.strategy, a.scratch, a.scratch_bytes, a.point_offsets, a.points, a.max_points, nullptr);
    };
    Args a;
#define ONE(k, change, needle) do { a = good[k]; change; expect(call(a), ctx, #change, needle); } while (0)
#define BOTH(change, needle) do { ONE(0, change, needle); ONE(1, change, needle); } while (0)
    BOTH(a.masks = nullptr, "null pointer");
    BOTH(a.offsets = nullptr, "null pointer");
    BOTH(a.point_offsets = nullptr, "null pointer");
    BOTH(a.points = nullptr, "null pointer");
    BOTH(a.native = 2, "native must be 0 or 1");
    BOTH(a.native = -1, "native must be 0 or 1");
    BOTH(a.capacity_bytes = -1, "capacity_bytes");
    BOTH(a.capacity = -1, "capacity and max_points");
    BOTH(a.max_points = -1, "capacity and max_points");
    BOTH(a.strategy = 2, "strategy");
    BOTH(a.B = 0, "another B");
    BOTH(a.B = 3, "another B");
    BOTH(a.B = 5, "another B");
    BOTH(a.host_table = nullptr, "null frame table");
    BOTH(a.dev_table = nullptr, "null frame table");
    BOTH(a.dev_table = (void*)(uintptr_t)(4096 + 8), "16-byte aligned");
    BOTH(a.host_table = t_three.data(), "another B");
    BOTH(a.host_table = t_bad.data(), "frame 2 of host_table");
    BOTH(a.host_table = t_junk.data(), "not a table of vti_pack_frames");
    BOTH(a.host_table = t_other.data(), "another canvas");
    BOTH(a.scratch = nullptr, "256-byte aligned");
    BOTH(a.scratch = (void*)(uintptr_t)((1 << 20) + 64), "256-byte aligned");
    BOTH(a.scratch_bytes -= 1, "scratch smaller than vti_mask_polygons_frames_scratch_bytes()");
    BOTH(a.offsets = (const int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    BOTH(a.point_offsets = (int32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    BOTH(a.points = (float*)(uintptr_t)(4096 + 2), "4-byte aligned");
    ONE(0, a.bases = (const int64_t*)one, "dev_mask_bases must be NULL with native = 0");
    ONE(1, a.bases = nullptr, "null dev_mask_bases");
    ONE(1, a.bases = (const int64_t*)(uintptr_t)(4096 + 4), "dev_mask_bases must be 8-byte aligned");
    ONE(0, a.masks = (const uint8_t*)(uintptr_t)(4096 + 8), "16-byte aligned");
    ONE(1, a.masks = (const uint8_t*)(uintptr_t)(4096 + 4), "8-byte aligned");
    ONE(1, (a.host_table = t_big.data(), a.scratch_bytes = (size_t)1 << 40), "frame 2 of host_table: H0 * W0 above 2^26");

    vti_destroy(other);
    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", refusals);
    return 0;
}
