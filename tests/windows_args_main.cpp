// Stand-alone program (its own main; never loaded into Python): repeats the refusals of vti_pack_windows and of the *_windows calls,
// the answers of the two size queries and vti_window_table_info, and expects the status and a message that begins with the
// function's name and names the frame.  The tables and the argument arrays are heap blocks of exactly their size, so a read or a
// write past them is the sanitizer's to report.  Every refusal comes before the first HIP call and the device pointers are fake and
// never dereferenced, so the program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so by
// tests/test_windows_abi.py; prints "ok <number of checks>" and returns 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vti.h"

static int failures = 0, checks = 0;

static void expect(int32_t rc, int32_t want, vti_ctx* ctx, const char* fn, const char* what, const char* needle) {
    const char* msg = vti_last_error(ctx);
    const bool ok = rc == want && strncmp(msg, fn, strlen(fn)) == 0 && msg[strlen(fn)] == ':' && (!needle || strstr(msg, needle));
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s: rc %d, message \"%s\"\n", what, rc, msg); }
    ++checks;
}

static void expect_true(bool ok, const char* what) {
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s\n", what); }
    ++checks;
}

static vti_ctx* make(int32_t H, int32_t W, int32_t max_batch) {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = 'n'; d.nc = 2; d.nm = 32; d.reg_max = 16; d.H = H; d.W = W; d.max_batch = max_batch; d.dtype = 0;
    vti_ctx* ctx = nullptr;
    if (vti_create(&d, &ctx) != VTI_OK || !ctx) { fprintf(stderr, "vti_create failed\n"); return nullptr; }
    return ctx;
}

int main() {
    vti_ctx* ctx = make(64, 96, 4);
    vti_ctx* other = make(64, 64, 4);
    vti_ctx* small = make(64, 96, 2);
    if (!ctx || !other || !small) return 2;
    const char* PACK = "vti_pack_windows";
    const int32_t H = 64, W = 96, B = 3;

    // ---- sizes
    expect_true(vti_window_table_bytes(0) == 0 && vti_window_table_bytes(-1) == 0, "zero sizes");
    const int64_t one = vti_window_table_bytes(1), three = vti_window_table_bytes(3);
    expect_true(one > 0 && three == one + 2 * (vti_window_table_bytes(2) - one), "sizes grow by the row");

    // ---- three frames back to back at multiples of 16; exact heap blocks
    const std::vector<int32_t> H0 = {140, 135, 480}, W0 = {200, 241, 640};
    std::vector<int64_t> off(3);
    int64_t total = 0;
    for (int b = 0; b < 3; ++b) { off[b] = total; total = (total + 3LL * H0[b] * W0[b] + 15) & ~15LL; }
    const std::vector<int32_t> good = {3, 5, 131, 97, 0, 0, 241, 135, 639, 479, 1, 1};
    std::vector<uint8_t> table((size_t)three, 0xAB), again((size_t)three, 0xCD);
    auto pack = [&](const std::vector<int32_t>& win, std::vector<uint8_t>& t, size_t nbytes) {
        return vti_pack_windows(ctx, H, W, H0.data(), W0.data(), off.data(), win.data(), B, total, t.data(), nbytes);
    };
    expect_true(pack(good, table, table.size()) == VTI_OK, "a good table packs");
    expect_true(pack(good, again, again.size()) == VTI_OK && table == again, "equal inputs give equal bytes, whatever the buffer held");
    expect_true(vti_pack_windows(nullptr, H, W, H0.data(), W0.data(), off.data(), good.data(), B, total, again.data(), again.size()) == VTI_OK &&
                table == again, "ctx is optional");

    // ---- the packer's refusals name the first failing frame
    struct Bad { int frame, field, value; const char* needle; };
    const Bad bads[] = {
        {0, 0, 70, "inside its frame"},      // x0 + w > W0
        {1, 1, 1, "inside its frame"},       // y0 + h > H0
        {2, 0, -1, "inside its frame"},      // x0 < 0
        {1, 1, -2, "inside its frame"},      // y0 < 0
        {0, 2, 0, ">= 1"},                   // w < 1
        {2, 3, 0, ">= 1"},                   // h < 1
        {1, 2, -5, ">= 1"},
        {2, 2, 2, "inside its frame"},       // x0 = 639, w = 2
    };
    for (const Bad& c : bads) {
        std::vector<int32_t> w = good;
        w[4 * c.frame + c.field] = c.value;
        char what[64], frame[32];
        snprintf(what, sizeof what, "window frame %d field %d = %d", c.frame, c.field, c.value);
        snprintf(frame, sizeof frame, "frame %d:", c.frame);
        const int32_t rc = pack(w, again, again.size());
        expect(rc, VTI_ERR_ARG, ctx, PACK, what, c.needle);
        expect_true(strstr(vti_last_error(ctx), frame) != nullptr, what);
    }
    {   // the FIRST failing frame is the one named
        std::vector<int32_t> w = good;
        w[4 * 1 + 2] = 0; w[4 * 2 + 3] = 0;
        expect(pack(w, again, again.size()), VTI_ERR_ARG, ctx, PACK, "first failing frame", "frame 1:");
    }
    {   // a window that the letterbox would resize below 1 px: 1 x 640 on a 64 x 96 canvas -> height 1 * 96 / 640 rounds to 0
        std::vector<int32_t> w = good;
        w[8] = 0; w[9] = 0; w[10] = 640; w[11] = 1;
        expect(pack(w, again, again.size()), VTI_ERR_ARG, ctx, PACK, "resized below 1 px", "below 1 px");
        expect_true(strstr(vti_last_error(ctx), "frame 2:") != nullptr, "resized below 1 px names its frame");
    }
    expect(pack(good, again, again.size() - 1), VTI_ERR_ARG, ctx, PACK, "short buffer", "smaller than");
    expect(vti_pack_windows(ctx, H, W, nullptr, W0.data(), off.data(), good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "null H0", "null");
    expect(vti_pack_windows(ctx, H, W, H0.data(), nullptr, off.data(), good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "null W0", "null");
    expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), nullptr, good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "null offsets", "null");
    expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), off.data(), nullptr, B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "null windows", "null");
    expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), off.data(), good.data(), B, total, nullptr, again.size()), VTI_ERR_ARG, ctx,
           PACK, "null table", "null");
    expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), off.data(), good.data(), 0, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "B < 1", "B < 1");
    expect(vti_pack_windows(small, H, W, H0.data(), W0.data(), off.data(), good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, small,
           PACK, "B above max_batch", "max_batch");
    expect(vti_pack_windows(ctx, 60, W, H0.data(), W0.data(), off.data(), good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
           PACK, "canvas", "multiples of 32");
    expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), off.data(), good.data(), B, total - 16, again.data(), again.size()), VTI_ERR_ARG,
           ctx, PACK, "frame past total_bytes", "frame 2: the frame runs past");
    {
        std::vector<int64_t> o = off;
        o[1] += 8;
        expect(vti_pack_windows(ctx, H, W, H0.data(), W0.data(), o.data(), good.data(), B, total, again.data(), again.size()), VTI_ERR_ARG, ctx,
               PACK, "offset alignment", "frame 1: byte_offset");
    }

    // ---- info: a whole-frame row is the frame table's row
    {
        std::vector<uint8_t> ft((size_t)vti_frame_table_bytes(B));
        expect_true(vti_pack_frames(ctx, H, W, H0.data(), W0.data(), off.data(), B, total, ft.data(), ft.size()) == VTI_OK, "frame table");
        int32_t wi[12], fi[8];
        double wd[5], fd[5];
        expect_true(vti_window_table_info(table.data(), 1, wi, wd) == VTI_OK && vti_frame_table_info(ft.data(), 1, fi, fd) == VTI_OK &&
                    memcmp(wi, fi, sizeof fi) == 0 && memcmp(wd, fd, sizeof fd) == 0 && wi[8] == 0 && wi[9] == 0 && wi[10] == 135 && wi[11] == 241,
                    "whole-frame window == frame row");
        expect_true(vti_window_table_info(table.data(), 0, wi, nullptr) == VTI_OK && wi[0] == 97 && wi[1] == 131 && wi[8] == 3 && wi[9] == 5 &&
                    (((int64_t)wi[7] << 32) | (uint32_t)wi[6]) == off[0] + 3 * (5 * 200 + 3), "row 0");
        expect_true(vti_window_table_info(table.data(), -1, wi, nullptr) == VTI_OK && wi[0] == B && wi[1] == H && wi[2] == W && wi[3] == 480 &&
                    wi[4] == 640, "header");
        expect_true(vti_window_table_info(table.data(), 3, wi, nullptr) == VTI_ERR_ARG && vti_window_table_info(nullptr, 0, wi, nullptr) == VTI_ERR_ARG &&
                    vti_window_table_info(table.data(), 0, nullptr, nullptr) == VTI_ERR_ARG && vti_window_table_info(ft.data(), 0, wi, nullptr) == VTI_ERR_ARG,
                    "info refusals");
        // the bytes query equals the frames query
        for (int32_t md : {1, 7, 300})
            expect_true(vti_mask_native_windows_bytes(ctx, table.data(), md) == vti_mask_native_frames_bytes(ctx, ft.data(), md) &&
                        vti_mask_native_windows_bytes(ctx, table.data(), md) > 0, "bytes query");
        expect_true(vti_mask_native_windows_bytes(ctx, table.data(), 0) == 0 && vti_mask_native_windows_bytes(nullptr, table.data(), 5) == 0 &&
                    vti_mask_native_windows_bytes(ctx, nullptr, 5) == 0 && vti_mask_native_windows_bytes(ctx, ft.data(), 5) == 0 &&
                    vti_mask_native_windows_bytes(other, table.data(), 5) == 0 && vti_mask_native_windows_bytes(small, table.data(), 5) == 0,
                    "bytes query refusals");
    }

    // ---- the device calls refuse on the host; fake device pointers
    void* dev = (void*)(uintptr_t)4096;
    uint8_t* d8 = (uint8_t*)dev;
    float* df = (float*)dev;
    int32_t* di = (int32_t*)dev;
    int64_t* dl = (int64_t*)dev;
    const char* LB = "vti_letterbox_windows";
    const char* SB = "vti_scale_boxes_windows";
    const char* MN = "vti_masks_native_windows";
    const char* PW = "vti_predict_windows";
    std::vector<uint8_t> bent = table;                       // frame 1's window moved out of its frame
    {
        const int64_t hdr = one - (vti_window_table_bytes(2) - one), row = vti_window_table_bytes(2) - one;
        int32_t x0 = 500;
        memcpy(bent.data() + hdr + row + 64 + 8 + 8, &x0, 4);
    }
    std::vector<uint8_t> junk(table.size(), 0);
    auto table_checks = [&](const char* fn, auto call) {
        expect(call(ctx, (const void*)table.data(), (const void*)nullptr, B), VTI_ERR_ARG, ctx, fn, "null device table", "null window table");
        expect(call(ctx, (const void*)nullptr, (const void*)dev, B), VTI_ERR_ARG, ctx, fn, "null host table", "null window table");
        expect(call(ctx, (const void*)table.data(), (const void*)((char*)dev + 8), B), VTI_ERR_ARG, ctx, fn, "alignment", "16-byte aligned");
        expect(call(ctx, (const void*)junk.data(), (const void*)dev, B), VTI_ERR_ARG, ctx, fn, "not a table", "vti_pack_windows");
        expect(call(ctx, (const void*)table.data(), (const void*)dev, 2), VTI_ERR_ARG, ctx, fn, "another B", "another B");
        expect(call(ctx, (const void*)table.data(), (const void*)dev, 0), VTI_ERR_ARG, ctx, fn, "B = 0", "another B");
        expect(call(other, (const void*)table.data(), (const void*)dev, B), VTI_ERR_ARG, other, fn, "another canvas", "another canvas");
        expect(call(ctx, (const void*)bent.data(), (const void*)dev, B), VTI_ERR_ARG, ctx, fn, "bent row", "frame 1 of host_table");
        expect_true(call((vti_ctx*)nullptr, (const void*)table.data(), (const void*)dev, B) == VTI_ERR_ARG, "null ctx");
    };
    table_checks(LB, [&](vti_ctx* c, const void* h, const void* d, int32_t b) { return vti_letterbox_windows(c, d8, h, d, b, d8, nullptr); });
    expect(vti_letterbox_windows(ctx, nullptr, table.data(), dev, B, d8, nullptr), VTI_ERR_ARG, ctx, LB, "null frames", "null");
    expect(vti_letterbox_windows(ctx, d8, table.data(), dev, B, nullptr, nullptr), VTI_ERR_ARG, ctx, LB, "null out", "null");
    expect(vti_letterbox_windows(ctx, d8 + 8, table.data(), dev, B, d8, nullptr), VTI_ERR_ARG, ctx, LB, "frames alignment", "16-byte");
    expect(vti_letterbox_windows(ctx, d8, table.data(), dev, B, d8 + 2, nullptr), VTI_ERR_ARG, ctx, LB, "out alignment", "4-byte");
    expect(vti_letterbox_windows(small, d8, table.data(), dev, B, d8, nullptr), VTI_ERR_ARG, small, LB, "B above max_batch", "max_batch");

    table_checks(SB, [&](vti_ctx* c, const void* h, const void* d, int32_t b) { return vti_scale_boxes_windows(c, df, di, h, d, b, 10, df, nullptr); });
    expect(vti_scale_boxes_windows(ctx, nullptr, di, table.data(), dev, B, 10, df, nullptr), VTI_ERR_ARG, ctx, SB, "null dets", "bad argument");
    expect(vti_scale_boxes_windows(ctx, df, nullptr, table.data(), dev, B, 10, df, nullptr), VTI_ERR_ARG, ctx, SB, "null counts", "bad argument");
    expect(vti_scale_boxes_windows(ctx, df, di, table.data(), dev, B, 10, nullptr, nullptr), VTI_ERR_ARG, ctx, SB, "null xyxy", "bad argument");
    expect(vti_scale_boxes_windows(ctx, df, di, table.data(), dev, B, 0, df, nullptr), VTI_ERR_ARG, ctx, SB, "max_det", "bad argument");
    expect(vti_scale_boxes_windows(ctx, df, di, table.data(), dev, B, 10, df + 1, nullptr), VTI_ERR_ARG, ctx, SB, "xyxy alignment", "bad argument");

    auto mn = [&](vti_ctx* c, const void* h, const void* d, int32_t b) {
        return vti_masks_native_windows(c, df, di, dev, h, d, b, 10, VTI_MASK_LOGIT, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr);
    };
    table_checks(MN, mn);
    expect(vti_masks_native_windows(ctx, nullptr, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "null dets", "bad argument");
    expect(vti_masks_native_windows(ctx, df, nullptr, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "null counts", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, nullptr, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "null proto", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, nullptr, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "null masks", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, nullptr, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "null offsets", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, di, nullptr, nullptr), VTI_ERR_ARG,
           ctx, MN, "null bases", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 0, 0, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG, ctx,
           MN, "max_det", "bad argument");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, -1, di, dl, nullptr), VTI_ERR_ARG, ctx, MN,
           "capacity_bytes", "capacity_bytes");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 5, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG, ctx,
           MN, "mode", "bad mode");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_U8, d8, 1 << 16, di, dl, nullptr),
           VTI_ERR_UNSUPPORTED, ctx, MN, "u8 packing", "VTI_PACK_BITS");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, 7, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG, ctx, MN,
           "packing", "bad packing");
    expect(vti_masks_native_windows(ctx, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8 + 4, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           ctx, MN, "masks alignment", "8-byte aligned");
    expect(vti_masks_native_windows(small, df, di, dev, table.data(), dev, B, 10, 0, VTI_PACK_BITS, d8, 1 << 16, di, dl, nullptr), VTI_ERR_ARG,
           small, MN, "B above max_batch", "B out of range");
    expect(mn(ctx, table.data(), dev, B), VTI_ERR_STATE, ctx, MN, "every argument accepted", "workspace not set");

    auto pw = [&](vti_ctx* c, const void* h, const void* d, int32_t b) {
        return vti_predict_windows(c, d8, h, d, b, 0, 0.25f, 0.7, 10, 0, VTI_MASK_LOGIT, VTI_PACK_BITS, d8, df, dev, df, di, d8, 1 << 16, di, dl,
                                   df, nullptr);
    };
    table_checks(PW, pw);
    expect(vti_predict_windows(ctx, nullptr, table.data(), dev, B, 0, 0.25f, 0.7, 10, 0, 0, VTI_PACK_BITS, d8, df, dev, df, di, d8, 1 << 16, di,
                               dl, df, nullptr), VTI_ERR_ARG, ctx, PW, "null frames", "dev_frames");
    expect(vti_predict_windows(ctx, d8, table.data(), dev, B, 0, 0.25f, 0.7, 10, 0, 0, VTI_PACK_BITS, nullptr, df, dev, df, di, d8, 1 << 16, di,
                               dl, df, nullptr), VTI_ERR_ARG, ctx, PW, "null scratch", "dev_input_scratch");
    expect(vti_predict_windows(ctx, d8, table.data(), dev, B, 0, 0.25f, 0.7, 10, 0, 0, VTI_PACK_BITS, d8, nullptr, dev, df, di, d8, 1 << 16, di,
                               dl, df, nullptr), VTI_ERR_ARG, ctx, PW, "null pred", "dev_pred");
    expect(vti_predict_windows(ctx, d8, table.data(), dev, B, 0, 0.25f, 0.7, 10, 0, 0, VTI_PACK_BITS, d8, df, dev, df, di, d8, 1 << 16, di, dl,
                               nullptr, nullptr), VTI_ERR_ARG, ctx, PW, "null xyxy", "dev_xyxy is required");
    expect(vti_predict_windows(ctx, d8, table.data(), dev, B, 0, 0.25f, 0.7, 10, 0, 0, VTI_PACK_U8, d8, df, dev, df, di, d8, 1 << 16, di, dl, df,
                               nullptr), VTI_ERR_UNSUPPORTED, ctx, PW, "u8 packing", "VTI_PACK_BITS");
    expect(vti_predict_windows(ctx, d8, table.data(), dev, B, 0, 0.25f, 0.7, 0, 0, 0, VTI_PACK_BITS, d8, df, dev, df, di, d8, 1 << 16, di, dl, df,
                               nullptr), VTI_ERR_ARG, ctx, PW, "max_det", "bad argument");
    expect(pw(ctx, table.data(), dev, B), VTI_ERR_STATE, ctx, PW, "every argument accepted", "weights not loaded");

    vti_destroy(ctx);
    vti_destroy(other);
    vti_destroy(small);
    if (failures) { fprintf(stderr, "%d of %d checks failed\n", failures, checks); return 1; }
    printf("ok %d\n", checks);
    return 0;
}
