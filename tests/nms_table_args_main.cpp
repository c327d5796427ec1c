// Stand-alone program (its own main; never loaded into Python): repeats the refusals of vti_pack_nms_table and vti_set_nms_table and
// the zero answers of vti_nms_table_bytes, and expects the status and a message that begins with the function's name and names the
// row and the field.  The tables, the parameter rows and the class lists are heap blocks of exactly their size, so a read or a write
// past them is the sanitizer's to report.  Both calls are host only and the device pointers are fake and never dereferenced, so the
// program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so by tests/test_nms_table_abi.py;
// prints "ok <number of checks>" and returns 0 when everything held.
#include <cmath>
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

static vti_ctx* make(int32_t nc, char scale = 'n') {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = scale; d.nc = nc; d.nm = 32; d.reg_max = 16; d.H = 64; d.W = 64; d.max_batch = 4; d.dtype = 0;
    vti_ctx* ctx = nullptr;
    if (vti_create(&d, &ctx) != VTI_OK || !ctx) { fprintf(stderr, "vti_create failed\n"); return nullptr; }
    return ctx;
}

int main() {
    vti_ctx* ctx = make(3);
    vti_ctx* other = make(2);
    vti_ctx* wide = make(VTI_NMS_TABLE_MAX_CLASSES + 1, 's');      // the s scale's class towers take any class count
    if (!ctx || !other || !wide) return 2;
    const char* PACK = "vti_pack_nms_table";
    const char* SET = "vti_set_nms_table";

    // ---- sizes
    expect_true(vti_nms_table_bytes(0) == 0 && vti_nms_table_bytes(-1) == 0 && vti_nms_table_bytes(VTI_NMS_TABLE_MAX_ROWS + 1) == 0, "zero sizes");
    const int64_t one = vti_nms_table_bytes(1), three = vti_nms_table_bytes(3);
    expect_true(one > 0 && three > one && (three - one) % 2 == 0 && vti_nms_table_bytes(VTI_NMS_TABLE_MAX_ROWS) > 0, "sizes grow by the row");

    // ---- a good table of three rows; the class lists are exact heap blocks
    std::vector<int32_t> only1 = {1}, dup = {2, 0, 2}, all = {0, 1, 2, 1};
    auto rows = [&]() {
        std::vector<vti_nms_params> p(3);
        p[0] = {0.20f, 200, 0.25, 0, 0, nullptr};
        p[1] = {0.50f, 20, 0.45, 1, (int32_t)only1.size(), only1.data()};
        p[2] = {0.25f, 300, 0.70, 0, (int32_t)dup.size(), dup.data()};
        return p;
    };
    std::vector<uint8_t> table((size_t)three, 0xAB), again((size_t)three, 0xCD);
    {
        std::vector<vti_nms_params> p = rows();
        expect_true(vti_pack_nms_table(ctx, p.data(), 3, table.data(), table.size()) == VTI_OK, "a good table packs");
        expect_true(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size()) == VTI_OK && table == again,
                    "equal inputs give equal bytes, whatever the buffer held");
        p[0].n_classes = (int32_t)all.size(); p[0].classes = all.data();      // every class named: no filter
        expect_true(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size()) == VTI_OK && table == again,
                    "a set that names every class equals no set");
    }

    // ---- pack refusals: each names the row and the field
    struct Bad { int row; const char* what; const char* needle; void (*edit)(vti_nms_params&); };
    const Bad bad[] = {
        {0, "conf -0.1", "row 0: conf", [](vti_nms_params& p) { p.conf = -0.1f; }},
        {1, "conf 1.5", "row 1: conf", [](vti_nms_params& p) { p.conf = 1.5f; }},
        {2, "conf NaN", "row 2: conf", [](vti_nms_params& p) { p.conf = NAN; }},
        {0, "iou -0.1", "row 0: iou", [](vti_nms_params& p) { p.iou = -0.1; }},
        {1, "iou 1.5", "row 1: iou", [](vti_nms_params& p) { p.iou = 1.5; }},
        {2, "iou NaN", "row 2: iou", [](vti_nms_params& p) { p.iou = (double)NAN; }},
        {1, "iou inf", "row 1: iou", [](vti_nms_params& p) { p.iou = (double)INFINITY; }},
        {1, "max_det 0", "row 1: max_det", [](vti_nms_params& p) { p.max_det = 0; }},
        {2, "agnostic 2", "row 2: agnostic", [](vti_nms_params& p) { p.agnostic = 2; }},
        {0, "n_classes -1", "row 0: n_classes", [](vti_nms_params& p) { p.n_classes = -1; }},
        {0, "a NULL list", "row 0: classes is NULL", [](vti_nms_params& p) { p.n_classes = 2; p.classes = nullptr; }},
    };
    for (const Bad& b : bad) {
        std::vector<vti_nms_params> p = rows();
        b.edit(p[b.row]);
        expect(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size()), VTI_ERR_ARG, ctx, PACK, b.what, b.needle);
    }
    {
        std::vector<vti_nms_params> p = rows();
        std::vector<int32_t> neg = {0, -1}, nc = {1, 3};
        p[1].n_classes = 2; p[1].classes = neg.data();
        expect(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size()), VTI_ERR_ARG, ctx, PACK, "class -1", "row 1: classes[1] = -1");
        p[1].classes = nc.data();
        expect(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size()), VTI_ERR_ARG, ctx, PACK, "class nc", "row 1: classes[1] = 3");
        p = rows();
        expect(vti_pack_nms_table(ctx, p.data(), 3, again.data(), again.size() - 1), VTI_ERR_ARG, ctx, PACK, "a short buffer", "smaller than");
        expect(vti_pack_nms_table(ctx, p.data(), 0, again.data(), again.size()), VTI_ERR_ARG, ctx, PACK, "no rows", "n_rows");
        expect(vti_pack_nms_table(ctx, nullptr, 3, again.data(), again.size()), VTI_ERR_ARG, ctx, PACK, "null params", "null");
        expect(vti_pack_nms_table(ctx, p.data(), 3, nullptr, again.size()), VTI_ERR_ARG, ctx, PACK, "null table", "null");
        expect_true(vti_pack_nms_table(nullptr, p.data(), 3, again.data(), again.size()) == VTI_ERR_ARG, "null ctx");
        // a class set on a model wider than the mask; the same rows without a set pack
        expect(vti_pack_nms_table(wide, p.data(), 3, again.data(), again.size()), VTI_ERR_UNSUPPORTED, wide, PACK, "nc above the mask", "row 1");
        p[1].n_classes = 0; p[2].n_classes = 0;
        expect_true(vti_pack_nms_table(wide, p.data(), 3, again.data(), again.size()) == VTI_OK, "no class set: any nc");
    }

    // ---- the setter: every refusal on the host, no device is touched
    const void* dev = (const void*)(uintptr_t)4096;
    const int32_t* idx = (const int32_t*)(uintptr_t)8192;
    expect(vti_set_nms_table(ctx, table.data(), (const void*)(uintptr_t)(4096 + 8), 3, idx), VTI_ERR_ARG, ctx, SET, "misaligned dev_table", "16-byte");
    expect(vti_set_nms_table(ctx, table.data(), nullptr, 3, idx), VTI_ERR_ARG, ctx, SET, "null dev_table", "dev_table");
    expect(vti_set_nms_table(ctx, table.data(), dev, 3, (const int32_t*)(uintptr_t)(8192 + 2)), VTI_ERR_ARG, ctx, SET, "misaligned index", "4-byte");
    expect(vti_set_nms_table(ctx, table.data(), dev, 2, idx), VTI_ERR_ARG, ctx, SET, "n_rows not the table's", "n_rows");
    expect(vti_set_nms_table(ctx, table.data(), dev, 0, idx), VTI_ERR_ARG, ctx, SET, "n_rows 0", "n_rows");
    expect(vti_set_nms_table(other, table.data(), dev, 3, idx), VTI_ERR_ARG, other, SET, "a table packed for another nc", "class count");
    {
        std::vector<uint8_t> hurt = table;
        hurt[0] ^= 0xFF;
        expect(vti_set_nms_table(ctx, hurt.data(), dev, 3, idx), VTI_ERR_ARG, ctx, SET, "a damaged header", "not a table");
        hurt = table;
        const float nan = NAN;
        memcpy(hurt.data() + (size_t)one, &nan, 4);      // row 1 begins where a table of one row ends; its first field is conf
        expect(vti_set_nms_table(ctx, hurt.data(), dev, 3, idx), VTI_ERR_ARG, ctx, SET, "a damaged row", "row 1: conf");
    }
    expect_true(vti_set_nms_table(nullptr, table.data(), dev, 3, idx) == VTI_ERR_ARG, "null ctx");
    expect_true(vti_set_nms_table(ctx, table.data(), dev, 3, idx) == VTI_OK, "a good table is set");
    expect_true(vti_set_nms_table(ctx, table.data(), dev, 3, nullptr) == VTI_OK, "a NULL index: row 0 for every frame");
    // with a table set, an NMS call with fake pointers still stops at today's checks (the workspace is not set)
    expect(vti_nms(ctx, (const float*)dev, 1, 0.25f, 0.7, 10, 0, (float*)dev, (int32_t*)dev, nullptr), VTI_ERR_STATE, ctx, "vti_nms",
           "nms before setup", "workspace");
    expect(vti_nms(ctx, (const float*)dev, 9, 0.25f, 0.7, 10, 0, (float*)dev, (int32_t*)dev, nullptr), VTI_ERR_ARG, ctx, "vti_nms",
           "nms with B above max_batch", "B out of range");
    expect_true(vti_set_nms_table(ctx, nullptr, nullptr, 0, nullptr) == VTI_OK, "clearing");
    expect_true(vti_set_nms_table(ctx, nullptr, dev, 7, idx) == VTI_OK, "clearing ignores the other arguments");

    vti_destroy(wide);
    vti_destroy(other);
    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
