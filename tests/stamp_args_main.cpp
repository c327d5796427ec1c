// Stand-alone program (its own main; never loaded into Python): drives the host-only half of the stamp calls -- vti_stamp_table_bytes
// and vti_pack_stamps on valid and invalid input, the tables in heap blocks of exactly their size -- and every argument check of
// vti_stamp and vti_stamp_frames with fake device pointers that are never dereferenced.  Every launching call is refused, so none
// reaches a HIP call and the program may run anywhere.  Built with -fsanitize=address,undefined and linked against libvti.so by
// tests/test_stamp_abi.py; prints "ok <number of checks>" and returns 0 when everything held.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vti.h"

static int failures = 0, checks = 0;

// rc is VTI_ERR_ARG and the message of ctx begins with "<fn>:" and holds needle
static void refused(int32_t rc, vti_ctx* ctx, const char* fn, const char* what, const char* needle) {
    const char* msg = ctx ? vti_last_error(ctx) : "";
    const size_t n = strlen(fn);
    const bool ok = rc == VTI_ERR_ARG && (!ctx || (strncmp(msg, fn, n) == 0 && msg[n] == ':' && (!needle || strstr(msg, needle))));
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s: rc %d, message \"%s\"\n", what, rc, msg); }
    ++checks;
}
static void expect(bool ok, const char* what) {
    if (!ok) { ++failures; fprintf(stderr, "FAIL %s\n", what); }
    ++checks;
}

static vti_stamp_desc desc(int32_t picture, int32_t x, int32_t y, int32_t w, int32_t h, int32_t pitch, int64_t at) {
    vti_stamp_desc d;
    memset(&d, 0, sizeof d);
    d.picture = picture; d.x = x; d.y = y; d.w = w; d.h = h; d.pitch = pitch; d.word_offset = at;
    d.bgr[0] = 10; d.bgr[1] = 20; d.bgr[2] = 30;
    return d;
}

int main() {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = 'n'; d.nc = 2; d.nm = 32; d.reg_max = 16; d.H = 64; d.W = 96; d.max_batch = 4; d.dtype = 0;
    vti_ctx* ctx = nullptr;
    if (vti_create(&d, &ctx) != VTI_OK || !ctx) { fprintf(stderr, "vti_create failed\n"); return 2; }

    // ---- the size of a table ------------------------------------------------------------------------------------------------------
    expect(vti_stamp_table_bytes(3, 4) == 64 + 3 * 16 + 4 * 32, "table bytes (3, 4)");
    expect(vti_stamp_table_bytes(1, 0) == 80, "table bytes (1, 0)");
    expect(vti_stamp_table_bytes(0, 1) == 0 && vti_stamp_table_bytes(VTI_STAMP_MAX_PICTURES + 1, 1) == 0, "table bytes: pictures");
    expect(vti_stamp_table_bytes(1, -1) == 0 && vti_stamp_table_bytes(1, VTI_STAMP_MAX_TOTAL + 1) == 0, "table bytes: stamps");

    // ---- the packer: three pictures, the second without a stamp -------------------------------------------------------------------
    const std::vector<int32_t> H0 = {37, 64, 8}, W0 = {53, 96, 8};
    const std::vector<vti_stamp_desc> good = {desc(0, 1, 2, 33, 4, 2, 0), desc(0, 0, 0, 5, 5, 1, 8), desc(2, 2, 2, 6, 6, 3, 13)};
    const int64_t n_words = 13 + 18;
    auto pack = [&](const std::vector<vti_stamp_desc>& s, std::vector<uint8_t>& table, int64_t words, size_t shorter = 0) {
        std::vector<vti_stamp_desc> exact(s);               // exactly n_stamps entries on the heap
        table.assign((size_t)vti_stamp_table_bytes(3, (int32_t)s.size()), 0xCD);
        return vti_pack_stamps(ctx, H0.data(), W0.data(), 3, exact.empty() ? nullptr : exact.data(), (int32_t)exact.size(), words,
                               table.data(), table.size() - shorter);
    };
    std::vector<uint8_t> table, scratch;
    expect(pack(good, table, n_words) == VTI_OK, "a valid table packs");
    std::vector<uint8_t> twice;
    expect(pack(good, twice, n_words) == VTI_OK && twice == table, "equal inputs give equal bytes");
    expect(pack({}, scratch, 0) == VTI_OK, "a table without stamps packs");
    expect(vti_pack_stamps(nullptr, H0.data(), W0.data(), 3, good.data(), 3, n_words, twice.data(), twice.size()) == VTI_OK, "ctx may be NULL");
    std::vector<vti_stamp_desc> s;
#define BAD(change, needle) do { s = good; change; refused(pack(s, scratch, n_words), ctx, "vti_pack_stamps", #change, needle); } while (0)
    BAD(s[1].picture = 3, "stamp 1: picture outside");
    BAD(s[0].picture = -1, "stamp 0: picture outside");
    BAD((s[0].picture = 2, s[0].w = 3), "stamp 1: picture must not decrease");
    BAD(s[2].w = 0, "stamp 2: w and h");
    BAD(s[0].h = 0, "stamp 0: w and h");
    BAD(s[0].x = 21, "stamp 0: the rectangle is not inside");
    BAD(s[0].y = 34, "stamp 0: the rectangle is not inside");
    BAD(s[2].x = -1, "stamp 2: the rectangle is not inside");
    BAD(s[2].h = 7, "stamp 2: the rectangle is not inside");
    BAD(s[0].x = INT32_MAX, "stamp 0: the rectangle is not inside");
    BAD(s[0].w = INT32_MAX, "stamp 0: the rectangle is not inside");
    BAD(s[0].pitch = 1, "stamp 0: pitch must be >=");
    BAD(s[1].pitch = 0, "stamp 1: pitch must be >=");
    BAD(s[1].pitch = VTI_STAMP_MAX_PITCH + 1, "stamp 1: pitch must be <=");
    BAD(s[2].word_offset = 14, "stamp 2: its rows run past n_words");
    BAD(s[1].word_offset = -1, "stamp 1: its rows run past n_words");
    BAD(s[1].word_offset = INT64_MAX, "stamp 1: its rows run past n_words");
    refused(pack(good, scratch, n_words, 1), ctx, "vti_pack_stamps", "a table one byte short", "smaller than");
    refused(pack(good, scratch, -1), ctx, "vti_pack_stamps", "n_words -1", "n_words");
    refused(vti_pack_stamps(ctx, nullptr, W0.data(), 3, good.data(), 3, n_words, scratch.data(), scratch.size()), ctx, "vti_pack_stamps", "null H0", "null");
    refused(vti_pack_stamps(ctx, H0.data(), W0.data(), 3, nullptr, 3, n_words, scratch.data(), scratch.size()), ctx, "vti_pack_stamps", "null stamps", "null");
    refused(vti_pack_stamps(ctx, H0.data(), W0.data(), 0, good.data(), 3, n_words, scratch.data(), scratch.size()), ctx, "vti_pack_stamps", "no picture", "n_pictures");
    const std::vector<int32_t> tall = {37, 8193, 8};
    refused(vti_pack_stamps(ctx, tall.data(), W0.data(), 3, good.data(), 3, n_words, scratch.data(), scratch.size()), ctx, "vti_pack_stamps", "a picture of 8193 rows", "picture 1");

    // ---- vti_stamp: three pictures of one size -------------------------------------------------------------------------------------
    const std::vector<int32_t> h1 = {37, 37, 37}, w1 = {53, 53, 53};
    const std::vector<vti_stamp_desc> uni = {desc(0, 1, 2, 33, 4, 2, 0), desc(0, 0, 0, 5, 5, 1, 8), desc(2, 2, 2, 6, 6, 3, 13)};
    std::vector<uint8_t> ut((size_t)vti_stamp_table_bytes(3, 3));
    if (vti_pack_stamps(ctx, h1.data(), w1.data(), 3, uni.data(), 3, n_words, ut.data(), ut.size()) != VTI_OK) { fprintf(stderr, "vti_pack_stamps failed\n"); return 2; }
    void* const one = (void*)(uintptr_t)4096;           // fake device pointers, never dereferenced
    struct Call { vti_ctx* ctx; uint8_t* pics; int32_t n, H0, W0; const void* ht; const void* dt; const uint32_t* bits; int64_t n_words; };
    const Call ok = {ctx, (uint8_t*)one, 3, 37, 53, ut.data(), one, (const uint32_t*)one, n_words};
    auto stamp = [](const Call& c) { return vti_stamp(c.ctx, c.pics, c.n, c.H0, c.W0, c.ht, c.dt, c.bits, c.n_words, nullptr); };
    Call c;
    std::vector<uint8_t> bent;
    auto patched = [&](const std::vector<uint8_t>& from, size_t at, int32_t v) { bent = from; memcpy(bent.data() + at, &v, 4); return (const void*)bent.data(); };
    const size_t rec0 = 64 + 3 * 16;
#define REFUSED(change, needle) do { c = ok; change; refused(stamp(c), c.ctx, "vti_stamp", #change, needle); } while (0)
    REFUSED(c.ctx = nullptr, nullptr);
    REFUSED(c.pics = nullptr, "null pointer");
    REFUSED(c.ht = nullptr, "null stamp table");
    REFUSED(c.dt = nullptr, "null stamp table");
    REFUSED(c.bits = nullptr, "null dev_bits");
    REFUSED(c.dt = (void*)(uintptr_t)(4096 + 8), "16-byte aligned");
    REFUSED(c.bits = (const uint32_t*)(uintptr_t)(4096 + 2), "4-byte aligned");
    REFUSED(c.n = 0, "bad size");
    REFUSED(c.n = 2, "another number of pictures");
    REFUSED(c.n = 4, "another number of pictures");
    REFUSED(c.H0 = 8193, "bad size");
    REFUSED(c.H0 = 38, "picture 0 of the stamp table is 37 x 53");
    REFUSED(c.W0 = 54, "picture 0 of the stamp table is 37 x 53");
    REFUSED(c.n_words = n_words - 1, "another n_words");
    REFUSED(c.ht = table.data(), "picture 1 of the stamp table is 64 x 96");       // the table of the three sizes
    REFUSED(c.ht = patched(ut, 0, 7), "not a table of vti_pack_stamps");
    REFUSED(c.ht = patched(ut, rec0 + 16, 60), "stamp 0 of host_table: the rectangle is not inside");      // w = 60
    REFUSED(c.ht = patched(ut, rec0 + 32 + 24, 0), "stamp 1 of host_table: pitch must be >=");
    REFUSED(c.ht = patched(ut, rec0 + 64 + 20, 40), "stamp 2 of host_table: the rectangle is not inside"); // h = 40
    REFUSED(c.ht = patched(ut, rec0 + 64 + 24, 4), "stamp 2 of host_table: its rows run past n_words");    // pitch = 4
    REFUSED(c.ht = patched(ut, 64 + 8, 1), "picture 0 of host_table: its range");
    REFUSED(c.ht = patched(ut, 64 + 32 + 8, 1), "picture 2 of host_table: its range");
    REFUSED(c.ht = patched(ut, 8, 4), "do not cover its stamps");

    // ---- vti_stamp_frames: the three sizes in one flat buffer ----------------------------------------------------------------------
    auto frames = [&](const std::vector<int32_t>& h, const std::vector<int32_t>& w, std::vector<uint8_t>& ft) {
        std::vector<int64_t> at;
        int64_t total = 0;
        for (size_t k = 0; k < h.size(); ++k) { at.push_back(total); total = (total + 3LL * h[k] * w[k] + 15) & ~15LL; }
        ft.resize((size_t)vti_frame_table_bytes((int32_t)h.size()));        // exactly the table's bytes on the heap
        return vti_pack_frames(ctx, d.H, d.W, h.data(), w.data(), at.data(), (int32_t)h.size(), total, ft.data(), ft.size());
    };
    std::vector<uint8_t> ft, ft_other, ft_two;
    const std::vector<int32_t> h2 = {37, 64, 9}, w2 = {53, 96, 8}, h3 = {37, 64}, w3 = {53, 96};
    if (frames(H0, W0, ft) != VTI_OK || frames(h2, w2, ft_other) != VTI_OK || frames(h3, w3, ft_two) != VTI_OK) { fprintf(stderr, "vti_pack_frames failed\n"); return 2; }
    struct FCall { vti_ctx* ctx; uint8_t* buf; const void* hft; const void* dft; int32_t n; const void* ht; const void* dt; const uint32_t* bits; int64_t n_words; };
    const FCall fok = {ctx, (uint8_t*)one, ft.data(), one, 3, table.data(), one, (const uint32_t*)one, n_words};
    auto stamp_frames = [](const FCall& c) { return vti_stamp_frames(c.ctx, c.buf, c.hft, c.dft, c.n, c.ht, c.dt, c.bits, c.n_words, nullptr); };
    FCall f;
#define FREFUSED(change, needle) do { f = fok; change; refused(stamp_frames(f), f.ctx, "vti_stamp_frames", #change, needle); } while (0)
    FREFUSED(f.ctx = nullptr, nullptr);
    FREFUSED(f.buf = nullptr, "null pointer");
    FREFUSED(f.buf = (uint8_t*)(uintptr_t)(4096 + 8), "dev_buf must be 16-byte aligned");
    FREFUSED(f.hft = nullptr, "null frame table");
    FREFUSED(f.dft = nullptr, "null frame table");
    FREFUSED(f.dft = (void*)(uintptr_t)(4096 + 8), "device frame table must be 16-byte aligned");
    FREFUSED(f.n = 2, "another B");
    FREFUSED(f.hft = ft_two.data(), "another B");
    FREFUSED(f.hft = patched(ft, 64 + 64, 1), "frame 1 of host_table");               // row 1: a byte offset that is no multiple of 16
    FREFUSED(f.hft = ft_other.data(), "picture 2 of the stamp table is 8 x 8, the call's is 9 x 8");
    FREFUSED(f.ht = ut.data(), "picture 1 of the stamp table is 37 x 53, the call's is 64 x 96");
    FREFUSED(f.ht = nullptr, "null stamp table");
    FREFUSED(f.dt = (void*)(uintptr_t)(4096 + 4), "16-byte aligned");
    FREFUSED(f.bits = nullptr, "null dev_bits");
    FREFUSED(f.n_words = n_words + 1, "another n_words");
    FREFUSED(f.ht = patched(table, rec0 + 64 + 8, 3), "stamp 2 of host_table: the rectangle is not inside");   // x = 3 in a picture of 8 columns

    vti_destroy(ctx);
    if (failures) return 1;
    printf("ok %d\n", checks);
    return 0;
}
