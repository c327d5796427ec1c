// csrc/jpeg_decode_dev.h compiled for the HOST: vti_decode_jpeg's stages run lane by lane on a descriptor table that libvti.so's
// vti_decode_jpeg_plan packed, so tests/test_jpeg_decode_host.py can hold the segment decoder, the rounds of the self-synchronising
// scheme, the block-count scan, the DC sums, the IDCT, the upsampling and the colour conversion to jpeg.decode without a GPU.  The
// phases are those of csrc/jpeg_decode.hip's kernels, one loop over the lanes where the kernel has a barrier.
#define VTI_HD
#include "jpeg_decode_dev.h"

#include <vector>

using namespace vti;
using namespace vti::jpd;

static const unsigned char kZig[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                                       28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                                       54, 47, 55, 62, 63};

static void entropy(const uint8_t* files, const JpegDecRow* R, uint8_t* scratch, int* info, int W) {
    const uint8_t* scan = files + R->scan_start;
    const long long scan_len = R->scan_end - R->scan_start, SB = R->seg_bytes;
    const int nseg = R->nseg;
    unsigned long long* entry = (unsigned long long*)(scratch + R->off_seg);
    unsigned long long* exitst = entry + nseg;
    SegSum* sums = (SegSum*)(exitst + nseg);
    SegSum* base = sums + nseg;
    int16_t* coef = (int16_t*)(scratch + R->off_coef);
    int err = 0, done = 0;
    for (int s = 0; s < nseg; ++s) {
        long long b = s * SB;
        if (s > 0 && scan[b - 1] == 0xFF) ++b;
        const unsigned long long E = (unsigned long long)(b * 8) << 16;
        entry[s] = E;
        decode_segment<false>(R, R->huff, scan, scan_len, (s + 1) * SB * 8, E, exitst[s], sums[s], 0, 0, coef, err, done);
    }
    int rounds = 1;
    for (int r = 1; r < nseg; ++r) {
        for (int s = 0; s < nseg; ++s) {
            unsigned dirty = 0;
            if (s > 0 && exitst[s - 1] != entry[s]) {
                entry[s] = exitst[s - 1];
                dirty = 1;
            }
            base[s].nrst = dirty;
        }
        int changed = 0;
        std::vector<unsigned long long> X(nseg);
        for (int s = 0; s < nseg; ++s) X[s] = exitst[s];
        for (int s = 0; s < nseg; ++s) {
            if (!base[s].nrst) continue;
            decode_segment<false>(R, R->huff, scan, scan_len, (s + 1) * SB * 8, entry[s], X[s], sums[s], 0, 0, coef, err, done);
            changed = 1;
        }
        for (int s = 0; s < nseg; ++s) exitst[s] = X[s];
        if (!changed) break;
        ++rounds;
    }
    const int per = (nseg + W - 1) / W;
    std::vector<unsigned> sn(W), sa(W);
    for (int t = 0; t < W; ++t) {
        const int s0 = t * per < nseg ? t * per : nseg, s1 = s0 + per < nseg ? s0 + per : nseg;
        unsigned n = 0, a = 0;
        for (int s = s0; s < s1; ++s) {
            a = sums[s].nrst ? sums[s].cnt : a + sums[s].cnt;
            n += sums[s].nrst;
        }
        sn[t] = n;
        sa[t] = a;
    }
    {
        unsigned n = 0, a = 0;
        for (int t = 0; t < W; ++t) {
            const unsigned tn = sn[t], ta = sa[t];
            sn[t] = n;
            sa[t] = a;
            a = tn ? ta : a + ta;
            n += tn;
        }
    }
    for (int t = 0; t < W; ++t) {
        const int s0 = t * per < nseg ? t * per : nseg, s1 = s0 + per < nseg ? s0 + per : nseg;
        unsigned n = sn[t], a = sa[t];
        for (int s = s0; s < s1; ++s) {
            const SegSum v = sums[s];
            base[s].nrst = n;
            base[s].cnt = a;
            a = v.nrst ? v.cnt : a + v.cnt;
            n += v.nrst;
        }
    }
    const long long IB = (long long)R->ri * R->bpm;
    for (int s = 0; s < nseg; ++s) {
        const SegSum b = base[s];
        const long long begun = b.nrst ? (long long)b.nrst * IB + b.cnt : b.cnt;
        SegSum sm;
        unsigned long long X;
        decode_segment<true>(R, R->huff, scan, scan_len, (s + 1) * SB * 8, entry[s], X, sm, begun, b.nrst, coef, err, done);
    }
    const SegSum b = base[nseg - 1], v = sums[nseg - 1];
    const long long nr = (long long)b.nrst + v.nrst, a = v.nrst ? v.cnt : (long long)b.cnt + v.cnt;
    const long long total = nr ? nr * IB + a : a;
    info[0] = (err || !done) ? 1 : 0;
    info[1] = nseg;
    info[2] = rounds;
    info[3] = (int)(total < R->nblk ? total : R->nblk);
}

static void dc_sums(const JpegDecRow* R, uint8_t* scratch) {
    int16_t* coef = (int16_t*)(scratch + R->off_coef);
    const int bpm = R->bpm, ri = R->ri;
    for (int c = 0; c < 3; ++c) {
        const int nb = c == 0 ? bpm - 2 : 1, first = c == 0 ? 0 : bpm - 3 + c, N = R->mcu_rows * R->mcu_cols * nb;
        int sum = 0;
        for (int i = 0; i < N; ++i) {
            const int mcu = i / nb, j = i - mcu * nb;
            if (ri && j == 0 && mcu % ri == 0) sum = 0;
            int16_t* p = coef + ((long long)mcu * bpm + first + j) * 64;
            sum += *p;
            *p = (int16_t)sum;
        }
    }
}

static void idct(const JpegDecRow* R, uint8_t* scratch) {
    const int bpm = R->bpm, hs = R->hs, vs = R->vs, nmcu = R->mcu_rows * R->mcu_cols;
    const int PW = R->mcu_cols * 8 * hs, PH = R->mcu_rows * 8 * vs, CW = R->mcu_cols * 8, CH = R->mcu_rows * 8;
    uint8_t* Y = scratch + R->off_planes;
    uint8_t* C = Y + (long long)PW * PH;
    for (int m = 0; m < nmcu; ++m) {
        const int my = m / R->mcu_cols, mx = m - my * R->mcu_cols;
        const int16_t* cf = (const int16_t*)(scratch + R->off_coef) + (long long)m * bpm * 64;
        int tile[6 * 72];
        for (int b = 0; b < bpm; ++b) {
            const int comp = b < bpm - 2 ? 0 : b - (bpm - 2) + 1;
            for (int lane = 0; lane < 64; ++lane)
                tile[b * 72 + (kZig[lane] >> 3) * 9 + (kZig[lane] & 7)] = (int)cf[b * 64 + lane] * (int)R->quant[comp][lane];
        }
        for (int lane = 0; lane < 8 * bpm; ++lane) idct_pass<11>(tile + (lane >> 3) * 72 + (lane & 7), 9);
        for (int lane = 0; lane < 8 * bpm; ++lane) idct_pass<18>(tile + 9 * lane, 1);
        for (int b = 0; b < bpm; ++b)
            for (int r = 0; r < 8; ++r)
                for (int c = 0; c < 8; ++c) {
                    const uint8_t px = (uint8_t)range_limit(tile[b * 72 + r * 9 + c]);
                    if (b < bpm - 2) {
                        const int by = b / hs, bx = b - by * hs;
                        Y[(long long)(my * 8 * vs + by * 8 + r) * PW + mx * 8 * hs + bx * 8 + c] = px;
                    } else {
                        C[(long long)(b - (bpm - 2)) * CW * CH + (long long)(my * 8 + r) * CW + mx * 8 + c] = px;
                    }
                }
    }
}

static void colour(const JpegDecRow* R, const uint8_t* scratch, int rgb, uint8_t* out) {
    const int H0 = R->H0, W0 = R->W0, hs = R->hs, vs = R->vs;
    const int PW = R->mcu_cols * 8 * hs, PH = R->mcu_rows * 8 * vs, CW = R->mcu_cols * 8, CH = R->mcu_rows * 8;
    const int ch = (H0 + vs - 1) / vs, cw = (W0 + hs - 1) / hs;
    const uint8_t* Y = scratch + R->off_planes;
    const uint8_t* Cb = Y + (long long)PW * PH;
    const uint8_t* Cr = Cb + (long long)CW * CH;
    for (int y = 0; y < H0; ++y)
        for (int x = 0; x < W0; ++x)
            store_pixel(Y[(long long)y * PW + x], chroma_at(Cb, CW, ch, cw, hs, vs, y, x) - 128, chroma_at(Cr, CW, ch, cw, hs, vs, y, x) - 128,
                        rgb, out + R->out_off + ((long long)y * W0 + x) * 3);
}

// files, table: what vti_decode_jpeg_plan parsed and wrote; out, scratch: of the plan's sizes; info i32 [n, 4]; lanes: the lanes of
// the entropy stage's workgroup (the chunks of its scan)
extern "C" void jpegd_emulate(const uint8_t* files, const uint8_t* table, int n, int rgb, uint8_t* out, int* info, uint8_t* scratch, int lanes) {
    const JpegDecRow* rows = (const JpegDecRow*)(table + sizeof(JpegDecHeader));
    for (int f = 0; f < n; ++f) {
        const JpegDecRow* R = rows + f;
        for (long long i = 0; i < (long long)R->nblk * 128; ++i) scratch[R->off_coef + i] = 0;
        entropy(files, R, scratch, info + 4 * f, lanes);
        dc_sums(R, scratch);
        idct(R, scratch);
        colour(R, scratch, rgb, out);
    }
}
