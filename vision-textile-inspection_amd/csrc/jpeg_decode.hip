// vti_decode_jpeg: baseline JPEG files (what a motion-JPEG camera delivers, what vti_encode_jpeg and cv2.imwrite save) -> frames on
// the device, byte for byte the package's jpeg.decode (libjpeg's defaults: jdhuff.c, jidctint.c, jdsample.c fancy upsampling,
// jdcolor.c).  The host parses and validates every header (decode_jpeg_parse) and packs one descriptor row per file; the kernels
// read the scan's bytes only.
//
// Five launches on one stream, no host synchronisation:
//   1 zero      the coefficient words the file uses
//   2 entropy   one workgroup per file.  The scan is cut into segments of segment_bytes.  Pass 1: every lane decodes its segments
//               from a guessed state (block 0 of the MCU, coefficient 0) and records its exit state (bit position, block within the
//               MCU, zigzag index) and the blocks it began; then rounds, separated by workgroup barriers: a segment whose entry state
//               differs from its predecessor's exit state is decoded again from that state.  Segment 0's entry is true, so after k
//               rounds segments 0..k are final; the loop is bounded by the segment count and ends when nothing changed (the
//               self-synchronising decode of Weissenberger & Schmidt).  Then the exclusive scan of the block counts (restart
//               markers restart it at a multiple of the interval), and pass 2: every segment once more from its true entry state,
//               coefficients to coef[block][zigzag], DC values as differences.
//   3 dc        per (file, component): the prefix sum of the DC differences in scan order, restarted at every restart boundary
//   4 idct      one wave per MCU: dequantisation + jpeg_idct_islow -> the Y, Cb, Cr planes (u8)
//   5 colour    per pixel: fancy upsampling of the chroma planes, YCbCr -> RGB, three byte stores at any address
//
// Bounds hold by construction: every read of the file is clamped to the scan's byte range, every coefficient store is guarded by the
// header's block count, a run past coefficient 63 is dropped, shift counts are at most 63, every loop has a size-derived bound.
#include "vti_internal.h"

#include <cstring>

namespace vti {
using namespace jpd;
namespace {

constexpr int kEntropyThreads = 1024;
constexpr uint8_t kZigD[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                               54, 47, 55, 62, 63};
struct ZigTabD { uint8_t z[64]; };
constexpr ZigTabD make_zig_d() {
    ZigTabD t = {};
    for (int i = 0; i < 64; ++i) t.z[i] = kZigD[i];
    return t;
}
__device__ const ZigTabD d_zig_d = make_zig_d();

__device__ inline const JpegDecRow* row_of(const void* table, int f) {
    return (const JpegDecRow*)((const uint8_t*)table + sizeof(JpegDecHeader)) + f;
}

// 1: grid (x, file): zero the file's coefficients, 16 bytes per lane (the area is 256-byte aligned and a multiple of 128 bytes)
__global__ __launch_bounds__(256) void jpegd_zero_kernel(const void* __restrict__ table, uint8_t* __restrict__ scratch) {
    const JpegDecRow* R = row_of(table, blockIdx.y);
    uint4* p = (uint4*)(scratch + R->off_coef);
    const long long n16 = (long long)R->nblk * 8;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

// 2: one workgroup per file
__global__ __launch_bounds__(kEntropyThreads) void jpegd_entropy_kernel(const uint8_t* __restrict__ files, const void* __restrict__ table,
                                                                        uint8_t* __restrict__ scratch, int* __restrict__ info) {
    __shared__ JpegDHuff s_huff[6];
    __shared__ unsigned s_n[kEntropyThreads], s_a[kEntropyThreads];
    __shared__ int s_changed, s_err, s_done;
    const JpegDecRow* R = row_of(table, blockIdx.x);
    const int tid = threadIdx.x, W = kEntropyThreads;
    {
        const unsigned* src = (const unsigned*)R->huff;
        unsigned* dst = (unsigned*)s_huff;
        for (int i = tid; i < (int)(sizeof(s_huff) / 4); i += W) dst[i] = src[i];
    }
    if (tid == 0) { s_changed = 0; s_err = 0; s_done = 0; }
    const uint8_t* scan = files + R->scan_start;
    const long long scan_len = R->scan_end - R->scan_start;
    const int nseg = R->nseg;
    const long long SB = R->seg_bytes;
    unsigned long long* entry = (unsigned long long*)(scratch + R->off_seg);
    unsigned long long* exitst = entry + nseg;
    SegSum* sums = (SegSum*)(exitst + nseg);
    SegSum* base = sums + nseg;                 // pass 1: .nrst = the segment is to be decoded again; then the exclusive scan
    int16_t* coef = (int16_t*)(scratch + R->off_coef);
    __syncthreads();
    int err = 0, done = 0;
    // pass 1, round 0: guessed states
    for (int s = tid; s < nseg; s += W) {
        long long b = s * SB;
        if (s > 0 && scan[b - 1] == 0xFF) ++b;          // a stuffed 0x00 or a marker's second byte is no place to start
        const unsigned long long E = (unsigned long long)(b * 8) << 16;
        entry[s] = E;
        SegSum sm;
        unsigned long long X;
        decode_segment<false>(R, s_huff, scan, scan_len, (s + 1) * SB * 8, E, X, sm, 0, 0, coef, err, done);
        exitst[s] = X;
        sums[s] = sm;
    }
    int rounds = 1;
    for (int r = 1; r < nseg; ++r) {
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (int s = tid; s < nseg; s += W) {
            unsigned dirty = 0;
            if (s > 0) {
                const unsigned long long E = exitst[s - 1];
                if (E != entry[s]) {
                    entry[s] = E;
                    dirty = 1;
                }
            }
            base[s].nrst = dirty;
        }
        __syncthreads();
        int any = 0;
        for (int s = tid; s < nseg; s += W) {
            if (!base[s].nrst) continue;
            SegSum sm;
            unsigned long long X;
            decode_segment<false>(R, s_huff, scan, scan_len, (s + 1) * SB * 8, entry[s], X, sm, 0, 0, coef, err, done);
            exitst[s] = X;
            sums[s] = sm;
            any = 1;
        }
        if (any) atomicOr(&s_changed, 1);
        __syncthreads();
        const int ch = s_changed;
        __syncthreads();
        if (!ch) break;
        ++rounds;
    }
    __syncthreads();
    // the exclusive scan of (markers, blocks since the last marker): (n1, a1) . (n2, a2) = (n1 + n2, n2 ? a2 : a1 + a2)
    const int per = (nseg + W - 1) / W;
    const int s0 = min(tid * per, nseg), s1 = min(s0 + per, nseg);
    {
        unsigned n = 0, a = 0;
        for (int s = s0; s < s1; ++s) {
            const SegSum v = sums[s];
            a = v.nrst ? v.cnt : a + v.cnt;
            n += v.nrst;
        }
        s_n[tid] = n;
        s_a[tid] = a;
    }
    __syncthreads();
    if (tid == 0) {
        unsigned n = 0, a = 0;
        for (int t = 0; t < W; ++t) {
            const unsigned tn = s_n[t], ta = s_a[t];
            s_n[t] = n;
            s_a[t] = a;
            a = tn ? ta : a + ta;
            n += tn;
        }
    }
    __syncthreads();
    {
        unsigned n = s_n[tid], a = s_a[tid];
        for (int s = s0; s < s1; ++s) {
            const SegSum v = sums[s];
            base[s].nrst = n;
            base[s].cnt = a;
            a = v.nrst ? v.cnt : a + v.cnt;
            n += v.nrst;
        }
    }
    __syncthreads();
    // pass 2: true entry states
    const long long IB = (long long)R->ri * R->bpm;
    for (int s = tid; s < nseg; s += W) {
        const SegSum b = base[s];
        const long long begun = b.nrst ? (long long)b.nrst * IB + b.cnt : b.cnt;
        SegSum sm;
        unsigned long long X;
        decode_segment<true>(R, s_huff, scan, scan_len, (s + 1) * SB * 8, entry[s], X, sm, begun, b.nrst, coef, err, done);
    }
    if (err) atomicOr(&s_err, 1);
    if (done) atomicOr(&s_done, 1);
    __syncthreads();
    if (tid == 0) {
        const SegSum b = base[nseg - 1], v = sums[nseg - 1];
        const long long nr = (long long)b.nrst + v.nrst, a = v.nrst ? v.cnt : (long long)b.cnt + v.cnt;
        const long long total = nr ? nr * IB + a : a;
        int* o = info + 4 * blockIdx.x;
        o[0] = (s_err || !s_done) ? VTI_JPEG_CORRUPT : 0;
        o[1] = nseg;
        o[2] = rounds;
        o[3] = (int)(total < R->nblk ? total : R->nblk);
    }
}

// 3: grid (component, file): the DC values from their differences.  Item i of component c is block (i / nb) * bpm + first + i % nb
// (nb blocks per MCU); the sum restarts at the first block of every restart interval.
__global__ __launch_bounds__(256) void jpegd_dc_kernel(const void* __restrict__ table, uint8_t* __restrict__ scratch) {
    __shared__ int s_sum[256], s_rst[256];
    const JpegDecRow* R = row_of(table, blockIdx.y);
    const int c = blockIdx.x, tid = threadIdx.x, bpm = R->bpm, ri = R->ri;
    const int nb = c == 0 ? bpm - 2 : 1, first = c == 0 ? 0 : bpm - 3 + c;
    const int N = R->mcu_rows * R->mcu_cols * nb;
    int16_t* coef = (int16_t*)(scratch + R->off_coef);
    const int per = (N + 255) / 256;
    const int i0 = min(tid * per, N), i1 = min(i0 + per, N);
    int sum = 0, rst = 0;
    for (int i = i0; i < i1; ++i) {
        const int mcu = i / nb, j = i - mcu * nb;
        if (ri && j == 0 && mcu % ri == 0) { sum = 0; rst = 1; }
        sum += coef[((long long)mcu * bpm + first + j) * 64];
    }
    s_sum[tid] = sum;
    s_rst[tid] = rst;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int t = 0; t < 256; ++t) {
            const int ts = s_sum[t], tr = s_rst[t];
            s_sum[t] = run;
            run = tr ? ts : run + ts;
        }
    }
    __syncthreads();
    sum = s_sum[tid];
    for (int i = i0; i < i1; ++i) {
        const int mcu = i / nb, j = i - mcu * nb;
        if (ri && j == 0 && mcu % ri == 0) sum = 0;
        int16_t* p = coef + ((long long)mcu * bpm + first + j) * 64;
        sum += *p;
        *p = (int16_t)sum;
    }
}

// 4: grid (x, file): one wave per MCU, four MCUs per workgroup.  The tile is jpeg_blocks_kernel's: 6 blocks of 8 rows pitched by 9
// ints, so the column pass (lane = block * 8 + column, address 72 * block + column + 9 * k) and the row pass (address 9 * lane + k)
// both touch distinct banks.
__global__ __launch_bounds__(256) void jpegd_idct_kernel(const void* __restrict__ table, uint8_t* __restrict__ scratch) {
    __shared__ int s_tile[4][6 * 72];
    const JpegDecRow* R = row_of(table, blockIdx.y);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nmcu = R->mcu_rows * R->mcu_cols, bpm = R->bpm, hs = R->hs, vs = R->vs;
    if ((long long)blockIdx.x * 4 >= nmcu) return;                      // the whole workgroup
    int m = blockIdx.x * 4 + wid;
    const bool live = m < nmcu;
    if (!live) m = nmcu - 1;
    const int my = m / R->mcu_cols, mx = m - my * R->mcu_cols;
    const int16_t* cf = (const int16_t*)(scratch + R->off_coef) + (long long)m * bpm * 64;
    int* tile = s_tile[wid];
    const int nat = d_zig_d.z[lane], at = (nat >> 3) * 9 + (nat & 7);
    for (int b = 0; b < bpm; ++b) {
        const int comp = b < bpm - 2 ? 0 : b - (bpm - 2) + 1;
        tile[b * 72 + at] = (int)cf[b * 64 + lane] * (int)R->quant[comp][lane];
    }
    __syncthreads();
    if (lane < 8 * bpm) idct_pass<11>(tile + (lane >> 3) * 72 + (lane & 7), 9);
    __syncthreads();
    if (lane < 8 * bpm) idct_pass<18>(tile + 9 * lane, 1);
    __syncthreads();
    if (!live) return;
    const int PW = R->mcu_cols * 8 * hs, PH = R->mcu_rows * 8 * vs, CW = R->mcu_cols * 8, CH = R->mcu_rows * 8;
    uint8_t* Y = scratch + R->off_planes;
    uint8_t* C = Y + (long long)PW * PH;
    const int r = lane >> 3, c = lane & 7;
    for (int b = 0; b < bpm; ++b) {
        const uint8_t px = (uint8_t)range_limit(tile[b * 72 + r * 9 + c]);
        if (b < bpm - 2) {
            const int by = b / hs, bx = b - by * hs;
            Y[(long long)(my * 8 * vs + by * 8 + r) * PW + mx * 8 * hs + bx * 8 + c] = px;
        } else {
            C[(long long)(b - (bpm - 2)) * CW * CH + (long long)(my * 8 + r) * CW + mx * 8 + c] = px;
        }
    }
}

// 5: grid (x, file): one pixel per lane and step
__global__ __launch_bounds__(256) void jpegd_colour_kernel(const void* __restrict__ table, const uint8_t* __restrict__ scratch, int rgb,
                                                           uint8_t* __restrict__ out) {
    const JpegDecRow* R = row_of(table, blockIdx.y);
    const int H0 = R->H0, W0 = R->W0, hs = R->hs, vs = R->vs;
    const int PW = R->mcu_cols * 8 * hs, PH = R->mcu_rows * 8 * vs, CW = R->mcu_cols * 8, CH = R->mcu_rows * 8;
    const int ch = (H0 + vs - 1) / vs, cw = (W0 + hs - 1) / hs;
    const uint8_t* Y = scratch + R->off_planes;
    const uint8_t* Cb = Y + (long long)PW * PH;
    const uint8_t* Cr = Cb + (long long)CW * CH;
    uint8_t* o = out + R->out_off;
    const long long npx = (long long)H0 * W0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npx; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / W0), x = (int)(i - (long long)y * W0);
        const int yy = Y[(long long)y * PW + x];
        const int cb = chroma_at(Cb, CW, ch, cw, hs, vs, y, x) - 128, cr = chroma_at(Cr, CW, ch, cw, hs, vs, y, x) - 128;
        store_pixel(yy, cb, cr, rgb, o + i * 3);
    }
}

// Annex K.3, for files without DHT segments (motion-JPEG)
const uint8_t kStdDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
const uint8_t kStdAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
const uint8_t kStdAcVals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
     0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
     0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
     0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
     0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
     0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
     0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
     0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
     0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
     0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
     0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
     0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
     0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
     0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};

struct RawHuff { bool set = false; uint8_t bits[16] = {}; uint8_t vals[256] = {}; int count = 0; };

// jpeg_make_d_derived_tbl; false for a table whose code lengths overflow the code space
bool derive_huff(const RawHuff& h, JpegDHuff& T) {
    memset(&T, 0, sizeof T);
    for (int l = 0; l < 18; ++l) T.maxcode[l] = -1;
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        const int cnt = h.bits[len - 1];
        if (cnt) {
            T.valoff[len] = k - code;
            for (int i = 0; i < cnt; ++i, ++code, ++k) {
                if (code >= (1 << len)) return false;
                if (len <= 9)
                    for (int f = code << (9 - len); f < (code + 1) << (9 - len); ++f) T.look[f] = (uint16_t)((len << 8) | h.vals[k]);
            }
            T.maxcode[len] = code - 1;
        }
        code <<= 1;
    }
    T.maxcode[17] = 0xFFFFF;
    memcpy(T.val, h.vals, 256);
    return h.count > 0;
}

}  // namespace

int decode_jpeg_parse(const uint8_t* d, long long n, JpegDecRow& R, std::string& err) {
    auto bad = [&](const char* m) { err = m; return (int)VTI_ERR_ARG; };
    auto unsupported = [&](const std::string& m) { err = m; return (int)VTI_ERR_UNSUPPORTED; };
    memset(&R, 0, sizeof R);
    if (n < 4 || d[0] != 0xFF || d[1] != 0xD8) return bad("not a JPEG file: no SOI marker");
    uint8_t qt[4][64];
    bool qt_set[4] = {};
    RawHuff dc[4], ac[4];
    bool any_dht = false, jfif = false, have_sof = false;
    int adobe = -1, ri = 0;
    uint8_t sof[6 + 3 * 4] = {};
    long long p = 2, L = 0;
    const uint8_t* body = nullptr;
    long long blen = 0;
    for (;;) {
        if (p >= n) return bad("truncated header: no SOS marker");
        if (d[p] != 0xFF) return bad("malformed header: a byte that is no marker between two segments");
        while (p < n && d[p] == 0xFF) ++p;
        if (p >= n) return bad("truncated header");
        const int m = d[p++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        if (m == 0xD9) return bad("EOI before any scan");
        if (p + 2 > n) return bad("truncated header");
        L = ((long long)d[p] << 8) | d[p + 1];
        if (L < 2 || p + L > n) return bad("truncated header: a segment runs past the end of the file");
        body = d + p + 2;
        blen = L - 2;
        if (m == 0xC0) {
            if (have_sof) return bad("two SOF markers");
            if (blen < 6 || blen != 6 + 3 * body[5]) return bad("bad SOF0 length");
            if (body[5] > 4) return unsupported("more than four components");
            memcpy(sof, body, (size_t)blen);
            have_sof = true;
        } else if (m == 0xC2) {
            return unsupported("progressive JPEG: only baseline sequential (SOF0) is decoded");
        } else if (m == 0xC1) {
            return unsupported("extended sequential JPEG: only baseline sequential (SOF0) is decoded");
        } else if (m == 0xC3 || m == 0xC5 || m == 0xC6 || m == 0xC7) {
            return unsupported("lossless or differential JPEG: only baseline sequential (SOF0) is decoded");
        } else if (m >= 0xC9 && m <= 0xCF) {
            return unsupported("arithmetic coding is not decoded");
        } else if (m == 0xDB) {
            for (long long q = 0; q < blen; q += 65) {
                const int pq = body[q] >> 4, tq = body[q] & 15;
                if (pq == 1) return unsupported("16-bit quantisation table");
                if (pq || tq > 3 || q + 65 > blen) return bad("bad DQT segment");
                memcpy(qt[tq], body + q + 1, 64);
                qt_set[tq] = true;
            }
        } else if (m == 0xC4) {
            for (long long q = 0; q < blen;) {
                if (q + 17 > blen) return bad("bad DHT segment");
                const int tc = body[q] >> 4, th = body[q] & 15;
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += body[q + 1 + i];
                if (tc > 1 || th > 3 || cnt > 256 || cnt < 1 || q + 17 + cnt > blen) return bad("bad DHT segment");
                RawHuff& h = tc ? ac[th] : dc[th];
                h = RawHuff();
                h.set = true;
                h.count = cnt;
                memcpy(h.bits, body + q + 1, 16);
                memcpy(h.vals, body + q + 17, (size_t)cnt);
                JpegDHuff T;
                if (!derive_huff(h, T)) return bad("bad Huffman table");
                any_dht = true;
                q += 17 + cnt;
            }
        } else if (m == 0xDD) {
            if (blen != 2) return bad("bad DRI segment");
            ri = (body[0] << 8) | body[1];
        } else if (m == 0xE0 && blen >= 5 && !memcmp(body, "JFIF\0", 5)) {
            jfif = true;
        } else if (m == 0xEE && blen >= 12 && !memcmp(body, "Adobe", 5)) {
            adobe = body[11];
        } else if (m == 0xDA) {
            break;
        }
        p += L;
    }
    if (!have_sof) return bad("SOS before SOF");
    const int prec = sof[0], H0 = (sof[1] << 8) | sof[2], W0 = (sof[3] << 8) | sof[4], nc = sof[5];
    if (prec != 8) return unsupported(std::to_string(prec) + "-bit samples: only 8-bit is decoded");
    if (nc == 1) return unsupported("greyscale file: only three-component YCbCr is decoded");
    if (nc != 3) return unsupported(std::to_string(nc) + " components: only three-component YCbCr is decoded");
    if (H0 < 1 || W0 < 1 || H0 > 8192 || W0 > 8192) return unsupported("frame size " + std::to_string(H0) + "x" + std::to_string(W0) + " outside 1..8192");
    int cid[3], ch[3], cv[3], cq[3];
    for (int i = 0; i < 3; ++i) {
        cid[i] = sof[6 + 3 * i];
        ch[i] = sof[7 + 3 * i] >> 4;
        cv[i] = sof[7 + 3 * i] & 15;
        cq[i] = sof[8 + 3 * i];
    }
    if (adobe >= 0 && adobe != 1) return unsupported("Adobe transform " + std::to_string(adobe) + ": only YCbCr (transform 1) is decoded");
    if (adobe < 0 && !jfif && cid[0] == 82 && cid[1] == 71 && cid[2] == 66) return unsupported("RGB components: only YCbCr is decoded");
    const int hs = ch[0], vs = cv[0];
    if (!((hs == 2 && vs == 2) || (hs == 2 && vs == 1) || (hs == 1 && vs == 1)) || ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1)
        return unsupported("sampling factors: only 2x2, 2x1 or 1x1 luma with 1x1 chroma is decoded");
    if (blen < 1 || blen != 4 + 2 * body[0]) return bad("bad SOS length");
    if (body[0] != 3) return unsupported("a scan that does not interleave all three components (multiple scans)");
    int sdc[3], sac[3];
    for (int i = 0; i < 3; ++i) {
        if (body[1 + 2 * i] != cid[i]) return unsupported("scan components out of frame order");
        sdc[i] = body[2 + 2 * i] >> 4;
        sac[i] = body[2 + 2 * i] & 15;
    }
    if (body[7] != 0 || body[8] != 63 || body[9] != 0) return unsupported("spectral selection or successive approximation in a sequential scan");
    if (!any_dht) {
        for (int t = 0; t < 2; ++t) {
            dc[t].set = ac[t].set = true;
            dc[t].count = 12;
            ac[t].count = 162;
            memcpy(dc[t].bits, kStdDcBits[t], 16);
            memcpy(ac[t].bits, kStdAcBits[t], 16);
            for (int i = 0; i < 12; ++i) dc[t].vals[i] = (uint8_t)i;
            memcpy(ac[t].vals, kStdAcVals[t], 162);
        }
    }
    for (int i = 0; i < 3; ++i) {
        if (cq[i] > 3 || !qt_set[cq[i]]) return bad("a component uses a quantisation table the file does not define");
        if (sdc[i] > 3 || sac[i] > 3 || !dc[sdc[i]].set || !ac[sac[i]].set) return bad("a component uses a Huffman table the file does not define");
        for (int k = 0; k < 64; ++k) {
            if (!qt[cq[i]][k]) return bad("a quantisation step of 0");
            R.quant[i][k] = qt[cq[i]][k];
        }
        if (!derive_huff(dc[sdc[i]], R.huff[i]) || !derive_huff(ac[sac[i]], R.huff[3 + i])) return bad("bad Huffman table");
    }
    const long long scan_start = p + L;
    long long q = scan_start, scan_end = n;
    while (q + 1 < n) {
        if (d[q] != 0xFF) { ++q; continue; }
        const int m = d[q + 1];
        if (m == 0 || (m >= 0xD0 && m <= 0xD7)) { q += 2; continue; }
        if (m == 0xFF) { ++q; continue; }
        scan_end = q;
        break;
    }
    for (long long r = scan_end; r + 1 < n; ++r) {
        if (d[r] == 0xFF && d[r + 1] == 0xDA) return unsupported("multiple scans");
        if (d[r] == 0xFF && d[r + 1] == 0xD9) break;
    }
    if (scan_end - scan_start > (1LL << 28)) return unsupported("a scan of more than 2^28 bytes");
    R.H0 = H0;
    R.W0 = W0;
    R.hs = hs;
    R.vs = vs;
    R.mcu_rows = (H0 + 8 * vs - 1) / (8 * vs);
    R.mcu_cols = (W0 + 8 * hs - 1) / (8 * hs);
    R.bpm = hs * vs + 2;
    R.nblk = R.mcu_rows * R.mcu_cols * R.bpm;
    R.ri = ri;
    R.scan_start = scan_start;
    R.scan_end = scan_end;
    R.file_len = n;
    return 0;
}

static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

size_t decode_jpeg_scratch_of(JpegDecRow& R, size_t at) {
    R.off_seg = (long long)at;
    at += al256((size_t)R.nseg * 32);
    R.off_coef = (long long)at;
    at += al256((size_t)R.nblk * 128);
    R.off_planes = (long long)at;
    at += al256((size_t)R.mcu_rows * R.mcu_cols * 64 * (R.hs * R.vs + 2));
    return at;
}

bool decode_jpeg_row_ok(const JpegDecRow& R, const JpegDecHeader& H, size_t& scratch_at, std::string& why) {
    auto no = [&](const char* m) { why = m; return false; };
    if (R.H0 < 1 || R.W0 < 1 || R.H0 > 8192 || R.W0 > 8192) return no("frame size");
    if (!((R.hs == 2 && R.vs == 2) || (R.hs == 2 && R.vs == 1) || (R.hs == 1 && R.vs == 1))) return no("sampling");
    if (R.mcu_rows != (R.H0 + 8 * R.vs - 1) / (8 * R.vs) || R.mcu_cols != (R.W0 + 8 * R.hs - 1) / (8 * R.hs) || R.bpm != R.hs * R.vs + 2 ||
        R.nblk != R.mcu_rows * R.mcu_cols * R.bpm)
        return no("MCU geometry");
    if (R.ri < 0 || R.ri > 65535) return no("restart interval");
    if (R.file_off < 0 || R.file_len < 4 || R.file_off + R.file_len > H.files_bytes) return no("file range");
    if (R.scan_start < R.file_off || R.scan_end < R.scan_start || R.scan_end > R.file_off + R.file_len || R.scan_end - R.scan_start > (1LL << 28))
        return no("scan range");
    const int sb = R.seg_bytes;
    if (sb != H.seg_bytes || sb < 16 || sb > 4096 || (sb & (sb - 1))) return no("segment size");
    const long long scan_len = R.scan_end - R.scan_start;
    if (R.nseg != (int)std::max<long long>(1, (scan_len + sb - 1) / sb)) return no("segment count");
    if (R.out_off < 0 || R.out_off + 3LL * R.H0 * R.W0 > H.out_bytes) return no("output range");
    JpegDecRow T = R;
    const size_t end = decode_jpeg_scratch_of(T, scratch_at);
    if (T.off_seg != R.off_seg || T.off_coef != R.off_coef || T.off_planes != R.off_planes || (long long)end > H.scratch_bytes) return no("scratch layout");
    scratch_at = end;
    for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 64; ++k)
            if (R.quant[c][k] < 1 || R.quant[c][k] > 255) return no("quantisation table");
    for (int t = 0; t < 6; ++t)
        for (int i = 0; i < 512; ++i)
            if ((R.huff[t].look[i] >> 8) > 9) return no("Huffman table");
    return true;
}

hipError_t launch_decode_jpeg(const uint8_t* files, const void* host_table, const void* dev_table, int n, int rgb, uint8_t* out, int* info,
                              void* scratch, hipStream_t st) {
    const JpegDecRow* rows = (const JpegDecRow*)((const uint8_t*)host_table + sizeof(JpegDecHeader));
    long long max_blk = 1, max_mcu = 1, max_px = 1;
    for (int f = 0; f < n; ++f) {
        max_blk = std::max<long long>(max_blk, rows[f].nblk);
        max_mcu = std::max<long long>(max_mcu, (long long)rows[f].mcu_rows * rows[f].mcu_cols);
        max_px = std::max<long long>(max_px, (long long)rows[f].H0 * rows[f].W0);
    }
    uint8_t* ws = (uint8_t*)scratch;
    const unsigned gz = (unsigned)std::min<long long>((max_blk * 8 + 255) / 256, 1024);
    hipLaunchKernelGGL(jpegd_zero_kernel, dim3(gz, n), dim3(256), 0, st, dev_table, ws);
    hipLaunchKernelGGL(jpegd_entropy_kernel, dim3(n), dim3(kEntropyThreads), 0, st, files, dev_table, ws, info);
    hipLaunchKernelGGL(jpegd_dc_kernel, dim3(3, n), dim3(256), 0, st, dev_table, ws);
    hipLaunchKernelGGL(jpegd_idct_kernel, dim3((unsigned)((max_mcu + 3) / 4), n), dim3(256), 0, st, dev_table, ws);
    const unsigned gc = (unsigned)std::min<long long>((max_px + 255) / 256, 4096);
    hipLaunchKernelGGL(jpegd_colour_kernel, dim3(gc, n), dim3(256), 0, st, dev_table, (const uint8_t*)ws, rgb, out);
    return hipGetLastError();
}

}  // namespace vti
