// vti_encode_jpeg: the saved JPEG (cv2.imwrite(save_path, annotated), main.py:314) on the device, byte for byte the package's
// jpeg.py (libjpeg's baseline file at a given quality: YCbCr 4:2:0, Annex K tables, jfdctint.c, one interleaved scan).
//
// Nine launches on one stream, no host synchronisation:
//   1 blocks     one wave per 16x16 MCU: colour conversion, 2x2 chroma average, integer FDCT, quantisation -> 6 x 64 zigzag int16
//                per MCU in scan order, the dummy blocks of a partial MCU materialised (zero AC, the DC of the block before)
//   2 lengths    one wave per block, lane i = zigzag coefficient i: the block's Huffman bit count
//   3 bit scan   per frame, the exclusive scan of the block bit counts (64-bit positions) and the frame's bit total
//   4 zero       the used words of the frame's unstuffed stream
//   5 bits       one wave per block: the same symbols again, written at the block's bit position (assembled in LDS, whole words
//                stored, the two words shared with the neighbours OR-ed in); the last block adds the 1-padding
//   6 count      0xFF bytes per 4096-byte chunk of the unstuffed stream
//   7 chunk scan per frame, the exclusive scan of those counts and the file size
//   8 offsets    the exclusive scan of the n file sizes -> dev_byte_offsets; the header bytes -> scratch
//   9 write      per chunk: header (chunk 0), the bytes with 0x00 after every 0xFF, EOI (last chunk); nothing when
//                dev_byte_offsets[n] > max_bytes
//
// vti_encode_jpeg_frames (frames of differing sizes, a frame table) runs the same nine kernels in their RAGGED instantiation behind
// one more launch (0 prefix): the exclusive scans of the frames' MCU counts and of their stream chunk counts, built from the device
// table into the scratch.  MCUs, blocks (6 per MCU) and chunks are numbered through the whole batch, so the scratch arrays are the
// uniform call's with every frame's part as long as that frame needs; a wave finds the frame of its MCU, block or chunk by binary
// search over the n + 1 prefix entries (it ends inside [0, n) whatever they hold) and takes H0, W0 and the frame's place from its row.
#include <cstring>

#include "vti_internal.h"

namespace vti {
namespace {

constexpr int kHeaderBytes = 623;
constexpr int kSofDims = 163;                 // SOI 2 + APP0 18 + DQT 2 x 69 + FF C0, length, precision: height and width, two bytes each
constexpr int kMaxBlockBits = 1658;          // DC 9 + 11; 63 AC coefficients of 16 + 10
constexpr int kChunkWords = 1024;            // the stuffing passes work on 4096-byte chunks of the unstuffed stream
constexpr int kScanThreads = 1024;

// Annex K.1 in zigzag order; K.3 as (bits, values)
constexpr uint8_t kZig[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                              28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                              54, 47, 55, 62, 63};
constexpr uint8_t kQBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr uint8_t kAcVals[2][162] = {
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

// symbol -> (length << 16) | code, by the canonical construction; tables dc0, ac0, dc1, ac1
struct HuffTabs { uint32_t t[4][256]; };
constexpr HuffTabs make_huff() {
    HuffTabs h = {};
    for (int tab = 0; tab < 4; ++tab) {
        const int chroma = tab >> 1, ac = tab & 1;
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            const int cnt = ac ? kAcBits[chroma][len - 1] : kDcBits[chroma][len - 1];
            for (int i = 0; i < cnt; ++i, ++k, ++code) h.t[tab][ac ? kAcVals[chroma][k] : k] = ((uint32_t)len << 16) | code;
            code <<= 1;
        }
    }
    return h;
}
constexpr HuffTabs kHuffHost = make_huff();
static_assert(kHuffHost.t[1][0xF0] == ((11u << 16) | 0x7F9) && kHuffHost.t[3][0xF0] == ((10u << 16) | 0x3FA) &&
              kHuffHost.t[1][0] == ((4u << 16) | 0xA) && kHuffHost.t[3][0] == (2u << 16), "Annex K codes");
__device__ const HuffTabs d_huff = make_huff();
struct ZigTab { uint8_t z[64]; };
constexpr ZigTab make_zig() {
    ZigTab t = {};
    for (int i = 0; i < 64; ++i) t.z[i] = kZig[i];
    return t;
}
__device__ const ZigTab d_zig = make_zig();
// the quantisation bases in ZIGZAG order
constexpr uint8_t zig_base(int c, int i) { return kQBase[c][kZig[i]]; }
struct QBaseZ { uint8_t q[2][64]; };
constexpr QBaseZ make_qbase() {
    QBaseZ z = {};
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) z.q[c][i] = zig_base(c, i);
    return z;
}
__device__ const QBaseZ d_qbase = make_qbase();

struct JpegHeader { uint8_t b[624]; };

constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }       // jccolor.c's FIX()
constexpr int kYR = fix16(.299), kYG = fix16(.587), kYB = fix16(.114), kCbR = fix16(.16874), kCbG = fix16(.33126), kHalf = fix16(.5),
              kCrG = fix16(.41869), kCrB = fix16(.08131);
__host__ __device__ inline int quant_of(int base, int scale) {
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

// One 1-D pass of jfdctint.c on d[0], d[s], .. d[7s]
template <bool FIRST>
__device__ inline void fdct_pass(int* d, int s) {
    const int a0 = d[0], a1 = d[s], a2 = d[2 * s], a3 = d[3 * s], a4 = d[4 * s], a5 = d[5 * s], a6 = d[6 * s], a7 = d[7 * s];
    const int t0 = a0 + a7, t7 = a0 - a7, t1 = a1 + a6, t6 = a1 - a6, t2 = a2 + a5, t5 = a2 - a5, t3 = a3 + a4, t4 = a3 - a4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15, r = 1 << (n - 1);
    if (FIRST) {
        d[0] = (t10 + t11) * 4;
        d[4 * s] = (t10 - t11) * 4;
    } else {
        d[0] = (t10 + t11 + 2) >> 2;
        d[4 * s] = (t10 - t11 + 2) >> 2;
    }
    int z1 = (t12 + t13) * 4433;
    d[2 * s] = (z1 + t13 * 6270 + r) >> n;
    d[6 * s] = (z1 - t12 * 15137 + r) >> n;
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d[7 * s] = (u4 + z1 + z3 + r) >> n;
    d[5 * s] = (u5 + z2 + z4 + r) >> n;
    d[3 * s] = (u6 + z2 + z3 + r) >> n;
    d[s] = (u7 + z1 + z4 + r) >> n;
}

// Where the frames are.  Uniform (rows == nullptr): n frames of H0 x W0 back to back, mr x mc MCUs and NC chunks each.  Ragged: frame k
// is row k of the device frame table; pm / pc [n + 1] are the exclusive scans of the frames' MCU and chunk counts (prefix kernel).
struct JpegGeo {
    const FrameRow* rows; const long long* pm; const long long* pc;
    int n, H0, W0, mr, mc;
    long long NC;
};

// the last k in [0, n) with pre[k] <= v (pre[0] = 0): always inside [0, n), whatever the array holds
__device__ inline int find_frame(const long long* __restrict__ pre, int n, long long v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (pre[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__host__ __device__ inline long long chunks_of_mcus(long long mcus) {      // the chunks that hold a frame's longest unstuffed stream
    const long long bytes = (mcus * 6 * kMaxBlockBits + 7) / 8;
    return (bytes + 4 * kChunkWords - 1) / (4 * kChunkWords);
}

// chunk `c` of the batch -> its frame and its index in that frame's stream
template <bool RAGGED>
__device__ inline void chunk_frame(const JpegGeo& g, long long c, long long& k, long long& t) {
    if (RAGGED) { k = find_frame(g.pc, g.n, c); t = c - g.pc[k]; }
    else { k = c / g.NC; t = c - k * g.NC; }
}

struct Ycc { int y, cb, cr; };
__device__ inline Ycc load_ycc(const uint8_t* f, int W0, int y, int x, int rgb) {
    const uint8_t* p = f + ((size_t)y * W0 + x) * 3;
    const int c0 = p[0], G = p[1], c2 = p[2];
    const int R = rgb ? c0 : c2, B = rgb ? c2 : c0;
    Ycc o;
    o.y = (kYR * R + kYG * G + kYB * B + 32768) >> 16;
    o.cb = (-kCbR * R - kCbG * G + kHalf * B + (128 << 16) + 32767) >> 16;
    o.cr = (kHalf * R - kCrG * G - kCrB * B + (128 << 16) + 32767) >> 16;
    return o;
}

// 1: one wave per MCU, four MCUs per workgroup.  Lane l owns the 2 x 2 cell (l >> 3, l & 7) of the MCU: four luma samples and one
// sample of each chroma plane.  The tile is 6 blocks of 8 rows pitched by 9 ints, so the row pass (lane = block * 8 + row, address
// 9 * lane + k) and the column pass (address 72 * block + column + 9 * k) both touch distinct banks.
template <bool RAGGED>
__global__ __launch_bounds__(256) void jpeg_blocks_kernel(const uint8_t* __restrict__ frames, long long n_mcu_all, JpegGeo g, int rgb,
                                                          int scale, int16_t* __restrict__ coef) {
    __shared__ int s_tile[4][6 * 72];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long m = (long long)blockIdx.x * 4 + wid;
    const bool live = m < n_mcu_all;
    if (!live) m = n_mcu_all - 1;                   // the wave still runs (workgroup barriers below); it stores nothing
    // the four MCUs of a workgroup can belong to different frames: the lookup is per wave (and every wave reaches every barrier)
    int H0 = g.H0, W0 = g.W0, mc = g.mc, r;
    const uint8_t* f;
    if (RAGGED) {
        const int k = find_frame(g.pm, g.n, m);
        const FrameRow& row = g.rows[k];
        H0 = row.H0; W0 = row.W0; mc = (W0 + 15) >> 4;
        r = (int)(m - g.pm[k]);
        f = frames + row.offset;
    } else {
        const int per = g.mr * mc;
        const long long k = m / per;
        r = (int)(m - k * per);
        f = frames + (size_t)k * H0 * W0 * 3;
    }
    const int my = r / mc, mx = r - my * mc;
    int* tile = s_tile[wid];
    const int cyl = lane >> 3, cxl = lane & 7;
    const int gy = my * 8 + cyl, gx = mx * 8 + cxl;                 // the cell = the chroma sample, in the chroma plane
    const int x0 = min(2 * gx, W0 - 1), x1 = min(2 * gx + 1, W0 - 1);
    const int bias = 1 + (cxl & 1);
    {
        const int y0 = min(2 * gy, H0 - 1), y1 = min(2 * gy + 1, H0 - 1);
        const Ycc a = load_ycc(f, W0, y0, x0, rgb), b = load_ycc(f, W0, y0, x1, rgb), c = load_ycc(f, W0, y1, x0, rgb),
                  d = load_ycc(f, W0, y1, x1, rgb);
        const int py = 2 * cyl, px = 2 * cxl;
        int* yb = tile + ((py >> 3) * 2 + (px >> 3)) * 72 + (py & 7) * 9 + (px & 7);
        yb[0] = a.y - 128;
        yb[1] = b.y - 128;
        yb[9] = c.y - 128;
        yb[10] = d.y - 128;
        int cb = (a.cb + b.cb + c.cb + d.cb + bias) >> 2, cr = (a.cr + b.cr + c.cr + d.cr + bias) >> 2;
        const int ch = (H0 + 1) >> 1;                                // chroma rows; the rows below repeat the last one
        if (gy >= ch) {
            const int yc0 = 2 * (ch - 1), yc1 = min(yc0 + 1, H0 - 1);
            const Ycc e = load_ycc(f, W0, yc0, x0, rgb), g = load_ycc(f, W0, yc0, x1, rgb), h = load_ycc(f, W0, yc1, x0, rgb),
                      i = load_ycc(f, W0, yc1, x1, rgb);
            cb = (e.cb + g.cb + h.cb + i.cb + bias) >> 2;
            cr = (e.cr + g.cr + h.cr + i.cr + bias) >> 2;
        }
        tile[4 * 72 + cyl * 9 + cxl] = cb - 128;
        tile[5 * 72 + cyl * 9 + cxl] = cr - 128;
    }
    __syncthreads();
    if (lane < 48) fdct_pass<true>(tile + 9 * lane, 1);
    __syncthreads();
    if (lane < 48) fdct_pass<false>(tile + (lane >> 3) * 72 + (lane & 7), 9);
    __syncthreads();
    const int nat = d_zig.z[lane], at = (nat >> 3) * 9 + (nat & 7);
    const int ybr = (H0 + 7) >> 3, ybc = (W0 + 7) >> 3;
    const bool dcol = 2 * mx + 1 >= ybc, drow = 2 * my + 1 >= ybr;
    int c[6];
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        const int v = tile[b * 72 + at];
        const unsigned q8 = 8u * (unsigned)quant_of(d_qbase.q[b >> 2][lane], scale);
        const unsigned a = (unsigned)(v < 0 ? -v : v);
        const int qv = (int)((a + (q8 >> 1)) / q8);
        c[b] = v < 0 ? -qv : qv;
    }
    // dummy blocks: zero AC, the DC of the block before it in the MCU
    const bool dummy1 = dcol, dummy2 = drow, dummy3 = drow || dcol;
    if (lane == 0) {
        if (dummy1) c[1] = c[0];
        if (dummy2) c[2] = c[1];
        if (dummy3) c[3] = c[2];
    } else {
        if (dummy1) c[1] = 0;
        if (dummy2) c[2] = 0;
        if (dummy3) c[3] = 0;
    }
    if (live) {
        int16_t* o = coef + (size_t)m * 384 + lane;
#pragma unroll
        for (int b = 0; b < 6; ++b) o[b * 64] = (int16_t)c[b];
    }
}

__device__ inline int wave_incl_scan(int x, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// value `v` of `len` <= 32 bits at bit position q (MSB first) of the wave's LDS words
__device__ inline void emit_bits(unsigned* buf, unsigned v, int len, int q) {
    if (len <= 0) return;
    const unsigned long long t = (unsigned long long)v << (64 - len - (q & 31));
    const unsigned hi = (unsigned)(t >> 32), lo = (unsigned)t;
    if (hi) atomicOr(&buf[q >> 5], hi);
    if (lo) atomicOr(&buf[(q >> 5) + 1], lo);
}

// 2 and 5: one wave per block of the scan, lane i = zigzag coefficient i.  WRITE = false: bitpos[block] = its bit count.
// WRITE = true: bitpos holds the exclusive scan; the block's bits go to the frame's stream (big-endian 32-bit words: bit p of the
// stream is bit 31 - p % 32 of word p / 32), which the zero kernel cleared.
template <bool WRITE, bool RAGGED>
__global__ __launch_bounds__(256) void jpeg_entropy_kernel(const int16_t* __restrict__ coef, long long n_blk_all, JpegGeo g,
                                                           unsigned long long* __restrict__ bitpos, unsigned* __restrict__ stream) {
    __shared__ unsigned s_buf[4][56];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    long long gb = (long long)blockIdx.x * 4 + wid;
    const bool live = gb < n_blk_all;
    if (!live) gb = n_blk_all - 1;
    long long k, j, nblk, first_word;                // the frame, the block's index in it, its blocks, its stream's first word
    if (RAGGED) {
        k = find_frame(g.pm, g.n, gb / 6);
        j = gb - 6 * g.pm[k]; nblk = 6 * (g.pm[k + 1] - g.pm[k]); first_word = g.pc[k] * kChunkWords;
    } else {
        nblk = (long long)g.mr * g.mc * 6;
        k = gb / nblk; j = gb - k * nblk; first_word = k * g.NC * kChunkWords;
    }
    const long long mcu = j / 6;
    const int b = (int)(j - mcu * 6), chroma = b >= 4;
    const int16_t* cf = coef + (size_t)gb * 64;
    int c = cf[lane];
    if (lane == 0) {        // the DC difference to the previous block of the same component (0 at the frame's first)
        int pred = 0;
        if (b >= 1 && b <= 3) pred = cf[-64];
        else if (mcu > 0) pred = cf[-(b == 0 ? 3 : 6) * 64];
        c -= pred;
    }
    const unsigned long long nzm = __ballot(lane > 0 && c != 0);                // nonzero AC positions
    const int last = nzm ? 63 - __builtin_clzll(nzm) : 0;                        // EOB follows it unless it is 63
    const unsigned* huff_ac = d_huff.t[2 * chroma + 1];
    const int mag = c < 0 ? -c : c;
    const int sz = mag ? 32 - __builtin_clz((unsigned)mag) : 0;
    unsigned main_v = 0;
    int main_len = 0, nzrl = 0;
    if (lane == 0 || c != 0) {
        int sym = sz;
        unsigned h;
        if (lane == 0) {
            h = d_huff.t[2 * chroma][sz & 15];
        } else {
            const unsigned long long before = (nzm | 1ull) & ((1ull << lane) - 1);
            const int run = lane - (63 - __builtin_clzll(before)) - 1;
            nzrl = run >> 4;
            sym = ((run & 15) << 4) | sz;
            h = huff_ac[sym & 255];
        }
        const unsigned extra = (unsigned)(c < 0 ? c - 1 : c) & ((1u << sz) - 1);
        main_v = ((h & 0xFFFF) << sz) | extra;
        main_len = (int)(h >> 16) + sz;
        if (lane == last && last < 63) {
            const unsigned e = huff_ac[0];
            main_v = (main_v << (e >> 16)) | (e & 0xFFFF);
            main_len += (int)(e >> 16);
        }
    }
    const unsigned zrl = huff_ac[0xF0];
    const int zlen = (int)(zrl >> 16);
    const int len = nzrl * zlen + main_len;
    const int incl = wave_incl_scan(len, lane);
    const int blk_bits = __shfl(incl, 63, 64);
    if (!WRITE) {
        if (live && lane == 0) bitpos[gb] = (unsigned long long)blk_bits;
        return;
    }
    unsigned* buf = s_buf[wid];
    if (lane < 56) buf[lane] = 0;
    __syncthreads();
    const unsigned long long P = bitpos[gb];
    const int q0 = (int)(P & 31);
    int q = q0 + incl - len;
    for (int z = 0; z < nzrl; ++z, q += zlen) emit_bits(buf, zrl & 0xFFFF, zlen, q);
    emit_bits(buf, main_v, main_len, q);
    int end = q0 + blk_bits;
    if (j == nblk - 1) {                            // the frame's last block pads the last byte with 1-bits
        const int pad = (int)((0 - (P + (unsigned long long)blk_bits)) & 7);
        if (lane == 0) emit_bits(buf, (1u << pad) - 1, pad, end);
        end += pad;
    }
    __syncthreads();
    const int nwords = (end + 31) >> 5;
    if (live && lane < nwords) {
        const unsigned v = buf[lane];
        unsigned* dst = stream + (size_t)first_word + (size_t)(P >> 5) + lane;
        if (lane == 0 || lane == nwords - 1) {      // shared with the neighbouring blocks
            if (v) atomicOr(dst, v);
        } else {
            *dst = v;
        }
    }
}

// A workgroup-wide exclusive scan of one value per thread; returns the prefix and the total (s_w: kScanThreads / 64 entries).
__device__ inline unsigned long long block_excl_scan(unsigned long long v, unsigned long long* s_w, unsigned long long& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned long long x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wid] = x;
    __syncthreads();
    unsigned long long pre = 0, tot = 0;
    for (int w = 0; w < kScanThreads / 64; ++w) {
        const unsigned long long t = s_w[w];
        if (w < wid) pre += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

// 0 (ragged only): one workgroup: pm, pc [0 .. n] = the exclusive scans of the frames' MCU and chunk counts, from the device table
__global__ __launch_bounds__(kScanThreads) void jpeg_prefix_kernel(const FrameRow* __restrict__ rows, int n, long long* pm, long long* pc) {
    __shared__ unsigned long long s_w[kScanThreads / 64];
    unsigned long long cm = 0, cc = 0;
    for (int b0 = 0; b0 < n; b0 += kScanThreads) {
        const int i = b0 + threadIdx.x;
        unsigned long long mcus = 0, chunks = 0;
        if (i < n) {
            mcus = (unsigned long long)((rows[i].H0 + 15) >> 4) * (unsigned long long)((rows[i].W0 + 15) >> 4);
            chunks = (unsigned long long)chunks_of_mcus((long long)mcus);
        }
        unsigned long long tm, tc;
        const unsigned long long em = block_excl_scan(mcus, s_w, tm), ec = block_excl_scan(chunks, s_w, tc);
        if (i < n) { pm[i] = (long long)(cm + em); pc[i] = (long long)(cc + ec); }
        cm += tm; cc += tc;
    }
    if (threadIdx.x == 0) { pm[n] = (long long)cm; pc[n] = (long long)cc; }
}

// 3: frame blockIdx.x: bitpos[frame] -> its exclusive scan, fbits[frame] = the total
template <bool RAGGED>
__global__ __launch_bounds__(kScanThreads) void jpeg_bit_scan_kernel(unsigned long long* bitpos, JpegGeo g, unsigned long long* fbits) {
    __shared__ unsigned long long s_w[kScanThreads / 64];
    const long long nblk = RAGGED ? 6 * (g.pm[blockIdx.x + 1] - g.pm[blockIdx.x]) : (long long)g.mr * g.mc * 6;
    unsigned long long* p = bitpos + (RAGGED ? (size_t)(6 * g.pm[blockIdx.x]) : (size_t)blockIdx.x * nblk);
    unsigned long long carry = 0;
    for (long long b0 = 0; b0 < nblk; b0 += kScanThreads) {
        const long long i = b0 + threadIdx.x;
        const unsigned long long v = i < nblk ? p[i] : 0;
        unsigned long long tot;
        const unsigned long long ex = block_excl_scan(v, s_w, tot);
        if (i < nblk) p[i] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) fbits[blockIdx.x] = carry;
}

__device__ inline unsigned long long used_bytes(const unsigned long long* fbits, long long k) { return (fbits[k] + 7) >> 3; }

// 4: workgroup (frame, chunk): zero the chunk's words that the frame's stream uses
template <bool RAGGED>
__global__ __launch_bounds__(256) void jpeg_zero_kernel(unsigned* stream, const unsigned long long* fbits, JpegGeo g) {
    long long k, t;
    chunk_frame<RAGGED>(g, blockIdx.x, k, t);
    const unsigned long long words = (used_bytes(fbits, k) + 3) >> 2;
    unsigned* s = stream + (size_t)blockIdx.x * kChunkWords;
    for (int i = threadIdx.x; i < kChunkWords; i += 256)
        if ((unsigned long long)t * kChunkWords + i < words) s[i] = 0;
}

__device__ inline int ff_count(unsigned w) {
    return ((w >> 24) == 0xFF) + (((w >> 16) & 0xFF) == 0xFF) + (((w >> 8) & 0xFF) == 0xFF) + ((w & 0xFF) == 0xFF);
}

// 6: one wave per (frame, chunk): 0xFF bytes of the chunk (the unused bytes of the last word are zero)
template <bool RAGGED>
__global__ __launch_bounds__(64) void jpeg_count_kernel(const unsigned* __restrict__ stream, const unsigned long long* __restrict__ fbits,
                                                        JpegGeo g, unsigned* __restrict__ chunk_ff) {
    long long k, t;
    chunk_frame<RAGGED>(g, blockIdx.x, k, t);
    const unsigned long long words = (used_bytes(fbits, k) + 3) >> 2;
    if ((unsigned long long)t * kChunkWords >= words) return;
    const unsigned* s = stream + (size_t)blockIdx.x * kChunkWords;
    int cnt = 0;
    for (int i = threadIdx.x; i < kChunkWords; i += 64)
        if ((unsigned long long)t * kChunkWords + i < words) cnt += ff_count(s[i]);
#pragma unroll
    for (int o = 32; o; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (threadIdx.x == 0) chunk_ff[blockIdx.x] = (unsigned)cnt;
}

// 7: frame blockIdx.x: the exclusive scan of its used chunks' counts, fsize[frame] = header + bytes + stuffing + EOI
template <bool RAGGED>
__global__ __launch_bounds__(kScanThreads) void jpeg_chunk_scan_kernel(unsigned* chunk_ff, const unsigned long long* fbits, JpegGeo g,
                                                                       long long* fsize) {
    __shared__ unsigned long long s_w[kScanThreads / 64];
    const unsigned long long bytes = used_bytes(fbits, blockIdx.x);
    const long long used = (long long)((bytes + 4 * kChunkWords - 1) / (4 * kChunkWords));
    unsigned* p = chunk_ff + (RAGGED ? (size_t)g.pc[blockIdx.x] : (size_t)blockIdx.x * g.NC);
    unsigned long long carry = 0;
    for (long long b0 = 0; b0 < used; b0 += kScanThreads) {
        const long long i = b0 + threadIdx.x;
        const unsigned long long v = i < used ? p[i] : 0;
        unsigned long long tot;
        const unsigned long long ex = block_excl_scan(v, s_w, tot);
        if (i < used) p[i] = (unsigned)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0) fsize[blockIdx.x] = (long long)(kHeaderBytes + bytes + carry + 2);
}

// 8: one workgroup: offsets[0 .. n] = the exclusive scan of fsize; the header -> scratch for the write kernel
__global__ __launch_bounds__(kScanThreads) void jpeg_offsets_kernel(const long long* fsize, long long n, long long* offsets, JpegHeader hdr,
                                                                    uint8_t* dev_hdr) {
    __shared__ unsigned long long s_w[kScanThreads / 64];
    if (threadIdx.x < 624) dev_hdr[threadIdx.x] = hdr.b[threadIdx.x];
    unsigned long long carry = 0;
    for (long long b0 = 0; b0 < n; b0 += kScanThreads) {
        const long long i = b0 + threadIdx.x;
        const unsigned long long v = i < n ? (unsigned long long)fsize[i] : 0;
        unsigned long long tot;
        const unsigned long long ex = block_excl_scan(v, s_w, tot);
        if (i < n) offsets[i] = (long long)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0) offsets[n] = (long long)carry;
}

// 9: one wave per (frame, chunk): the chunk's bytes with 0x00 after every 0xFF at their place in the file; chunk 0 also writes the
// header, the last used chunk the EOI marker.  Nothing when the n files do not fit in max_bytes.
template <bool RAGGED>
__global__ __launch_bounds__(64) void jpeg_write_kernel(const unsigned* __restrict__ stream, const unsigned long long* __restrict__ fbits,
                                                        JpegGeo g, const unsigned* __restrict__ chunk_ff,
                                                        const long long* __restrict__ offsets, long long n, long long max_bytes,
                                                        const uint8_t* __restrict__ dev_hdr, uint8_t* __restrict__ out) {
    if (offsets[n] > max_bytes) return;
    long long k, t;
    chunk_frame<RAGGED>(g, blockIdx.x, k, t);
    const unsigned long long bytes = used_bytes(fbits, k);
    const unsigned long long start = (unsigned long long)t * (4 * kChunkWords);
    if (start >= bytes) return;
    const int lane = threadIdx.x;
    uint8_t* file = out + offsets[k];
    if (t == 0) {
        if (RAGGED) {                               // the header in the scratch is the batch's; SOF0 carries this file's height and width
            const int H0 = g.rows[k].H0, W0 = g.rows[k].W0;
            for (int i = lane; i < kHeaderBytes; i += 64) {
                const int d = i - kSofDims;
                file[i] = d == 0 ? (uint8_t)(H0 >> 8) : d == 1 ? (uint8_t)H0 : d == 2 ? (uint8_t)(W0 >> 8) : d == 3 ? (uint8_t)W0 : dev_hdr[i];
            }
        } else {
            for (int i = lane; i < kHeaderBytes; i += 64) file[i] = dev_hdr[i];
        }
    }
    uint8_t* o = file + kHeaderBytes + start + chunk_ff[blockIdx.x];
    const unsigned* s = stream + (size_t)blockIdx.x * kChunkWords;
    const unsigned long long left = bytes - start;                      // bytes of the stream from this chunk's start on
    long long run = 0;
    for (int i0 = 0; i0 < kChunkWords && (unsigned long long)i0 * 4 < left; i0 += 64) {
        const unsigned long long at = (unsigned long long)(i0 + lane) * 4;
        const int nv = at >= left ? 0 : left - at >= 4 ? 4 : (int)(left - at);
        const unsigned w = nv ? s[i0 + lane] : 0;
        int cnt = 0;
        for (int j = 0; j < nv; ++j) cnt += ((w >> (24 - 8 * j)) & 0xFF) == 0xFF;
        const int len = nv + cnt;
        const int incl = wave_incl_scan(len, lane);
        uint8_t* p = o + run + (incl - len);
        for (int j = 0; j < nv; ++j) {
            const uint8_t v = (uint8_t)(w >> (24 - 8 * j));
            *p++ = v;
            if (v == 0xFF) *p++ = 0;
        }
        run += __shfl(incl, 63, 64);
    }
    if (start + 4 * kChunkWords >= bytes && lane == 0) {
        o[run] = 0xFF;
        o[run + 1] = 0xD9;
    }
}

}  // namespace

bool encode_jpeg_layout(long long n, int H0, int W0, JpegLayout& L) {
    if (n < 1 || H0 < 1 || W0 < 1 || H0 > 8192 || W0 > 8192) return false;
    L.mr = (H0 + 15) / 16;
    L.mc = (W0 + 15) / 16;
    if (n * L.mr * L.mc > (1LL << 28)) return false;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.nblk = (long long)L.mr * L.mc * 6;
    L.stream_bytes = (L.nblk * kMaxBlockBits + 7) / 8;                  // the most bytes a frame's unstuffed stream can have
    L.NC = (L.stream_bytes + 4 * kChunkWords - 1) / (4 * kChunkWords);
    L.off_fbits = 1024;                                                 // the header's 624 bytes come first
    L.off_fsize = L.off_fbits + al((size_t)n * 8);
    L.off_coef = L.off_fsize + al((size_t)n * 8);
    L.off_bitpos = L.off_coef + al((size_t)n * L.nblk * 128);
    L.off_stream = L.off_bitpos + al((size_t)n * L.nblk * 8);
    L.off_chunk = L.off_stream + al((size_t)n * L.NC * kChunkWords * 4);
    L.total = L.off_chunk + al((size_t)n * L.NC * 4);
    L.max_file = kHeaderBytes + 2 + 2 * L.stream_bytes;                 // every byte stuffed
    return true;
}

void encode_jpeg_header(int H0, int W0, int quality, uint8_t out[624]) {
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    uint8_t* p = out;
    auto put = [&](std::initializer_list<int> v) { for (int x : v) *p++ = (uint8_t)x; };
    put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0, 67, c});
        for (int i = 0; i < 64; ++i) *p++ = (uint8_t)quant_of(kQBase[c][kZig[i]], scale);
    }
    put({0xFF, 0xC0, 0, 17, 8, H0 >> 8, H0 & 255, W0 >> 8, W0 & 255, 3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int tab = 0; tab < 4; ++tab) {
        const int chroma = tab >> 1, ac = tab & 1, nvals = ac ? 162 : 12;
        put({0xFF, 0xC4, 0, 3 + 16 + nvals, (ac << 4) | chroma});
        for (int i = 0; i < 16; ++i) *p++ = ac ? kAcBits[chroma][i] : kDcBits[chroma][i];
        for (int i = 0; i < nvals; ++i) *p++ = ac ? kAcVals[chroma][i] : (uint8_t)i;
    }
    put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0});
    *p++ = 0;                                                           // 623 bytes and one of padding
}

bool encode_jpeg_frames_layout(const void* host_table, JpegFramesLayout& L) {
    FrameTableHeader h;
    memcpy(&h, host_table, sizeof h);
    if (h.magic != kFrameTableMagic || h.B < 1) return false;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    L.n = h.B; L.n_mcu = 0; L.n_chunk = 0; L.max_bytes = 0;
    for (int k = 0; k < h.B; ++k) {
        FrameRow r;
        memcpy(&r, (const char*)host_table + sizeof h + (size_t)k * sizeof r, sizeof r);
        JpegLayout one;
        if (!encode_jpeg_layout(1, r.H0, r.W0, one)) return false;
        L.n_mcu += (long long)one.mr * one.mc;
        L.n_chunk += chunks_of_mcus((long long)one.mr * one.mc);
        L.max_bytes += one.max_file;
    }
    if (L.n_mcu > (1LL << 28)) return false;
    const size_t n = (size_t)h.B;
    L.off_pm = 1024;                                                    // the header's 624 bytes come first
    L.off_pc = L.off_pm + al((n + 1) * 8);
    L.off_fbits = L.off_pc + al((n + 1) * 8);
    L.off_fsize = L.off_fbits + al(n * 8);
    L.off_coef = L.off_fsize + al(n * 8);
    L.off_bitpos = L.off_coef + al((size_t)L.n_mcu * 6 * 128);
    L.off_stream = L.off_bitpos + al((size_t)L.n_mcu * 6 * 8);
    L.off_chunk = L.off_stream + al((size_t)L.n_chunk * kChunkWords * 4);
    L.total = L.off_chunk + al((size_t)L.n_chunk * 4);
    return true;
}

namespace {

// the nine launches behind either entry point; g.rows selects the instantiation
template <bool RAGGED>
hipError_t encode_launches(const uint8_t* frames, const JpegGeo& g, long long n_mcu, long long n_chunk, int rgb, int quality, uint8_t* ws,
                           unsigned long long* fbits, long long* fsize, int16_t* coef, unsigned long long* bitpos, unsigned* stream,
                           unsigned* chunk_ff, long long* offsets, uint8_t* out, long long max_bytes, hipStream_t st) {
    const long long n_blk = n_mcu * 6;
    const int n = g.n, scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    JpegHeader hdr;
    encode_jpeg_header(g.H0, g.W0, quality, hdr.b);
    const dim3 chunks((unsigned)n_chunk);
    hipLaunchKernelGGL(jpeg_blocks_kernel<RAGGED>, dim3((unsigned)((n_mcu + 3) / 4)), dim3(256), 0, st, frames, n_mcu, g, rgb, scale, coef);
    hipLaunchKernelGGL((jpeg_entropy_kernel<false, RAGGED>), dim3((unsigned)((n_blk + 3) / 4)), dim3(256), 0, st, (const int16_t*)coef,
                       n_blk, g, bitpos, stream);
    hipLaunchKernelGGL(jpeg_bit_scan_kernel<RAGGED>, dim3(n), dim3(kScanThreads), 0, st, bitpos, g, fbits);
    hipLaunchKernelGGL(jpeg_zero_kernel<RAGGED>, chunks, dim3(256), 0, st, stream, (const unsigned long long*)fbits, g);
    hipLaunchKernelGGL((jpeg_entropy_kernel<true, RAGGED>), dim3((unsigned)((n_blk + 3) / 4)), dim3(256), 0, st, (const int16_t*)coef,
                       n_blk, g, bitpos, stream);
    hipLaunchKernelGGL(jpeg_count_kernel<RAGGED>, chunks, dim3(64), 0, st, (const unsigned*)stream, (const unsigned long long*)fbits, g,
                       chunk_ff);
    hipLaunchKernelGGL(jpeg_chunk_scan_kernel<RAGGED>, dim3(n), dim3(kScanThreads), 0, st, chunk_ff, (const unsigned long long*)fbits, g,
                       fsize);
    hipLaunchKernelGGL(jpeg_offsets_kernel, dim3(1), dim3(kScanThreads), 0, st, (const long long*)fsize, (long long)n, offsets, hdr, ws);
    hipLaunchKernelGGL(jpeg_write_kernel<RAGGED>, chunks, dim3(64), 0, st, (const unsigned*)stream, (const unsigned long long*)fbits, g,
                       (const unsigned*)chunk_ff, (const long long*)offsets, (long long)n, max_bytes, (const uint8_t*)ws, out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_encode_jpeg(const uint8_t* frames, int n, int H0, int W0, int rgb, int quality, void* scratch, long long* offsets,
                              uint8_t* out, long long max_bytes, hipStream_t st) {
    JpegLayout L;
    if (!encode_jpeg_layout(n, H0, W0, L)) return hipErrorInvalidValue;
    uint8_t* ws = (uint8_t*)scratch;
    const JpegGeo g{nullptr, nullptr, nullptr, n, H0, W0, L.mr, L.mc, L.NC};
    return encode_launches<false>(frames, g, (long long)n * L.mr * L.mc, (long long)n * L.NC, rgb, quality, ws,
                                  (unsigned long long*)(ws + L.off_fbits), (long long*)(ws + L.off_fsize), (int16_t*)(ws + L.off_coef),
                                  (unsigned long long*)(ws + L.off_bitpos), (unsigned*)(ws + L.off_stream), (unsigned*)(ws + L.off_chunk),
                                  offsets, out, max_bytes, st);
}

hipError_t launch_encode_jpeg_frames(const uint8_t* frames, const void* host_table, const FrameRow* rows, int rgb, int quality,
                                     void* scratch, long long* offsets, uint8_t* out, long long max_bytes, hipStream_t st) {
    JpegFramesLayout L;
    if (!encode_jpeg_frames_layout(host_table, L)) return hipErrorInvalidValue;
    uint8_t* ws = (uint8_t*)scratch;
    long long* pm = (long long*)(ws + L.off_pm);
    long long* pc = (long long*)(ws + L.off_pc);
    hipLaunchKernelGGL(jpeg_prefix_kernel, dim3(1), dim3(kScanThreads), 0, st, rows, L.n, pm, pc);
    // H0, W0 of the header in the scratch are placeholders: the write kernel patches every file's own
    const JpegGeo g{rows, pm, pc, L.n, 1, 1, 0, 0, 0};
    return encode_launches<true>(frames, g, L.n_mcu, L.n_chunk, rgb, quality, ws, (unsigned long long*)(ws + L.off_fbits),
                                 (long long*)(ws + L.off_fsize), (int16_t*)(ws + L.off_coef), (unsigned long long*)(ws + L.off_bitpos),
                                 (unsigned*)(ws + L.off_stream), (unsigned*)(ws + L.off_chunk), offsets, out, max_bytes, st);
}

}  // namespace vti
