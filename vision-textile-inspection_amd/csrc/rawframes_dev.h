// vti_convert_raw's arithmetic and per-lane work as plain C++ for host and device: the raw-table rows, the pixel rule of the
// package's rawframes.py (OpenCV's BT.601 limited-range 20-bit fixed point, chroma replicated) and the work item one lane does.
// csrc/rawframes.hip builds its kernel from these; tests/rawframes_host_cover.cpp compiles them for the host and runs the items
// one by one on exact-size buffers, so both the vector and the byte path are held to rawframes.to_bgr without a GPU.
#pragma once
#include <stdint.h>

#ifndef VTI_HD
#define VTI_HD __host__ __device__
#endif

namespace vti {

enum { kRawYUYV = 0, kRawUYVY = 1, kRawNV12 = 2, kRawNV21 = 3, kRawI420 = 4, kRawYV12 = 5, kRawFormats = 6 };
constexpr int kRawMaxSide = 8192;
constexpr int kRawMaxFrames = 4096;
constexpr int kRawTableMagic = 0x31574156;      // "VAW1"

struct RawRow {
    long long raw_off;          // of the frame's first byte in the raw buffer (a multiple of 16)
    long long raw_len;          // raw_frame_bytes(fmt, H0, W0)
    int H0, W0, fmt, pad;
};
static_assert(sizeof(RawRow) == 32, "raw table rows are 32 bytes");
struct RawTableHeader {
    int magic, n;
    long long raw_bytes;        // of the raw buffer the offsets were laid out in (out_raw_offsets[n])
    int pad[12];
};
static_assert(sizeof(RawTableHeader) == 64, "the rows of a raw table stay 32-byte aligned");

namespace raw {

VTI_HD inline bool fmt_420(int fmt) { return fmt >= kRawNV12; }

// bytes of one frame; 0 for a size or format the conversion does not take
VTI_HD inline long long frame_bytes(int fmt, int H0, int W0) {
    if (fmt < 0 || fmt >= kRawFormats || H0 < 2 || W0 < 2 || H0 > kRawMaxSide || W0 > kRawMaxSide || (W0 & 1)) return 0;
    if (fmt_420(fmt) && (H0 & 1)) return 0;
    return fmt_420(fmt) ? (long long)H0 * W0 * 3 / 2 : 2LL * H0 * W0;
}

// Work items of one frame.  4:2:2: the frame is one run of H0*W0/2 four-byte pixel pairs (W0 is even, so no pair straddles a
// row); an item is 4 pairs = 16 raw bytes = 8 pixels = 24 output bytes.  4:2:0: an item is 16 columns of two rows that share
// their chroma row: 2 x 16 luma bytes, 16 chroma bytes, 2 x 48 output bytes.
constexpr int kPairsPerItem = 4;
constexpr int kColsPerItem = 16;
VTI_HD inline int items_of(int fmt, int H0, int W0) {
    return fmt_420(fmt) ? (H0 / 2) * ((W0 + kColsPerItem - 1) / kColsPerItem) : (H0 * W0 / 2 + kPairsPerItem - 1) / kPairsPerItem;
}

constexpr int CY = 1220542, CUB = 2116026, CUG = -409993, CVG = -852492, CVR = 1673527, SHIFT = 20;

struct Chroma { int ruv, guv, buv; };
VTI_HD inline Chroma chroma_of(int U, int V) {
    const int u = U - 128, v = V - 128;
    return {(1 << (SHIFT - 1)) + CVR * v, (1 << (SHIFT - 1)) + CVG * v + CUG * u, (1 << (SHIFT - 1)) + CUB * u};
}
VTI_HD inline unsigned clamp8(int v) { return (unsigned)(v < 0 ? 0 : v > 255 ? 255 : v); }
// one pixel as a 24-bit value: first byte in bits 0..7 (B, or R with rgb)
VTI_HD inline unsigned pixel(int Y, const Chroma& c, int rgb) {
    const int y = (Y > 16 ? Y - 16 : 0) * CY;       // at most 239 * CY + 2^19 + CVR * 127 < 2^31
    const unsigned r = clamp8((y + c.ruv) >> SHIFT), g = clamp8((y + c.guv) >> SHIFT), b = clamp8((y + c.buv) >> SHIFT);
    return rgb ? (r | g << 8 | b << 16) : (b | g << 8 | r << 16);
}
// four 24-bit pixels -> three little-endian words
VTI_HD inline void pack4(unsigned p0, unsigned p1, unsigned p2, unsigned p3, unsigned* w) {
    w[0] = p0 | p1 << 24;
    w[1] = p1 >> 8 | p2 << 16;
    w[2] = p2 >> 16 | p3 << 8;
}

struct alignas(16) V16 { unsigned w[4]; };
struct alignas(8) V8 { unsigned w[2]; };

// NW words from p, of which the first `valid` bytes exist.  All bytes there and p a multiple of VEC: loads of VEC bytes; else byte
// loads of exactly the valid bytes (the rest of the words is 0).
template <int NW, int VEC>
VTI_HD inline void load_words(const uint8_t* p, int valid, unsigned* w) {
    if (valid == 4 * NW && ((uintptr_t)p & (VEC - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 4 * NW / VEC; ++k) {
            if (VEC == 16) {
                const V16 v = *(const V16*)(p + 16 * k);
                w[4 * k] = v.w[0]; w[4 * k + 1] = v.w[1]; w[4 * k + 2] = v.w[2]; w[4 * k + 3] = v.w[3];
            } else {
                const V8 v = *(const V8*)(p + 8 * k);
                w[2 * k] = v.w[0]; w[2 * k + 1] = v.w[1];
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < NW; ++k) w[k] = 0;
#pragma unroll
    for (int k = 0; k < 4 * NW; ++k)
        if (k < valid) w[k >> 2] |= (unsigned)p[k] << (8 * (k & 3));
}
// the first `valid` bytes of NW words to p, and no other byte
template <int NW, int VEC>
VTI_HD inline void store_words(uint8_t* p, int valid, const unsigned* w) {
    if (valid == 4 * NW && ((uintptr_t)p & (VEC - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < 4 * NW / VEC; ++k) {
            if (VEC == 16) {
                V16 v;
                v.w[0] = w[4 * k]; v.w[1] = w[4 * k + 1]; v.w[2] = w[4 * k + 2]; v.w[3] = w[4 * k + 3];
                *(V16*)(p + 16 * k) = v;
            } else {
                V8 v;
                v.w[0] = w[2 * k]; v.w[1] = w[2 * k + 1];
                *(V8*)(p + 8 * k) = v;
            }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4 * NW; ++k)
        if (k < valid) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
}
VTI_HD inline unsigned byte_of(const unsigned* w, int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// One frame as the kernel sees it: raw and out are the frame's first bytes (any byte address).
struct Frame {
    const uint8_t* raw;
    uint8_t* out;
    int H0, W0, fmt;
};

// item `i` of a 4:2:2 frame (0 <= i < items_of): pairs 4i .. 4i+3 of the run, the last item possibly fewer
VTI_HD inline void item_422(const Frame& F, int rgb, int i) {
    const int pairs = F.H0 * F.W0 / 2, p0 = i * kPairsPerItem;
    const int np = pairs - p0 < kPairsPerItem ? pairs - p0 : kPairsPerItem;
    unsigned q[4], px[8], o[6];
    load_words<4, 16>(F.raw + 4LL * p0, 4 * np, q);
    const int uyvy = F.fmt == kRawUYVY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const unsigned w = q[j], b0 = w & 255, b1 = (w >> 8) & 255, b2 = (w >> 16) & 255, b3 = w >> 24;
        const int y0 = (int)(uyvy ? b1 : b0), y1 = (int)(uyvy ? b3 : b2);      // YUYV: Y0 U Y1 V; UYVY: U Y0 V Y1
        const Chroma c = chroma_of((int)(uyvy ? b0 : b1), (int)(uyvy ? b2 : b3));
        px[2 * j] = pixel(y0, c, rgb);
        px[2 * j + 1] = pixel(y1, c, rgb);
    }
    pack4(px[0], px[1], px[2], px[3], o);
    pack4(px[4], px[5], px[6], px[7], o + 3);
    store_words<6, 8>(F.out + 6LL * p0, 6 * np, o);
}

// item `i` of a 4:2:0 frame: row pair i / cpr, columns 16 * (i % cpr) .. +15 (fewer at the right edge; W0 is even)
VTI_HD inline void item_420(const Frame& F, int rgb, int i) {
    const int H0 = F.H0, W0 = F.W0, cpr = (W0 + kColsPerItem - 1) / kColsPerItem;
    const int rp = i / cpr, x0 = (i - rp * cpr) * kColsPerItem;
    const int nc = W0 - x0 < kColsPerItem ? W0 - x0 : kColsPerItem;
    const uint8_t* y0p = F.raw + (long long)(2 * rp) * W0 + x0;
    const uint8_t* cbase = F.raw + (long long)H0 * W0;
    unsigned ya[4], yb[4], cu[2], cv[2];
    load_words<4, 16>(y0p, nc, ya);
    load_words<4, 16>(y0p + W0, nc, yb);
    if (F.fmt == kRawNV12 || F.fmt == kRawNV21) {
        unsigned c[4];
        load_words<4, 16>(cbase + (long long)rp * W0 + x0, nc, c);
        cu[0] = cu[1] = cv[0] = cv[1] = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const unsigned a = byte_of(c, 2 * j), b = byte_of(c, 2 * j + 1);
            cu[j >> 2] |= (F.fmt == kRawNV12 ? a : b) << (8 * (j & 3));
            cv[j >> 2] |= (F.fmt == kRawNV12 ? b : a) << (8 * (j & 3));
        }
    } else {
        const long long plane = (long long)(H0 / 2) * (W0 / 2), at = (long long)rp * (W0 / 2) + x0 / 2;
        load_words<2, 8>(cbase + (F.fmt == kRawI420 ? 0 : plane) + at, nc / 2, cu);
        load_words<2, 8>(cbase + (F.fmt == kRawI420 ? plane : 0) + at, nc / 2, cv);
    }
    unsigned pa[16], pb[16], oa[12], ob[12];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const Chroma c = chroma_of((int)byte_of(cu, j), (int)byte_of(cv, j));
        pa[2 * j] = pixel((int)byte_of(ya, 2 * j), c, rgb);
        pa[2 * j + 1] = pixel((int)byte_of(ya, 2 * j + 1), c, rgb);
        pb[2 * j] = pixel((int)byte_of(yb, 2 * j), c, rgb);
        pb[2 * j + 1] = pixel((int)byte_of(yb, 2 * j + 1), c, rgb);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        pack4(pa[4 * k], pa[4 * k + 1], pa[4 * k + 2], pa[4 * k + 3], oa + 3 * k);
        pack4(pb[4 * k], pb[4 * k + 1], pb[4 * k + 2], pb[4 * k + 3], ob + 3 * k);
    }
    uint8_t* o0 = F.out + 3 * ((long long)(2 * rp) * W0 + x0);
    store_words<12, 16>(o0, 3 * nc, oa);
    store_words<12, 16>(o0 + 3LL * W0, 3 * nc, ob);
}

VTI_HD inline void item(const Frame& F, int rgb, int i) {
    if (fmt_420(F.fmt)) item_420(F, rgb, i);
    else item_422(F, rgb, i);
}

}  // namespace raw
}  // namespace vti
