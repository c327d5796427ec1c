// Device functions of the contour tracer (polygons.hip: vti_mask_polygons) that vti_annotate (annotate.hip) traces the fabric outline
// with: the union-find over the runs of a zero-padded 64-bit-word image, the 8-neighbourhood windows and the outer-border
// following with streamed CHAIN_APPROX_SIMPLE (polygons.py's _trace_outer + _approx_simple).  Included by both translation units.
#pragma once
#include "vti_internal.h"

namespace vti {
namespace poly {

constexpr int kThreads = 256;
constexpr int kLdsBytes = 156 * 1024;               // dynamic LDS when the image fits (a whole 960 x 1280 mask is 153600 bytes):
                                                    // the image, then parent[] when the slot's runs fit in the rest
typedef unsigned long long u64;

constexpr int kFormLds = 1, kFormScratch = 2;       // PolyLayout::forms: where the images of a call's slots are kept

// The labelling area of one H x W mask: parent | runs | row_start | the image when it does not fit the LDS (each part a multiple
// of 256 bytes).  Host: the sizes the scratch is made of; device: whether a slot of a frame table fits the areas of its call.
__host__ __device__ inline void poly_parts(int H, int W, PolyLayout& L) {
    const size_t r_max = (size_t)H * (size_t)((W + 1) / 2);     // at most ceil(W/2) runs per row
    L.WW = (W + 63) / 64;
    L.img_bytes = (size_t)H * L.WW * 8;
    L.in_lds = L.img_bytes <= (size_t)kLdsBytes;
    L.forms = L.in_lds ? kFormLds : kFormScratch;
    L.off_runs = (r_max * 4 + 255) & ~(size_t)255;
    L.off_rows = 2 * L.off_runs;
    L.off_img = L.off_rows + (((size_t)(H + 1) * 4 + 255) & ~(size_t)255);
    L.area_bytes = L.off_img + (L.in_lds ? 0 : (L.img_bytes + 255) & ~(size_t)255);
}

// scale_coords((H, W), pts, (H0, W0)) as polygons.py computes it: gain and pads in double (Python floats), each rounded to f32 once;
// the vertices then take (c - pad) / gain in f32 with a correctly rounded division and the clip to the frame.  The same IEEE
// double operations on the host (vti_mask_polygons: one geometry per call) and on the device (vti_mask_polygons_frames: the slot's
// frame, from its row of the table); the build keeps floating-point contraction off.
struct PolyMap { float padx, pady, gain, W0, H0; };
__host__ __device__ inline PolyMap poly_map(int H, int W, int H0, int W0) {
    const double gy = (double)H / (double)H0, gx = (double)W / (double)W0, gain = gx < gy ? gx : gy;
    const double padx = ((double)W - (double)W0 * gain) / 2, pady = ((double)H - (double)H0 * gain) / 2;
    return PolyMap{(float)padx, (float)pady, (float)gain, (float)W0, (float)H0};
}

// parent[] lives in LDS or in the workgroup's own part of the scratch; every access is atomic (agent scope: past the CU's vector
// cache when it is global memory)
__device__ __forceinline__ int ld_p(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_p(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x, halving the path on the way (a non-root's parent only ever moves to another ancestor, so the halving is safe
// against concurrent links, which change roots only)
__device__ int uf_find(int* parent, int x, int bound, bool& bad) {
    for (int it = 0; it <= bound; ++it) {
        const int p = ld_p(parent + x);
        if (p == x) return x;
        const int g = ld_p(parent + p);
        if (g != p) st_p(parent + x, g);
        x = g;
    }
    bad = true;
    return x;
}

// link the sets of a and b, the larger root under the smaller; a failed compare-and-swap means another lane linked that root
// first (each failure is one link made elsewhere, so at most `bound` retries)
__device__ void uf_union(int* parent, int a, int b, int bound, bool& bad) {
    for (int it = 0; it <= bound; ++it) {
        a = uf_find(parent, a, bound, bad);
        b = uf_find(parent, b, bound, bad);
        if (bad || a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old;
    }
    bad = true;
}

// block-wide exclusive scan of one int per thread (256 threads, 4 waves)
__device__ int block_excl_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[wid] = x;
    __syncthreads();
    int pre = 0, tot = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const int t = s_w[w];
        if (w < wid) pre += t;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return pre + x - v;
}

// word w (columns 64w .. 64w+63) of one mask row, LSB-first; columns >= W (the pad bits of native rows) are cleared
__device__ __forceinline__ u64 load_word(const uint8_t* row, int w, int row_bytes, int W, int vec) {
    u64 m = 0;
    const int b0 = w * 8;
    if (vec == 8) {
        m = *(const u64*)(row + b0);
    } else if (vec == 4) {
        m = *(const unsigned*)(row + b0);
        if (b0 + 4 < row_bytes) m |= (u64)(*(const unsigned*)(row + b0 + 4)) << 32;
    } else {
        for (int k = 0; k < 8 && b0 + k < row_bytes; ++k) m |= (u64)row[b0 + k] << (8 * k);
    }
    const int valid = W - w * 64;
    return valid >= 64 ? m : (m & ((1ull << valid) - 1));
}

// bits (x-1, x, x+1) of an image row as bits 0..2; columns outside [0, 64*WW) read as background
__device__ __forceinline__ unsigned win3(const u64* row, int x, int WW) {
    const int w = x >> 6, b = x & 63;
    const u64 m = row[w];
    unsigned v;
    if (b == 0) {
        v = (unsigned)(m << 1) & 7u;
        if (w > 0) v |= (unsigned)(row[w - 1] >> 63);
    } else {
        v = (unsigned)(m >> (b - 1)) & 7u;
        if (b == 63 && w + 1 < WW) v |= ((unsigned)row[w + 1] & 1u) << 2;
    }
    return v;
}

// polygons.py's 8-neighbourhood, counter-clockwise on the screen: E, NE, N, NW, W, SW, S, SE
static __constant__ int kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
static __constant__ int kDX[8] = {1, 1, 0, -1, -1, -1, 0, 1};

// bit d set iff the neighbour in direction d of (y, x) is foreground
__device__ __forceinline__ unsigned nb8(const u64* img, int WW, int H, int y, int x) {
    const unsigned up = y > 0 ? win3(img + (size_t)(y - 1) * WW, x, WW) : 0u;
    const unsigned mid = win3(img + (size_t)y * WW, x, WW);
    const unsigned dn = y + 1 < H ? win3(img + (size_t)(y + 1) * WW, x, WW) : 0u;
    return ((mid >> 2) & 1u) | ((up >> 2) & 1u) << 1 | ((up >> 1) & 1u) << 2 | (up & 1u) << 3 | (mid & 1u) << 4 |
           (dn & 1u) << 5 | ((dn >> 1) & 1u) << 6 | ((dn >> 2) & 1u) << 7;
}

// _trace_outer + _approx_simple of polygons.py from the start pixel (sy, sx) (its W, NW, N and NE neighbours are background).
// Returns the number of kept vertices and in c0 whether the chain's first point is one of them.  WRITE: the vertices go to
// the emitter in chain order, `c0` being the count pass's answer (the first point's fate is known only at the end).
// `em(pos, y, x, bad)` stores vertex `pos` of the contour (WRITE only).
template <bool WRITE, class Emit>
__device__ int trace_outer(int WW, int H, const u64* img, int sy, int sx, int bound, int& c0, bool& bad, Emit& em) {
    const unsigned nb = nb8(img, WW, H, sy, sx);
    int d0 = -1;
    for (int k = 0; k < 8; ++k) {                   // first neighbour turning CLOCKWISE from west: W, NW, N, NE, E, SE, S, SW
        const int d = (4 - k) & 7;
        if ((nb >> d) & 1u) { d0 = d; break; }
    }
    if (d0 < 0) {                                   // an isolated pixel
        if (WRITE) em(0, sy, sx, bad);
        c0 = 1;
        return 1;
    }
    const int fpy = sy + kDY[d0], fpx = sx + kDX[d0];
    int cy = sy, cx = sx, dprev = d0;               // direction from the current point to the previous one
    int m = 0, d_first = 0, d_in = 0, d = 0, cnt = 0;
    int pos = WRITE ? c0 : 0;
    for (int step = 0;; ++step) {
        if (step > bound) { bad = true; return 0; }
        const unsigned nbc = nb8(img, WW, H, cy, cx);
        const unsigned rot = ((nbc | nbc << 8) >> (dprev + 1)) & 0xffu;     // the previous point's bit is always set
        d = (dprev + 1 + (__builtin_ctz(rot | 0x100u))) & 7;
        const int ny = cy + kDY[d], nx = cx + kDX[d];
        if (ny == sy && nx == sx && cy == fpy && cx == fpx) break;
        if (m == 0) {
            d_first = d;
        } else if (d_in != d) {                     // point m (the current one) is a corner of the chain
            if (WRITE) em(pos, cy, cx, bad);
            ++pos;
            ++cnt;
        }
        d_in = d;
        ++m;
        dprev = (d + 4) & 7;
        cy = ny;
        cx = nx;
    }
    int c0_in;                                      // direction from the chain's last point into its first
    if (cy == sy && cx == sx) {                     // the chain came back to its start: the repeated end point is dropped
        c0_in = d_in;
    } else {                                        // last point = first_prev; it steps to the start along d
        if (d_in != d) {
            if (WRITE) em(pos, cy, cx, bad);
            ++pos;
            ++cnt;
        }
        c0_in = d;
    }
    int keep0 = c0_in != d_first;
    if (cnt + keep0 == 0) keep0 = 1;                // `keep or [chain[0]]`
    if (WRITE) {
        if (keep0 != c0) bad = true;
        else if (keep0) em(0, sy, sx, bad);
    }
    c0 = keep0;
    return cnt + keep0;
}

// Steps b and c of the labelling on the H x WW image: the runs of every row (runs[r] = x0 | x1 << 16 in raster order, row_start = the
// exclusive scan of the per-row counts, row_start[H] = the total R, which is returned) and the union-find that joins 8-connected
// runs of consecutive rows, the larger root always under the smaller.  `parent` comes back as the array the links are in: LDS
// behind the image when IN_LDS and it fits, else parent_g.  `bad`: a loop reached its bound (per thread; the caller combines).
// Ends without a barrier: the caller fences and synchronises before it reads parent[].
template <bool IN_LDS>
__device__ int label_runs(const u64* img, int H, int WW, unsigned* runs, int* row_start, int* parent_g, u64* s_img, int* s_w,
                          int*& parent, bool& bad) {
    const int tid = threadIdx.x;
    // b. runs per row -> row_start (exclusive scan, 256 rows at a time)
    int carry = 0;
    for (int y0 = 0; y0 < H; y0 += kThreads) {
        const int y = y0 + tid;
        int c = 0;
        if (y < H) {
            const u64* row = img + (size_t)y * WW;
            u64 prev = 0;
            for (int w = 0; w < WW; ++w) {
                const u64 mw = row[w];
                c += __popcll(mw & ~((mw << 1) | (prev >> 63)));
                prev = mw;
            }
        }
        int tot;
        const int ex = block_excl_scan(c, s_w, tot);
        if (y < H) row_start[y] = carry + ex;
        carry += tot;
    }
    const int R = carry;
    if (tid == 0) row_start[H] = R;
    // union-find in LDS when it fits next to the image (LDS atomics instead of round trips to L2), else in the scratch
    parent = parent_g;
    if (IN_LDS && (size_t)H * WW * 8 + (size_t)R * 4 <= (size_t)kLdsBytes) parent = (int*)(s_img + (size_t)H * WW);
    __syncthreads();
    for (int y = tid; y < H; y += kThreads) {   // runs[r] = x0 | x1 << 16, in raster order; parent[r] = r
        int r = row_start[y];
        const u64* row = img + (size_t)y * WW;
        u64 prev = 0, cur = row[0];
        int x0 = 0;
        bool open = false;
        for (int w = 0; w < WW; ++w) {
            const u64 next = w + 1 < WW ? row[w + 1] : 0;
            u64 st = cur & ~((cur << 1) | (prev >> 63));
            u64 en = cur & ~((cur >> 1) | (next << 63));
            for (int k = 0; k < 128; ++k) {     // events alternate start / end along the row: one bit per trip
                if (open) {
                    if (!en) break;
                    const int x1 = w * 64 + __builtin_ctzll(en);
                    en &= en - 1;
                    runs[r] = (unsigned)x0 | (unsigned)x1 << 16;
                    st_p(parent + r, r);
                    ++r;
                    open = false;
                } else {
                    if (!st) break;
                    x0 = w * 64 + __builtin_ctzll(st);
                    st &= st - 1;
                    open = true;
                }
            }
            prev = cur;
            cur = next;
        }
    }
    __threadfence();
    __syncthreads();
    // c. 8-connectivity between consecutive rows: run a of row y meets run b of row y-1 iff b.x0 <= a.x1+1 and a.x0 <= b.x1+1
    bad = false;
    for (int y = 1 + tid; y < H; y += kThreads) {
        int i = row_start[y], j = row_start[y - 1];
        const int ie = row_start[y + 1], je = row_start[y];
        while (i < ie && j < je) {              // each trip advances i or j
            const unsigned ra = runs[i], rb = runs[j];
            const int ax0 = ra & 0xffff, ax1 = ra >> 16, bx0 = rb & 0xffff, bx1 = rb >> 16;
            if (bx1 + 1 < ax0) {
                ++j;
            } else if (ax1 + 1 < bx0) {
                ++i;
            } else {
                uf_union(parent, i, j, R, bad);
                if (ax1 < bx1) ++i; else ++j;
            }
        }
    }
    return R;
}

}  // namespace poly
}  // namespace vti
