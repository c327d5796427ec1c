// Results.masks.xy on the device (vti_mask_polygons): the outer border of every 8-connected component of a bit-packed instance
// mask, CHAIN_APPROX_SIMPLE-compressed and mapped to frame pixels, bit-identical to the host restatement in polygons.py
// (masks2segments followed by scale_coords).  DESIGN.md section 5d.
//
// Three launches on the stream, ordered by the kernel boundaries only:
//   1. count:  per slot the number of vertices of its polygon -> offsets[slot + 1] (-1 when a loop bound was exceeded);
//   2. scan:   one workgroup turns those counts into the exclusive scan offsets[0..n] and writes the status word;
//   3. write:  when offsets[n] <= max_points (and the status is 0), every slot's vertices at points[offsets[slot]..].
// Count and write are the same kernel: a workgroup owns one slot at a time (no communication between workgroups) and
//   a. copies the mask into a zero-padded image of 64-bit words (LDS when it fits, else its own part of the scratch),
//   b. lists the horizontal runs of every row (row_start = exclusive scan of the per-row run counts),
//   c. joins the runs of row y to the 8-connected runs of row y-1 with a union-find that always links the larger root under the
//      smaller one (in LDS when it fits beside the image), so a component's root is its raster-first run and the root's first pixel
//      is the start pixel of polygons.py,
//   d. traces the outer border of every component (one lane per component), streaming CHAIN_APPROX_SIMPLE as it goes.
// The write launch repeats a-d (the scratch is per workgroup, not per slot) and then re-traces the chosen contour ("largest") or
// every contour ("concat") with stores.  Every loop is bounded by the image size; exceeding a bound is reported, never spun on.
#include <climits>

#include "vti_internal.h"

namespace vti {

namespace {

constexpr int kThreads = 256;
constexpr int kGroups = VTI_POLY_WORKGROUPS;        // the persistent grid: scratch holds one labelling area per workgroup
constexpr int kHeader = 256;                        // scratch bytes before the first area: the status word
constexpr int kLdsBytes = 156 * 1024;               // dynamic LDS when the image fits (a whole 960 x 1280 mask is 153600 bytes):
                                                    // the image, then parent[] when the slot's runs fit in the rest

typedef unsigned long long u64;

struct PolyArgs {
    const uint8_t* masks;
    int n;
    const int* n_live;
    int H, W, row_bytes, WW, vec;                   // WW: 64-bit words per image row; vec: 8 / 4 / 1 bytes per global load
    int strategy;
    unsigned char* scratch;
    size_t area_bytes, off_runs, off_rows, off_img;
    float padx, pady, gain, W0, H0;
    int* offsets;
    float* points;
    long long max_points;
};

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
__constant__ int kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};
__constant__ int kDX[8] = {1, 1, 0, -1, -1, -1, 0, 1};

// bit d set iff the neighbour in direction d of (y, x) is foreground
__device__ __forceinline__ unsigned nb8(const u64* img, int WW, int H, int y, int x) {
    const unsigned up = y > 0 ? win3(img + (size_t)(y - 1) * WW, x, WW) : 0u;
    const unsigned mid = win3(img + (size_t)y * WW, x, WW);
    const unsigned dn = y + 1 < H ? win3(img + (size_t)(y + 1) * WW, x, WW) : 0u;
    return ((mid >> 2) & 1u) | ((up >> 2) & 1u) << 1 | ((up >> 1) & 1u) << 2 | (up & 1u) << 3 | (mid & 1u) << 4 |
           (dn & 1u) << 5 | ((dn >> 1) & 1u) << 6 | ((dn >> 2) & 1u) << 7;
}

__device__ __forceinline__ void emit(const PolyArgs& a, float* out, int pos, int limit, int y, int x, bool& bad) {
    if (pos >= limit) { bad = true; return; }
    // scale_coords: (c - f32(pad)) / f32(gain) in f32 with correctly rounded division, then clipped to the frame
    const float fx = fminf(fmaxf(__fdiv_rn((float)x - a.padx, a.gain), 0.f), a.W0);
    const float fy = fminf(fmaxf(__fdiv_rn((float)y - a.pady, a.gain), 0.f), a.H0);
    out[2 * (size_t)pos] = fx;
    out[2 * (size_t)pos + 1] = fy;
}

// _trace_outer + _approx_simple of polygons.py from the start pixel (sy, sx) (its W, NW, N and NE neighbours are background).
// Returns the number of kept vertices and in c0 whether the chain's first point is one of them.  WRITE: the vertices go to
// out[0 .. limit) in chain order, `c0` being the count pass's answer (the first point's fate is known only at the end).
template <bool WRITE>
__device__ int trace_outer(const PolyArgs& a, const u64* img, int sy, int sx, int bound, int& c0, bool& bad, float* out, int limit) {
    const int WW = a.WW, H = a.H;
    const unsigned nb = nb8(img, WW, H, sy, sx);
    int d0 = -1;
    for (int k = 0; k < 8; ++k) {                   // first neighbour turning CLOCKWISE from west: W, NW, N, NE, E, SE, S, SW
        const int d = (4 - k) & 7;
        if ((nb >> d) & 1u) { d0 = d; break; }
    }
    if (d0 < 0) {                                   // an isolated pixel
        if (WRITE) emit(a, out, 0, limit, sy, sx, bad);
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
            if (WRITE) emit(a, out, pos, limit, cy, cx, bad);
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
            if (WRITE) emit(a, out, pos, limit, cy, cx, bad);
            ++pos;
            ++cnt;
        }
        c0_in = d;
    }
    int keep0 = c0_in != d_first;
    if (cnt + keep0 == 0) keep0 = 1;                // `keep or [chain[0]]`
    if (WRITE) {
        if (keep0 != c0) bad = true;
        else if (keep0) emit(a, out, 0, limit, sy, sx, bad);
    }
    c0 = keep0;
    return cnt + keep0;
}

template <bool WRITE, bool IN_LDS>
__global__ __launch_bounds__(kThreads) void mask_polygons_kernel(PolyArgs a) {
    extern __shared__ u64 s_img[];
    __shared__ int s_w[kThreads / 64];
    __shared__ long long s_lw[kThreads / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int* status = (int*)a.scratch;
    if (WRITE && (*status != 0 || (long long)a.offsets[a.n] > a.max_points)) return;
    unsigned char* area = a.scratch + kHeader + (size_t)blockIdx.x * a.area_bytes;
    int* const parent_g = (int*)area;
    const unsigned* runs = (const unsigned*)(area + a.off_runs);
    int* row_start = (int*)(area + a.off_rows);
    u64* img = IN_LDS ? s_img : (u64*)(area + a.off_img);
    const int H = a.H, W = a.W, WW = a.WW;
    const int trace_bound = 4 * (H + 2) * (W + 2);  // polygons.py's `4 * img.size` guard on the padded image
    int n_live = a.n;
    if (a.n_live) n_live = min(max(*a.n_live, 0), a.n);

    for (int slot = blockIdx.x; slot < a.n; slot += gridDim.x) {
        if (slot >= n_live) {                       // a dead slot of a fixed-capacity buffer: not read, empty polygon
            if (!WRITE && tid == 0) a.offsets[slot + 1] = 0;
            continue;
        }
        int base = 0, expect = 0;
        if (WRITE) {
            base = a.offsets[slot];
            expect = a.offsets[slot + 1] - base;
            if (expect == 0) continue;
        }
        if (tid == 0) s_bad = 0;
        // a. the mask as H rows of WW zero-padded 64-bit words
        const uint8_t* m = a.masks + (size_t)slot * H * a.row_bytes;
#pragma unroll 4
        for (int i = tid; i < H * WW; i += kThreads) {
            const int y = i / WW, w = i - y * WW;
            img[i] = load_word(m + (size_t)y * a.row_bytes, w, a.row_bytes, W, a.vec);
        }
        __syncthreads();
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
        int* parent = parent_g;
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
                        ((unsigned*)runs)[r] = (unsigned)x0 | (unsigned)x1 << 16;
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
        bool bad = false;
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
        if (bad) s_bad = 1;
        __threadfence();
        __syncthreads();
        // d. one lane per component: trace and count; the root's parent entry becomes ~(count * 2 + first point kept)
        long long best = -1;                        // count << 32 | (INT_MAX - root): the most vertices, then the first root
        int sum = 0;
        bad = s_bad != 0;
        if (!bad) {
            for (int y = tid; y < H; y += kThreads) {
                for (int r = row_start[y]; r < row_start[y + 1]; ++r) {
                    if (ld_p(parent + r) != r) continue;
                    int c0 = 0;
                    const int cnt = trace_outer<false>(a, img, y, (int)(runs[r] & 0xffff), trace_bound, c0, bad, nullptr, 0);
                    st_p(parent + r, ~(cnt * 2 + c0));
                    sum += cnt;
                    best = max(best, (long long)cnt << 32 | (unsigned)(INT_MAX - r));
                }
            }
        }
        if (bad) s_bad = 1;
        for (int o = 32; o > 0; o >>= 1) {
            sum += __shfl_xor(sum, o, 64);
            best = max(best, (long long)__shfl_xor(best, o, 64));
        }
        if (lane == 0) { s_w[wid] = sum; s_lw[wid] = best; }
        __threadfence();
        __syncthreads();
        int total = 0;
        best = -1;
        for (int w = 0; w < kThreads / 64; ++w) { total += s_w[w]; best = max(best, s_lw[w]); }
        bad = s_bad != 0;
        __syncthreads();                            // s_w is the concat scan's next
        const int count = bad ? -1 : (a.strategy == VTI_POLY_LARGEST ? (best < 0 ? 0 : (int)(best >> 32)) : total);
        if (!WRITE) {
            if (tid == 0) a.offsets[slot + 1] = count;
            __syncthreads();                        // s_w / s_lw / s_bad are reused by the next slot
            continue;
        }
        if (count != expect) {                      // the count launch saw another answer: write nothing
            if (tid == 0) atomicOr(status, VTI_POLY_ERR_BOUND);
            __syncthreads();
            continue;
        }
        float* out = a.points + 2 * (size_t)base;
        if (a.strategy == VTI_POLY_LARGEST) {
            if (tid == 0 && best >= 0) {
                const int r = INT_MAX - (int)(unsigned)(best & 0xffffffffll);
                int lo = 0, hi = H - 1;             // the root's row: the last y with row_start[y] <= r
                for (int k = 0; k < 32 && lo < hi; ++k) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (row_start[mid] <= r) lo = mid; else hi = mid - 1;
                }
                int c0 = (~ld_p(parent + r)) & 1;
                bool wbad = false;
                trace_outer<true>(a, img, lo, (int)(runs[r] & 0xffff), trace_bound, c0, wbad, out, expect);
                if (wbad) atomicOr(status, VTI_POLY_ERR_BOUND);
            }
        } else {
            // every component in raster order of its start pixel: an exclusive scan of the root counts over contiguous run ranges
            const int per = (R + kThreads - 1) / kThreads, r0 = min(tid * per, R), r1 = min(r0 + per, R);
            int local = 0;
            for (int r = r0; r < r1; ++r) {
                const int code = ld_p(parent + r);
                if (code < 0) local += (~code) >> 1;
            }
            int tot;
            int off = block_excl_scan(local, s_w, tot);
            for (int r = r0; r < r1; ++r) {
                const int code = ld_p(parent + r);
                if (code < 0) {
                    st_p(parent + r, ~(off * 2 + ((~code) & 1)));
                    off += (~code) >> 1;
                }
            }
            __threadfence();
            __syncthreads();
            bool wbad = tot != expect;
            if (!wbad) {
                for (int y = tid; y < H; y += kThreads) {
                    for (int r = row_start[y]; r < row_start[y + 1]; ++r) {
                        const int code = ld_p(parent + r);
                        if (code >= 0) continue;
                        const int o = (~code) >> 1;
                        int c0 = (~code) & 1;
                        trace_outer<true>(a, img, y, (int)(runs[r] & 0xffff), trace_bound, c0, wbad, out + 2 * (size_t)o, expect - o);
                    }
                }
            }
            if (wbad) atomicOr(status, VTI_POLY_ERR_BOUND);
        }
        __syncthreads();
    }
}

// offsets[1..n] hold the per-slot counts (-1: a bound was exceeded) -> the exclusive scan offsets[0..n] and the status word
__global__ __launch_bounds__(kThreads) void mask_polygons_scan_kernel(int* offsets, int n, int* status) {
    __shared__ long long s_w[kThreads / 64];
    __shared__ int s_flags;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) s_flags = 0;
    __syncthreads();
    long long carry = 0;
    for (int b0 = 0; b0 < n; b0 += kThreads) {
        const int i = b0 + tid;
        long long v = 0;
        if (i < n) {
            const int c = offsets[i + 1];
            if (c < 0) atomicOr(&s_flags, VTI_POLY_ERR_BOUND);
            else v = c;
        }
        long long x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) s_w[wid] = x;
        __syncthreads();
        long long pre = 0, tot = 0;
        for (int w = 0; w < kThreads / 64; ++w) {
            const long long t = s_w[w];
            if (w < wid) pre += t;
            tot += t;
        }
        __syncthreads();
        const long long incl = carry + pre + x;
        if (i < n) {
            if (incl > INT_MAX) atomicOr(&s_flags, VTI_POLY_ERR_RANGE);
            offsets[i + 1] = incl > INT_MAX ? INT_MAX : (int)incl;
        }
        carry += tot;
    }
    __syncthreads();
    if (tid == 0) {
        offsets[0] = 0;
        *status = s_flags;
    }
}

}  // namespace

void mask_polygons_layout(int H, int W, int row_bytes, PolyLayout& L) {
    (void)row_bytes;                                // the image is re-laid out in 64-bit words whatever the input rows are
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t r_max = (size_t)H * (size_t)((W + 1) / 2);     // at most ceil(W/2) runs per row
    L.WW = (W + 63) / 64;
    L.img_bytes = (size_t)H * L.WW * 8;
    L.in_lds = L.img_bytes <= (size_t)kLdsBytes;
    L.off_runs = al(r_max * 4);
    L.off_rows = L.off_runs + al(r_max * 4);
    L.off_img = L.off_rows + al((size_t)(H + 1) * 4);
    L.area_bytes = L.off_img + (L.in_lds ? 0 : al(L.img_bytes));
    L.total = kHeader + (size_t)kGroups * L.area_bytes;
}

template <bool WRITE, bool IN_LDS>
static hipError_t launch_one(const PolyArgs& a, int grid, size_t lds, hipStream_t st) {
    return launch_lds<mask_polygons_kernel<WRITE, IN_LDS>>(dim3(grid), dim3(kThreads), lds, st, a);
}

hipError_t launch_mask_polygons(const uint8_t* masks, int n, const int* n_live, int H, int W, int row_bytes, double gain,
                                double padx, double pady, int H0, int W0, int strategy, void* scratch, int* offsets, float* points,
                                long long max_points, hipStream_t st) {
    PolyLayout L;
    mask_polygons_layout(H, W, row_bytes, L);
    PolyArgs a;
    a.masks = masks; a.n = n; a.n_live = n_live;
    a.H = H; a.W = W; a.row_bytes = row_bytes; a.WW = L.WW;
    a.vec = ((row_bytes & 7) == 0 && ((uintptr_t)masks & 7) == 0) ? 8 : ((row_bytes & 3) == 0 && ((uintptr_t)masks & 3) == 0) ? 4 : 1;
    a.strategy = strategy;
    a.scratch = (unsigned char*)scratch;
    a.area_bytes = L.area_bytes; a.off_runs = L.off_runs; a.off_rows = L.off_rows; a.off_img = L.off_img;
    a.padx = (float)padx; a.pady = (float)pady; a.gain = (float)gain; a.W0 = (float)W0; a.H0 = (float)H0;
    a.offsets = offsets; a.points = points; a.max_points = max_points;
    const int grid = n < kGroups ? n : kGroups;
    const size_t lds = L.in_lds ? kLdsBytes : 0;
    hipError_t e = hipSuccess;
    if (n > 0) e = L.in_lds ? launch_one<false, true>(a, grid, lds, st) : launch_one<false, false>(a, grid, lds, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mask_polygons_scan_kernel, dim3(1), dim3(kThreads), 0, st, offsets, n, (int*)scratch);
    e = hipGetLastError();
    if (e != hipSuccess || n == 0 || !points) return e;
    return L.in_lds ? launch_one<true, true>(a, grid, lds, st) : launch_one<true, false>(a, grid, lds, st);
}

}  // namespace vti
