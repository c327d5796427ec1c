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
// vti_mask_polygons_frames is the same three kernels on the slots of a frame table: poly_slot gives every slot the geometry of its
// frame, and count and write are launched once per form (image in LDS / in the scratch) the table holds, each skipping the other's.
#include <climits>

#include "polygons_dev.h"

namespace vti {

namespace {

using namespace poly;

constexpr int kGroups = VTI_POLY_WORKGROUPS;        // the persistent grid: scratch holds one labelling area per workgroup
constexpr int kHeader = 256;                        // scratch bytes before the first area: the status word

struct PolyArgs {
    const uint8_t* masks;
    int n;
    const int* n_live;
    int H, W, row_bytes, WW, vec;                   // WW: 64-bit words per image row; vec: 8 / 4 / 1 bytes per global load
    int strategy;
    unsigned char* scratch;
    size_t area_bytes, off_runs, off_rows, off_img;
    PolyMap map;                                    // the one geometry's (rows == nullptr)
    int* offsets;
    float* points;
    long long max_points;
    // vti_mask_polygons_frames: the slot's frame is found in slot_offsets[0 .. B] and its geometry comes from that frame's row
    const FrameRow* rows;                           // nullptr: every slot has the geometry above (vti_mask_polygons)
    const int* slot_offsets;
    const long long* bases;                         // the ragged native rows: i64 [B + 1]; nullptr: letterbox masks of H x W
    long long capacity_bytes;
    int B, forms;                                   // forms: the launches this call makes (kFormLds | kFormScratch)
};

// What tracing one slot needs: where its rows are, the image they make and the map of its vertices to the frame.  One function
// serves both calls: vti_mask_polygons' slots all have the geometry of the arguments; a slot of vti_mask_polygons_frames has its
// frame's.  `live` = false: nothing of the slot is read, its polygon is empty.
struct PolySlot {
    const uint8_t* m;
    int H, W, row_bytes, WW, vec;
    bool live, in_lds;
    PolyMap map;
};

__device__ __forceinline__ PolySlot poly_slot(const PolyArgs& a, int slot, int n_live) {
    PolySlot g;
    g.live = slot < n_live;
    g.H = a.H; g.W = a.W; g.row_bytes = a.row_bytes; g.WW = a.WW; g.vec = a.vec;
    g.map = a.map;
    if (!a.rows) {
        g.m = a.masks + (size_t)slot * a.H * a.row_bytes;
        g.in_lds = (size_t)a.H * a.WW * 8 <= (size_t)kLdsBytes;
        return g;
    }
    g.m = a.masks;
    g.in_lds = true;
    if (!g.live) return g;
    int lo = 0, hi = a.B;                           // the last b with slot_offsets[b] <= slot: ends in [0, B) whatever the array holds
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.slot_offsets[mid] <= slot) lo = mid; else hi = mid;
    }
    const int H0 = a.rows[lo].H0, W0 = a.rows[lo].W0;
    if (H0 < 1 || W0 < 1 || H0 > 16384 || W0 > 16384) { g.live = false; return g; }
    long long at = (long long)slot * a.H * a.row_bytes;
    if (a.bases) {                                  // instance i of frame b: H0 rows of 8 ceil(W0 / 64) bytes at bases[b] + i * slot_bytes
        g.H = H0; g.W = W0; g.WW = (W0 + 63) >> 6; g.row_bytes = 8 * g.WW;
        const long long slot_bytes = (long long)H0 * g.row_bytes, inst = (long long)slot - a.slot_offsets[lo], base = a.bases[lo];
        at = base + inst * slot_bytes;
        if (inst < 0 || base < 0 || (base & 7) || at + slot_bytes > a.capacity_bytes) { g.live = false; return g; }
    }
    g.m = a.masks + at;
    g.map = poly_map(g.H, g.W, H0, W0);
    // the areas are pitched by the largest geometry of the host table: a slot that would not fit its area, or whose form this call
    // does not launch (the device table is not the host's), is not traced
    PolyLayout one;
    poly_parts(g.H, g.W, one);
    g.in_lds = one.in_lds;
    if (one.off_runs > a.off_runs || one.off_runs > a.off_rows - a.off_runs || one.off_img - one.off_rows > a.off_img - a.off_rows ||
        one.area_bytes - one.off_img > a.area_bytes - a.off_img || !(a.forms & (one.in_lds ? kFormLds : kFormScratch)))
        g.live = false;
    return g;
}

// the emitter of trace_outer: vertex `pos` of a slot's polygon, mapped to the frame
struct PolyEmit {
    const PolyMap& a; float* out; int limit;
    __device__ __forceinline__ void operator()(int pos, int y, int x, bool& bad) const {
        if (pos >= limit) { bad = true; return; }
        // scale_coords: (c - f32(pad)) / f32(gain) in f32 with correctly rounded division, then clipped to the frame
        const float fx = fminf(fmaxf(__fdiv_rn((float)x - a.padx, a.gain), 0.f), a.W0);
        const float fy = fminf(fmaxf(__fdiv_rn((float)y - a.pady, a.gain), 0.f), a.H0);
        out[2 * (size_t)pos] = fx;
        out[2 * (size_t)pos + 1] = fy;
    }
};

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
    int n_live = a.n;
    if (a.n_live) n_live = min(max(*a.n_live, 0), a.n);

    for (int slot = blockIdx.x; slot < a.n; slot += gridDim.x) {
        const PolySlot g = poly_slot(a, slot, n_live);
        if (!g.live) {                              // a dead slot of a fixed-capacity buffer: not read, empty polygon
            if (!WRITE && tid == 0) a.offsets[slot + 1] = 0;
            continue;
        }
        if (a.rows && g.in_lds != IN_LDS) continue; // the other form's launch traces this slot
        const int H = g.H, W = g.W, WW = g.WW;
        const int trace_bound = 4 * (H + 2) * (W + 2);  // polygons.py's `4 * img.size` guard on the padded image
        PolyEmit no_emit{g.map, nullptr, 0};
        int base = 0, expect = 0;
        if (WRITE) {
            base = a.offsets[slot];
            expect = a.offsets[slot + 1] - base;
            if (expect == 0) continue;
        }
        if (tid == 0) s_bad = 0;
        // a. the mask as H rows of WW zero-padded 64-bit words
        const uint8_t* m = g.m;
#pragma unroll 4
        for (int i = tid; i < H * WW; i += kThreads) {
            const int y = i / WW, w = i - y * WW;
            img[i] = load_word(m + (size_t)y * g.row_bytes, w, g.row_bytes, W, g.vec);
        }
        __syncthreads();
        // b + c. runs per row, row_start, and the union-find over the runs of consecutive rows (polygons_dev.h)
        int* parent;
        bool bad;
        const int R = label_runs<IN_LDS>(img, H, WW, (unsigned*)runs, row_start, parent_g, s_img, s_w, parent, bad);
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
                    const int cnt = trace_outer<false>(WW, H, img, y, (int)(runs[r] & 0xffff), trace_bound, c0, bad, no_emit);
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
                PolyEmit em{g.map, out, expect};
                trace_outer<true>(WW, H, img, lo, (int)(runs[r] & 0xffff), trace_bound, c0, wbad, em);
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
                        PolyEmit em{g.map, out + 2 * (size_t)o, expect - o};
                        trace_outer<true>(WW, H, img, y, (int)(runs[r] & 0xffff), trace_bound, c0, wbad, em);
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

void mask_polygons_layout_frames(const int* H, const int* W, int n, PolyLayout& L) {
    size_t runs = 0, rows = 0, img = 0;
    L = PolyLayout{};
    for (int k = 0; k < n; ++k) {
        PolyLayout one;
        poly_parts(H[k], W[k], one);
        runs = std::max(runs, one.off_runs);
        rows = std::max(rows, one.off_img - one.off_rows);
        img = std::max(img, one.area_bytes - one.off_img);
        L.forms |= one.forms;
        L.WW = std::max(L.WW, one.WW);
        L.img_bytes = std::max(L.img_bytes, one.img_bytes);
    }
    L.in_lds = L.forms == kFormLds;
    L.off_runs = runs;
    L.off_rows = 2 * runs;
    L.off_img = L.off_rows + rows;
    L.area_bytes = L.off_img + img;
    L.total = kHeader + (size_t)kGroups * L.area_bytes;
}

void mask_polygons_layout(int H, int W, int row_bytes, PolyLayout& L) {
    (void)row_bytes;                                // the image is re-laid out in 64-bit words whatever the input rows are
    mask_polygons_layout_frames(&H, &W, 1, L);
}

template <bool WRITE, bool IN_LDS>
static hipError_t launch_one(const PolyArgs& a, int grid, size_t lds, hipStream_t st) {
    return launch_lds<mask_polygons_kernel<WRITE, IN_LDS>>(dim3(grid), dim3(kThreads), lds, st, a);
}

// count (once per form of the layout; each skips the other's slots) -> scan -> write (as count)
static hipError_t launch_all(const PolyArgs& a, int forms, hipStream_t st) {
    const int n = a.n, grid = n < kGroups ? n : kGroups;
    hipError_t e = hipSuccess;
    if (n > 0 && (forms & kFormLds)) e = launch_one<false, true>(a, grid, kLdsBytes, st);
    if (e == hipSuccess && n > 0 && (forms & kFormScratch)) e = launch_one<false, false>(a, grid, 0, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mask_polygons_scan_kernel, dim3(1), dim3(kThreads), 0, st, a.offsets, n, (int*)a.scratch);
    e = hipGetLastError();
    if (e != hipSuccess || n == 0 || !a.points) return e;
    if (forms & kFormLds) e = launch_one<true, true>(a, grid, kLdsBytes, st);
    if (e == hipSuccess && (forms & kFormScratch)) e = launch_one<true, false>(a, grid, 0, st);
    return e;
}

static void fill_common(PolyArgs& a, const PolyLayout& L, int strategy, void* scratch, int* offsets, float* points, long long max_points) {
    a.strategy = strategy;
    a.scratch = (unsigned char*)scratch;
    a.area_bytes = L.area_bytes; a.off_runs = L.off_runs; a.off_rows = L.off_rows; a.off_img = L.off_img;
    a.offsets = offsets; a.points = points; a.max_points = max_points;
    a.forms = L.forms;
}

static int load_vec(const uint8_t* masks, int row_bytes) {
    return ((row_bytes & 7) == 0 && ((uintptr_t)masks & 7) == 0) ? 8 : ((row_bytes & 3) == 0 && ((uintptr_t)masks & 3) == 0) ? 4 : 1;
}

hipError_t launch_mask_polygons(const uint8_t* masks, int n, const int* n_live, int H, int W, int row_bytes, int H0, int W0,
                                int strategy, void* scratch, int* offsets, float* points, long long max_points, hipStream_t st) {
    PolyLayout L;
    mask_polygons_layout(H, W, row_bytes, L);
    PolyArgs a{};
    a.masks = masks; a.n = n; a.n_live = n_live;
    a.H = H; a.W = W; a.row_bytes = row_bytes; a.WW = L.WW;
    a.vec = load_vec(masks, row_bytes);
    a.map = poly_map(H, W, H0, W0);
    fill_common(a, L, strategy, scratch, offsets, points, max_points);
    return launch_all(a, L.forms, st);
}

hipError_t launch_mask_polygons_frames(const uint8_t* masks, const long long* bases, long long capacity_bytes, const int* slot_offsets,
                                       const FrameRow* rows, int B, int capacity, int H, int W, const PolyLayout& L, int strategy,
                                       void* scratch, int* offsets, float* points, long long max_points, hipStream_t st) {
    PolyArgs a{};
    a.masks = masks; a.n = capacity; a.n_live = slot_offsets + B;
    a.H = H; a.W = W; a.row_bytes = W / 8; a.WW = (W + 63) / 64;
    a.vec = bases ? (((uintptr_t)masks & 7) == 0 ? 8 : 1) : load_vec(masks, a.row_bytes);
    a.map = poly_map(H, W, H, W);
    a.rows = rows; a.slot_offsets = slot_offsets; a.bases = bases; a.capacity_bytes = capacity_bytes; a.B = B;
    fill_common(a, L, strategy, scratch, offsets, points, max_points);
    return launch_all(a, L.forms, st);
}

}  // namespace vti
