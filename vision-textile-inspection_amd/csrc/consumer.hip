// Consumer-side reductions of measurement.py on the GPU, second generation:
//   * A4 + A7 and A4 + A5 + A6 straight from the BIT-PACKED masks vti_masks writes: the nearest resize to the frame
//     (measurement.py:79, cv2.INTER_NEAREST) is folded into integer weight tables, so no [n, H0, W0] bitmap is ever
//     materialised and the consumer's payload shrinks from n*H*W bytes to n*5 + W0 integers (what a multi-GPU gather ships);
//   * N3: batched pixel -> world (cv2.undistortPoints' 5-iteration inverse of the k1,k2,p1,p2,k3 model + ray/plane
//     intersection, measurement.py:44-65) and the 1-D 2-means of measurement.py:88-113, in float64 as the reference.
// All integer results are exact; the float64 ones follow the reference's operation order (-ffp-contract=off).
#include <climits>
#include <cstring>
#include <type_traits>

#include "measure_dev.h"

namespace vti {

// ---- A4 + A7: per-instance moments / column extents of the frame-sized bitmap, from the bit-packed mask -------------
// Destination pixel (y, x) of the H0 x W0 bitmap copies source pixel (sy(y), sx(x)); so with
//   cx[sx] = #{x : sx(x) = sx}, xs[sx] = sum of those x, cy[sy], ys[sy] likewise,
//   m00 = sum_set cy*cx,  m10 = sum_set cy*xs,  m01 = sum_set ys*cx,  min/max col = first/last x of the extreme set sx
// (over set source pixels that have at least one destination row and column).  One workgroup per instance.
// VW = 32-bit words per load (4: 16-byte loads, slots a multiple of 16 bytes; 2: 8-byte loads, for the native rows of
// vti_masks_native, whose slots are only a multiple of 8 bytes).  RAW: raw[slot] = 1 iff any bit of the slot is set, the emptiness
// of the mask as predict returns it (vti_measure's drop_empty), before the resize can skip set source pixels.
// FRAMES (vti_measure_frames): the frames differ in size; the slot's frame is found in offsets[0 .. B] (instance i of frame b is slot
// offsets[b] + i) and H0, W0 are that frame's, from its row of the frame table.  The search ends at an index in [0, B) whatever
// the offsets hold, so no table address is formed outside the B rows.
// RAGGED (vti_measure_frames_native; with FRAMES, VW = 2): the slots are the frame-size rows of vti_masks_native_frames.  Instance i of
// frame b starts at byte bases[b] + i * slot_bytes[b] and is H0[b] rows of 2 ceil(W0[b] / 64) words (the identity branch, as the
// uniform native call); a slot that does not end at or before capacity_bytes -- or whose offsets / bases do not place it inside the
// buffer at an 8-byte boundary -- is the empty mask and nothing of it is read.
template <int VW, bool RAW, bool FRAMES = false, bool RAGGED = false>
__global__ __launch_bounds__(256) void mask_stats_bits_kernel(const unsigned* __restrict__ bits, const int* __restrict__ n_live,
                                                              int H, int W, int H0, int W0, long long* __restrict__ stats,
                                                              int* __restrict__ raw, const int* __restrict__ offsets = nullptr,
                                                              const FrameRow* __restrict__ frames = nullptr, int B = 0,
                                                              const long long* __restrict__ bases = nullptr, long long capacity_bytes = 0) {
    extern __shared__ int tab[];            // cx[W] xs[W] xf[W] xl[W] cy[H] ys[H]
    int* cx = tab; int* xs = cx + W; int* xf = xs + W; int* xl = xf + W; int* cy = xl + W; int* ys = cy + H;
    const int tid = threadIdx.x, slot = blockIdx.x;
    if (n_live && slot >= *n_live) {        // a dead slot of a fixed-capacity buffer: the empty-mask answer, nothing read
        if (tid < 5) stats[(size_t)slot * 5 + tid] = tid < 3 ? 0 : -1;
        if (RAW && tid == 0) raw[slot] = 0;
        return;
    }
    if (FRAMES) {
        int lo = 0, hi = B;                 // the last b with offsets[b] <= slot
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] <= slot) lo = mid; else hi = mid;
        }
        H0 = frames[lo].H0; W0 = frames[lo].W0;
        if (RAGGED) {
            const int wpr_b = 2 * ((W0 + 63) / 64);
            const long long slot_bytes = (long long)H0 * wpr_b * 4, inst = (long long)slot - offsets[lo], at = bases[lo] + inst * slot_bytes;
            if (inst < 0 || bases[lo] < 0 || (bases[lo] & 7) || at + slot_bytes > capacity_bytes) {
                if (tid < 5) stats[(size_t)slot * 5 + tid] = tid < 3 ? 0 : -1;
                if (RAW && tid == 0) raw[slot] = 0;
                return;
            }
            H = H0; W = W0 = 32 * wpr_b;
            bits += at >> 2;
        }
    }
    const bool ident = H0 == H && W0 == W;
    if (!ident) {
        for (int i = tid; i < W; i += 256) { cx[i] = 0; xs[i] = 0; xf[i] = INT_MAX; xl[i] = -1; }
        for (int i = tid; i < H; i += 256) { cy[i] = 0; ys[i] = 0; }
        __syncthreads();
        const double ifx = 1.0 / ((double)W0 / (double)W), ify = 1.0 / ((double)H0 / (double)H);
        for (int x = tid; x < W0; x += 256) {
            const int s = nn_src(x, ifx, W);
            atomicAdd(&cx[s], 1); atomicAdd(&xs[s], x); atomicMin(&xf[s], x); atomicMax(&xl[s], x);
        }
        for (int y = tid; y < H0; y += 256) {
            const int s = nn_src(y, ify, H);
            atomicAdd(&cy[s], 1); atomicAdd(&ys[s], y);
        }
        __syncthreads();
    }
    const int wpr = W >> 5;                 // 32-bit words per mask row (W is a multiple of 32)
    // a slot is H * W / 8 bytes, a multiple of 128 (H, W multiples of 32), and `bits` is 16-byte aligned (checked by the launcher):
    // 16-byte loads, four of them in flight per thread before the first word is looked at (the loop was one dependent 4-byte load
    // per trip: latency-bound at a third of what the masks' L2 / HBM residency gives)
    using V = typename std::conditional<VW == 4, uint4, uint2>::type;
    const V* m4 = (const V*)(RAGGED ? bits : bits + (size_t)slot * H * wpr);
    const int n4 = (H * wpr) / VW;
    long long m00 = 0, m10 = 0, m01 = 0;
    int mn = INT_MAX, mx = -1, seen = 0;
    auto word = [&](unsigned w, int sy, int x0) {
        if (!w) return;
        if (ident) {
            const int pc = __popc(w);
            // sum of the set bit positions: bit k of a position contributes 2^k times the population of its mask
            const int ps = __popc(w & 0xAAAAAAAAu) + 2 * __popc(w & 0xCCCCCCCCu) + 4 * __popc(w & 0xF0F0F0F0u) +
                           8 * __popc(w & 0xFF00FF00u) + 16 * __popc(w & 0xFFFF0000u);
            m00 += pc; m10 += (long long)x0 * pc + ps; m01 += (long long)sy * pc;
            mn = min(mn, x0 + __ffs(w) - 1); mx = max(mx, x0 + 31 - __clz(w));
        } else {
            const int wy = cy[sy];
            if (!wy) return;
            long long rc = 0, rx = 0;
            while (w) {
                const int sx = x0 + __ffs(w) - 1;
                w &= w - 1;
                if (!cx[sx]) continue;
                rc += cx[sx]; rx += xs[sx];
                mn = min(mn, xf[sx]); mx = max(mx, xl[sx]);
            }
            m00 += rc * wy; m10 += rx * wy; m01 += rc * ys[sy];
        }
    };
    constexpr int U = 4;
    for (int i0 = tid; i0 < n4; i0 += 256 * U) {
        V q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = i0 + 256 * u;
            q[u] = i < n4 ? m4[i] : V{};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const unsigned* ww = reinterpret_cast<const unsigned*>(&q[u]);
            unsigned any = 0;
#pragma unroll
            for (int k = 0; k < VW; ++k) any |= ww[k];
            if (!any) continue;
            if (RAW) seen = 1;
            const int i = (i0 + 256 * u) * VW;
            int sy = i / wpr, c = i - sy * wpr;                           // word column inside the row; the words may cross a row end
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                word(ww[k], sy, c << 5);
                if (++c == wpr) { c = 0; ++sy; }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        m00 += __shfl_down(m00, o); m10 += __shfl_down(m10, o); m01 += __shfl_down(m01, o);
        mn = min(mn, __shfl_down(mn, o)); mx = max(mx, __shfl_down(mx, o));
        if (RAW) seen |= __shfl_down(seen, o);
    }
    __shared__ long long r00[4], r10[4], r01[4];
    __shared__ int rmn[4], rmx[4], rsn[4];
    if ((tid & 63) == 0) {
        r00[tid >> 6] = m00; r10[tid >> 6] = m10; r01[tid >> 6] = m01; rmn[tid >> 6] = mn; rmx[tid >> 6] = mx;
        if (RAW) rsn[tid >> 6] = seen;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            m00 += r00[w]; m10 += r10[w]; m01 += r01[w]; mn = min(mn, rmn[w]); mx = max(mx, rmx[w]);
            if (RAW) seen |= rsn[w];
        }
        long long* o = stats + (size_t)slot * 5;
        o[0] = m00; o[1] = m10; o[2] = m01; o[3] = m00 ? mn : -1; o[4] = mx;
        if (RAW) raw[slot] = seen;
    }
}

hipError_t launch_mask_stats_bits(const uint8_t* bits, int n, const int* n_live, int H, int W, int H0, int W0, long long* stats,
                                  hipStream_t st) {
    if (n == 0) return hipSuccess;
    if ((W & 31) || (H & 31) || ((uintptr_t)bits & 15) || (size_t)(4 * W + 2 * H) * 4 > 60 * 1024) return hipErrorInvalidValue;      // 16-byte loads
    hipLaunchKernelGGL((mask_stats_bits_kernel<4, false>), dim3(n), dim3(256), (size_t)(4 * W + 2 * H) * 4, st, (const unsigned*)bits, n_live,
                       H, W, H0, W0, stats, (int*)nullptr, (const int*)nullptr, (const FrameRow*)nullptr, 0);
    return hipGetLastError();
}

// ---- A4 + A5 + A6, batched: per frame the lower envelope of the union of its instances of class `cls` -----------------
// (measurement.py:160-185 on the frame-sized bitmaps of measurement.py:70-86).  envelope[b, x] = the largest frame row y whose
// source pixel (sy(y), sx(x)) is set in ANY selected instance, -1 if none.  yl[sy] = last frame row that maps to sy (-1: none),
// monotone in sy, so the answer is yl of the largest set source row.  A mask is zero outside its box grown by 8 px (two
// prototype pixels of bilinear reach, the same bound mask_plan_kernel uses), so only those rows are read.
// vti_measure adds two things (measurement.py:253-260, 280-289): an ROI filter on the frame-px boxes `xyxy` (roi_on = 0: none; an
// instance is kept when the centre of its int-truncated box lies inside roi = {x_min, y_min, x_max, y_max}, bounds inclusive), and
// the NATIVE form for the frame-size rows of vti_masks_native (wpr words per row, zero pad bits): there the resize is the identity
// and a mask is zero outside the rows [y1, y2) of its frame-px box, so those bound the search.
// `sel` carries the class and the ROI as given (clamped to H0 x W0 here).  With a camera table (`table` != nullptr,
// vti_measure_cameras) they come from row cam_of_frame[b] instead, range-checked against n_cams before the row's address is formed;
// a frame whose index is outside gets an all -1 envelope.
struct EnvSel { int cls, roi_enabled, roi[4]; };
template <bool NATIVE>
__global__ __launch_bounds__(256) void envelope_bits_kernel(const unsigned* __restrict__ bits, const int* __restrict__ offsets,
                                                            const float* __restrict__ dets, int max_det, int row, int capacity,
                                                            EnvSel sel, int H, int W, int H0, int W0, int* __restrict__ envelope,
                                                            const float* __restrict__ xyxy, int native_wpr,
                                                            const CameraRow* __restrict__ table, const int* __restrict__ cam_of_frame,
                                                            int n_cams, const FrameRow* __restrict__ frames = nullptr,
                                                            const long long* __restrict__ bases = nullptr, long long capacity_bytes = 0) {
    extern __shared__ int yl[];             // [H] (not NATIVE)
    __shared__ int red[4][64];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int pitch = W0;                   // of the envelope rows: W0, or the largest W0 of a frame table (the grid covers it)
    if (frames) {
        H0 = frames[b].H0; W0 = frames[b].W0;
        if ((int)blockIdx.x * 64 >= W0) return;                 // columns this frame does not have: nothing is written
    }
    if (table) {
        const int ci = cam_of_frame[b];
        if (ci < 0 || ci >= n_cams) {                           // uniform over the workgroup
            const int xo = blockIdx.x * 64 + tid;
            if (tid < 64 && xo < W0) envelope[(size_t)b * pitch + xo] = -1;
            return;
        }
        const CameraRow* c = table + ci;
        sel.cls = c->fabric_id; sel.roi_enabled = c->roi_enabled;
        for (int k = 0; k < 4; ++k) sel.roi[k] = c->roi[k];
    }
    const int cls = sel.cls;
    int4 roi;
    const bool roi_on = roi_clamp(sel.roi_enabled, sel.roi, H0, W0, roi);
    if (!NATIVE) {
        for (int i = tid; i < H; i += 256) yl[i] = -1;
        __syncthreads();
        const double ify = 1.0 / ((double)H0 / (double)H);
        for (int y = tid; y < H0; y += 256) atomicMax(&yl[nn_src(y, ify, H)], y);
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (tid & 63), rg = tid >> 6;
    const int xc = x < W0 ? x : W0 - 1;
    const int sx = NATIVE ? xc : nn_src(xc, 1.0 / ((double)W0 / (double)W), W);
    const bool ragged = NATIVE && bases;    // vti_measure_frames_native: the frame's own rows, from bases[b] on
    const int wpr = NATIVE ? (ragged ? 2 * ((W0 + 63) / 64) : native_wpr) : W >> 5;
    const int Hm = NATIVE ? H0 : H;         // rows of a mask slot
    const int s0 = offsets[b];
    int s1 = min(offsets[b + 1], capacity);
    const unsigned* fbits = bits;           // where slot `srel` starts
    int srel = 0;
    if (ragged) {                           // the instances whose slot ends at or before capacity_bytes; none if the base is no offset
        const long long base = bases[b], slot_bytes = (long long)Hm * wpr * 4;
        const long long fit = base >= 0 && !(base & 7) && capacity_bytes > base ? (capacity_bytes - base) / slot_bytes : 0;
        s1 = (int)min((long long)s1, (long long)s0 + fit);
        if (s1 > s0) fbits = bits + (base >> 2);
        srel = s0;
    }
    int env = -1;
    // the frame's instances of the wanted class, listed first (a thread per instance; the order is irrelevant to a max): the row
    // search below then runs over those only -- walking all instances with one dependent class load each was the kernel's time
    __shared__ int s_sel[256][3];
    __shared__ int s_nsel;
    for (int r0 = s0; r0 < s1; r0 += 256) {
        __syncthreads();                                       // the previous round's list has been consumed
        if (tid == 0) s_nsel = 0;
        __syncthreads();
        if (r0 + tid < s1) {
            const size_t di = (size_t)b * max_det + (r0 + tid - s0);
            const float* d = dets + di * row;
            if ((cls < 0 || (int)d[5] == cls) && (!roi_on || roi_keeps(xyxy + di * 4, roi))) {
                int ya, yb;
                if (NATIVE) { ya = (int)floorf(xyxy[di * 4 + 1]); yb = (int)ceilf(xyxy[di * 4 + 3]); }
                else { ya = (int)floorf(d[1] - 8.f); yb = (int)ceilf(d[3] + 8.f); }
                ya = max(ya, 0); yb = min(yb, Hm - 1);
                const int pos = atomicAdd(&s_nsel, 1);
                s_sel[pos][0] = r0 + tid; s_sel[pos][1] = ya; s_sel[pos][2] = yb;
            }
        }
        __syncthreads();
        const int nsel = s_nsel;
        for (int j = 0; j < nsel; ++j) {
            const int s = s_sel[j][0], ya = s_sel[j][1], yb = s_sel[j][2];
            const unsigned* m = fbits + (size_t)(s - srel) * Hm * wpr + (sx >> 5);
            for (int sy = yb - rg; sy >= ya; sy -= 4) {           // top of the search first: the first hit of a lane is its largest
                if ((m[(size_t)sy * wpr] >> (sx & 31)) & 1u) {
                    const int y = NATIVE ? sy : yl[sy];
                    env = max(env, y);
                    if (y >= 0) break;
                }
            }
        }
    }
    red[rg][tid & 63] = env;
    __syncthreads();
    if (rg == 0 && x < W0) envelope[(size_t)b * pitch + x] = max(max(red[0][tid], red[1][tid]), max(red[2][tid], red[3][tid]));
}

hipError_t launch_envelope_bits(const uint8_t* bits, const int* offsets, const float* dets, int B, int max_det, int nm,
                                int capacity, int cls, int H, int W, int H0, int W0, int* envelope, hipStream_t st) {
    if (B == 0) return hipSuccess;
    if ((W & 31) || ((uintptr_t)bits & 3) || (size_t)H * 4 > 60 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(envelope_bits_kernel<false>, dim3((W0 + 63) / 64, B), dim3(256), (size_t)H * 4, st, (const unsigned*)bits, offsets,
                       dets, max_det, 6 + nm, capacity, EnvSel{cls, 0, {0, 0, 0, 0}}, H, W, H0, W0, envelope, (const float*)nullptr, 0,
                       (const CameraRow*)nullptr, (const int*)nullptr, 0, (const FrameRow*)nullptr);
    return hipGetLastError();
}

// ---- N3a: pixel -> world on the fabric plane (measurement.py:44-65) ----------------------------------------------------
// cv2.undistortPoints(pts, K, dist, P=None) with its default criteria (COUNT 5): x0 = (u - cx) / fx, then 5 fixed-point steps
//   r2 = x^2 + y^2; icdist = 1 / (1 + ((k3 r2 + k2) r2 + k1) r2); dX = 2 p1 x y + p2 (r2 + 2 x^2); dY = p1 (r2 + 2 y^2) + 2 p2 x y
//   x = (x0 - dX) icdist; y = (y0 - dY) icdist          (k4..k6, s1..s4, tilt = 0 for the 5-coefficient model of
// camera_calibration.json; OpenCV leaves the loop if icdist < 0).  Then the ray (x, y, 1) meets the plane n.X + d = 0:
//   s = -d / (n . ray); X_cam = s ray; X_world = R^T (X_cam - t); no point when |n . ray| < 1e-9.
// (GeomParams: with CameraRow in measure_dev.h.)

// (pixel_to_world itself: measure_dev.h, shared with vti_annotate_checker's prep kernel.)

__global__ __launch_bounds__(256) void pixels_to_world_kernel(const double* __restrict__ uv, int n, GeomParams g,
                                                               double* __restrict__ xyz, int* __restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double o[3];
    const bool ok = pixel_to_world(g, uv[2 * i], uv[2 * i + 1], o);
    double* out = xyz + 3 * (size_t)i;
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = o[k];
    valid[i] = ok ? 1 : 0;
}

static GeomParams make_geom(const double* K, const double* dist, const double* R, const double* t) {
    GeomParams g;
    g.fx = K[0]; g.fy = K[4]; g.cx = K[2]; g.cy = K[5];
    g.k1 = dist[0]; g.k2 = dist[1]; g.p1 = dist[2]; g.p2 = dist[3]; g.k3 = dist[4];
    for (int i = 0; i < 9; ++i) g.R[i] = R[i];
    for (int i = 0; i < 3; ++i) { g.t[i] = t[i]; g.n[i] = R[3 * i + 2]; }       // plane normal = third column of R (measurement.py:46)
    g.d = -((g.n[0] * g.t[0] + g.n[1] * g.t[1]) + g.n[2] * g.t[2]);            // measurement.py:47
    return g;
}

hipError_t launch_pixels_to_world(const double* uv, int n, const double* K, const double* dist, const double* R,
                                  const double* t, double* xyz, int* valid, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(pixels_to_world_kernel, dim3((n + 255) / 256), dim3(256), 0, st, uv, n, make_geom(K, dist, R, t), xyz, valid);
    return hipGetLastError();
}

// ---- N3b: kmeans_1d_two_clusters (measurement.py:88-113), one wave per frame ------------------------------------------
// numpy's float64 `mean` = pairwise sum / count; the loop's exit test compares the new centres with `==`, so the sums are
// formed exactly as numpy forms them (8 interleaved partial sums per block of <= 128, halves above that).
__device__ __forceinline__ double np_pairwise_leaf(const double* a, int n) {       // n <= 128
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
}

// numpy recurses on halves above 128 elements (the first half a multiple of 8 long): sum(a, n) = sum(a, n2) + sum(a + n2, n - n2).
// Evaluated here with an explicit frame stack (depth <= log2(n / 128) + 1).
__device__ double np_pairwise_sum(const double* a, int n) {
    struct Fr { int off, n, state; double left; };
    Fr fr[12];
    fr[0] = {0, n, 0, 0.0};
    int sp = 1;
    double ret = 0.0;
    while (sp > 0) {
        Fr& f = fr[sp - 1];
        if (f.n <= 128) { ret = np_pairwise_leaf(a + f.off, f.n); --sp; continue; }
        int n2 = f.n / 2;
        n2 -= n2 % 8;
        if (f.state == 0) { f.state = 1; fr[sp] = {f.off, n2, 0, 0.0}; ++sp; }
        else if (f.state == 1) { f.left = ret; f.state = 2; fr[sp] = {f.off + n2, f.n - n2, 0, 0.0}; ++sp; }
        else { ret = f.left + ret; --sp; }
    }
    return ret;
}

// The loop of measurement.py:93-113 on one thread for n >= 2 values; lab0[0, n) must be 0 on entry (the initial `labels`).  Returns
// 0 or 1: which of lab0 / lab1 holds the returned labels (the PREVIOUS assignment when the loop stops early); g0, g1: n doubles of
// scratch each.  Shared by kmeans1d2_kernel and measure_frames_kernel.
// LATEST (checker_frames_kernel): check_stitch_distance.py:143-171 is the same loop, but sets `labels = new_labels` on both early
// exits, so the assignment just computed is the one returned.  The two texts differ when the loop stops in its first pass on
// unchanged seeds (two tight rows whose means are their min and max): the first keeps the initial zeros, this one the split.
template <bool LATEST = false>
__device__ int kmeans1d2_serial(const double* vals, int n, int max_iters, int* lab0, int* lab1, double* g0, double* g1, double& c0,
                                double& c1) {
    c0 = vals[0]; c1 = vals[0];
    for (int i = 1; i < n; ++i) { c0 = fmin(c0, vals[i]); c1 = fmax(c1, vals[i]); }
    int cur = 0;                            // lab[cur] = `labels`, lab[cur ^ 1] = `new_labels`
    for (int it = 0; it < max_iters; ++it) {
        int* nl = cur ? lab0 : lab1;
        int n1 = 0, k0 = 0, k1 = 0;
        for (int i = 0; i < n; ++i) {
            const int l = fabs(vals[i] - c1) < fabs(vals[i] - c0) ? 1 : 0;
            nl[i] = l; n1 += l;
            if (l) g1[k1++] = vals[i]; else g0[k0++] = vals[i];
        }
        if (n1 == 0 || n1 == n) { if (LATEST) cur ^= 1; break; }
        const double nc0 = np_pairwise_sum(g0, k0) / (double)k0, nc1 = np_pairwise_sum(g1, k1) / (double)k1;
        if (nc0 == c0 && nc1 == c1) { if (LATEST) cur ^= 1; break; }
        c0 = nc0; c1 = nc1; cur ^= 1;
    }
    return cur;
}

__global__ __launch_bounds__(64) void kmeans1d2_kernel(const double* __restrict__ values, const int* __restrict__ counts, int max_n,
                                                       int max_iters, int* __restrict__ labels, double* __restrict__ centers) {
    extern __shared__ double sm[];          // vals[max_n] | group0[max_n] | group1[max_n]
    double* vals = sm; double* g0 = sm + max_n; double* g1 = g0 + max_n;
    __shared__ int lab[2][1024];
    const int b = blockIdx.x, lane = threadIdx.x;
    int n = counts[b];
    n = n < 0 ? 0 : (n > max_n ? max_n : n);
    const double* v = values + (size_t)b * max_n;
    int* L = labels + (size_t)b * max_n;
    for (int i = lane; i < n; i += 64) { vals[i] = v[i]; lab[0][i] = 0; }
    for (int i = lane; i < max_n; i += 64) L[i] = 0;
    __syncthreads();
    if (lane != 0) return;                  // <= a few hundred values: the order-exact sums are serial anyway
    if (n < 2) {                            // measurement.py:90-91: all zeros, both centres = mean (NaN for an empty input, as numpy)
        const double m = n ? vals[0] : __builtin_nan("");
        centers[2 * b] = m; centers[2 * b + 1] = m;
        return;
    }
    double c0, c1;
    const int cur = kmeans1d2_serial(vals, n, max_iters, lab[0], lab[1], g0, g1, c0, c1);
    for (int i = 0; i < n; ++i) L[i] = lab[cur][i];
    centers[2 * b] = c0; centers[2 * b + 1] = c1;
}

hipError_t launch_kmeans1d2(const double* values, const int* counts, int B, int max_n, int max_iters, int* labels,
                            double* centers, hipStream_t st) {
    if (B == 0) return hipSuccess;
    if (max_n < 1 || max_n > 1024) return hipErrorInvalidValue;     // LDS tables; the reference caps detections at 200 (config.py:73)
    hipLaunchKernelGGL(kmeans1d2_kernel, dim3(B), dim3(64), (size_t)max_n * 3 * sizeof(double), st, values, counts, max_n, max_iters,
                       labels, centers);
    return hipGetLastError();
}

// ---- process_frame's measurement record (measurement.py:240-472), one workgroup per frame -----------------------------------
// Inputs: per-slot moments (mask_stats_bits_kernel, frame-size bitmap) and raw emptiness, and the frame's lower envelope of its
// ROI-kept fabric masks (envelope_bits_kernel).  Steps, in the reference's order:
//   1. instances in detection order -> the stitch list (ballot / prefix counts: the order feeds the pairwise sums and the 2-means)
//      and the count of non-empty kept fabric masks;
//   2. status: no fabric / empty union, then no stitches;
//   3. a lane per stitch: centroid + extents or the int-box fall-backs, width (two points to the plane), the +-N envelope
//      medians of the proximity test and of the edge, and the distance candidate (two more points);
//   4. row selection: 2-means on one lane with the cluster means recomputed from the returned labels, or the median split;
//   5. the final set (proximity, or the selected row when nothing is near), the ordered distance / width lists and their means.
struct MeasureArgs {
    CameraRow cam;                                                  // the one camera (TABLE = false)
    const CameraRow* table; const int* cam_of_frame; int n_cams;    // or a row per frame (TABLE = true)
    const long long* stats; const int* raw; const int* envelope;
    const float* dets; const float* xyxy; const int* counts; const int* offsets;
    int max_det, row, capacity, H0, W0;
    const FrameRow* frames;                                         // per-frame H0, W0 (then W0 above is the envelope pitch), or nullptr
    double* frame_f64; int* frame_i32; double* stitch_f64; int* stitch_i32;
};

// Exclusive rank of this thread's flag among the workgroup's (256 threads, thread order) and the total.
__device__ __forceinline__ int block_rank(bool f, int* s_cnt, int& total) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(f);
    if (lane == 0) s_cnt[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { const int c = s_cnt[k]; off += k < w ? c : 0; total += c; }
    __syncthreads();
    return off + __popcll(m & ((1ull << lane) - 1ull));
}

// np.median of [env[clip(c + dx, 0, W0 - 1)] for |dx| <= nb if >= 0] (measurement.py:413-418, 441-445): false when empty.  At most
// 2 nb + 1 values: the order statistics by counting (ties broken by position), no sort.
__device__ bool env_median(const int* env, int W0, int c, int nb, double& med) {
    int k = 0;
    for (int dx = -nb; dx <= nb; ++dx) k += env[min(max(c + dx, 0), W0 - 1)] >= 0;
    if (!k) return false;
    const int q0 = (k - 1) >> 1, q1 = k >> 1;      // the two middle ranks (equal for odd k)
    int v0 = 0, v1 = 0;
    for (int a = -nb; a <= nb; ++a) {
        const int va = env[min(max(c + a, 0), W0 - 1)];
        if (va < 0) continue;
        int r = 0;
        for (int dx = -nb; dx <= nb; ++dx) {
            const int v = env[min(max(c + dx, 0), W0 - 1)];
            r += v >= 0 && (v < va || (v == va && dx < a));
        }
        if (r == q0) v0 = va;
        if (r == q1) v1 = va;
    }
    med = (k & 1) ? (double)v1 : ((double)v0 + (double)v1) / 2.0;
    return true;
}

__device__ __forceinline__ double dist_mm(const double* p, const double* q) {
    const double d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
    return sqrt((d0 * d0 + d1 * d1) + d2 * d2) * 1000.0;
}

enum { F_FINAL = 64, F_CAND = 128 };   // kernel-internal flag bits (final set, distance computable), above the VTI_STITCH_* bits

// TABLE: the frame's settings are row cam_of_frame[b] of the camera table, copied once before anything is stored;
// otherwise the row in the launch arguments.  Either way the arithmetic below sees the same values in the same order.
template <bool TABLE>
__global__ __launch_bounds__(256) void measure_frames_kernel(MeasureArgs a) {
    extern __shared__ double msm[];        // M = max_det: cy | width | dist | edge | g0 | g1 (f64), then idx | flags | lab0 | lab1 (i32)
    const int M = a.max_det;
    double* s_cy = msm; double* s_wd = s_cy + M; double* s_ds = s_wd + M; double* s_ed = s_ds + M; double* g0 = s_ed + M; double* g1 = g0 + M;
    int* s_idx = (int*)(g1 + M); int* s_fl = s_idx + M; int* lab0 = s_fl + M; int* lab1 = lab0 + M;
    __shared__ int s_cnt[4];
    __shared__ long long s_es[4];
    __shared__ int s_ec[4], s_pick[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const int* env = a.envelope + (size_t)b * a.W0;
    const double NaN = __builtin_nan("");
    const int H0 = a.frames ? a.frames[b].H0 : a.H0, W0 = a.frames ? a.frames[b].W0 : a.W0;
    int ci = 0;
    if (TABLE) {
        ci = a.cam_of_frame[b];
        if (ci < 0 || ci >= a.n_cams) {         // uniform over the workgroup; no table address has been formed
            for (int i = tid; i < n; i += 256) {
                const int s = s0 + i;
                if (s < 0 || s >= a.capacity) continue;
                if (a.stitch_f64) for (int k = 0; k < 7; ++k) a.stitch_f64[(size_t)s * 7 + k] = NaN;
                if (a.stitch_i32) { a.stitch_i32[(size_t)s * 2] = 0; a.stitch_i32[(size_t)s * 2 + 1] = -1; }
            }
            if (tid == 0) {
                a.frame_f64[2 * b] = NaN; a.frame_f64[2 * b + 1] = NaN;
                int* o = a.frame_i32 + 6 * b;
                o[0] = VTI_MEASURE_BAD_CAMERA; o[1] = o[2] = o[3] = o[4] = o[5] = 0;
            }
            return;
        }
    }
    const CameraRow r = TABLE ? a.table[ci] : a.cam;
    int4 roi;
    const bool roi_on = roi_clamp(r.roi_enabled, r.roi, H0, W0, roi);

    // 1. stitch list and fabric count (measurement.py:248-273)
    int n_st = 0, n_fab = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid, s = s0 + i;
        bool st = false, fab = false;
        if (i < n) {
            const bool live = s >= 0 && s < a.capacity;
            const long long m00 = live ? a.stats[(size_t)s * 5] : 0;
            const bool raw = live && (a.raw ? a.raw[s] != 0 : m00 > 0);
            const size_t di = (size_t)b * M + i;
            const int cls = (int)a.dets[di * a.row + 5];
            const bool keep = (!r.drop_empty || raw) && (!roi_on || roi_keeps(a.xyxy + di * 4, roi));
            st = keep && cls == r.stitch_id;
            fab = keep && cls == r.fabric_id && m00 > 0;
            if (!st && live) {
                if (a.stitch_f64) for (int k = 0; k < 7; ++k) a.stitch_f64[(size_t)s * 7 + k] = NaN;
                if (a.stitch_i32) { a.stitch_i32[(size_t)s * 2] = 0; a.stitch_i32[(size_t)s * 2 + 1] = -1; }
            }
        }
        int tot_st, tot_fab;
        const int pos = block_rank(st, s_cnt, tot_st);
        if (st) s_idx[n_st + pos] = i;
        (void)block_rank(fab, s_cnt, tot_fab);
        n_st += tot_st; n_fab += tot_fab;
    }
    // 2. the envelope's valid columns (their mean is fabric_mean_y, measurement.py:390-392: integer sum, exact)
    long long es = 0;
    int ec = 0;
    for (int x = tid; x < W0; x += 256) { const int v = env[x]; if (v >= 0) { es += v; ++ec; } }
    for (int o = 32; o > 0; o >>= 1) { es += __shfl_down(es, o); ec += __shfl_down(ec, o); }
    if ((tid & 63) == 0) { s_es[tid >> 6] = es; s_ec[tid >> 6] = ec; }
    __syncthreads();                        // also publishes s_idx
    es = (s_es[0] + s_es[1]) + (s_es[2] + s_es[3]);
    ec = (s_ec[0] + s_ec[1]) + (s_ec[2] + s_ec[3]);
    const int status = (n_fab == 0 || ec == 0) ? VTI_MEASURE_NO_FABRIC : (n_st == 0 ? VTI_MEASURE_NO_STITCHES : VTI_MEASURE_OK);

    // 3. per stitch (measurement.py:300-368, 408-420, 436-459)
    for (int j = tid; j < n_st; j += 256) {
        const int i = s_idx[j], s = s0 + i;
        const bool live = s >= 0 && s < a.capacity;
        const float* bx = a.xyxy + ((size_t)b * M + i) * 4;
        const int x1 = (int)bx[0], y1 = (int)bx[1], x2 = (int)bx[2], y2 = (int)bx[3];
        double cx, cy, left, right;
        int fl = VTI_STITCH_KEPT;
        const long long* m = a.stats + (size_t)s * 5;
        if (live && m[0] > 0) {
            fl |= VTI_STITCH_MASK;
            cx = (double)m[1] / (double)m[0]; cy = (double)m[2] / (double)m[0];
            left = (double)m[3]; right = (double)m[4];
        } else {
            cx = (double)((long long)x1 + x2) / 2.0; cy = (double)((long long)y1 + y2) / 2.0;
            left = (double)x1; right = (double)x2;
        }
        double wd = NaN, ds = NaN, ed = NaN;
        if (status == VTI_MEASURE_OK) {
            double pl[3], pr[3];
            const bool okl = pixel_to_world(r.g, left, cy, pl), okr = pixel_to_world(r.g, right, cy, pr);
            if (okl && okr) { wd = dist_mm(pr, pl); fl |= VTI_STITCH_WIDTH; }
            const int c = (int)rint(cx);                                   // python round(): half to even
            double med;
            if (env_median(env, W0, c, r.nb, med) && fabs(cy - rint(med)) < r.max_px) fl |= VTI_STITCH_NEAR;
            if (env_median(env, W0, min(max(c, 0), W0 - 1), r.nb, med)) {
                ed = med;
                double ps[3], pe[3];
                const bool oks = pixel_to_world(r.g, cx, cy, ps), oke = pixel_to_world(r.g, cx, ed, pe);
                if (oks && oke) { ds = dist_mm(ps, pe); fl |= F_CAND; }
            }
        }
        s_cy[j] = cy; s_wd[j] = wd; s_ds[j] = ds; s_ed[j] = ed; s_fl[j] = fl;
        lab0[j] = 0;
        if (live && a.stitch_f64) {
            double* o = a.stitch_f64 + (size_t)s * 7;
            o[0] = cx; o[1] = cy; o[2] = left; o[3] = right;
        }
    }
    __syncthreads();

    // 4. row selection (measurement.py:370-406)
    if (status == VTI_MEASURE_OK) {
        if (n_st >= 2 && r.skip_cluster) {
            for (int j = tid; j < n_st; j += 256) {                        // ranks -> the sorted centroids, in g0
                const double v = s_cy[j];
                int r = 0;
                for (int k = 0; k < n_st; ++k) r += s_cy[k] < v || (s_cy[k] == v && k < j);
                g0[r] = v;
            }
            __syncthreads();
            const double med = (n_st & 1) ? g0[n_st >> 1] : (g0[(n_st >> 1) - 1] + g0[n_st >> 1]) / 2.0;
            const bool two = g0[n_st - 1] - g0[0] > r.two_row;
            for (int j = tid; j < n_st; j += 256)
                if (!two || s_cy[j] >= med) s_fl[j] |= VTI_STITCH_SELECTED;
        } else if (n_st >= 2) {
            if (tid == 0) {
                double c0, c1;
                const int which = kmeans1d2_serial(s_cy, n_st, r.kmeans_iters, lab0, lab1, g0, g1, c0, c1);
                const int* L = which ? lab1 : lab0;
                int k0 = 0, k1 = 0;
                for (int j = 0; j < n_st; ++j) { if (L[j]) g1[k1++] = s_cy[j]; else g0[k0++] = s_cy[j]; }
                const double f = (double)es / (double)ec;
                const double m0 = k0 ? np_pairwise_sum(g0, k0) / (double)k0 : 1e9, m1 = k1 ? np_pairwise_sum(g1, k1) / (double)k1 : 1e9;
                s_pick[0] = fabs(m0 - f) < fabs(m1 - f) ? 0 : 1;
                s_pick[1] = which;
            }
            __syncthreads();
            const int* L = s_pick[1] ? lab1 : lab0;
            for (int j = tid; j < n_st; j += 256)
                if (L[j] == s_pick[0]) s_fl[j] |= VTI_STITCH_SELECTED;
        } else {
            for (int j = tid; j < n_st; j += 256) s_fl[j] |= VTI_STITCH_SELECTED;
        }
        __syncthreads();
        // 5. final set (measurement.py:408-431): the selected stitches near the envelope, else all selected ones
        bool near = false;
        for (int j = tid; j < n_st; j += 256)
            near |= (s_fl[j] & (VTI_STITCH_SELECTED | VTI_STITCH_NEAR)) == (VTI_STITCH_SELECTED | VTI_STITCH_NEAR);
        near = __syncthreads_or(near);
        for (int j = tid; j < n_st; j += 256) {
            int fl = s_fl[j];
            if ((fl & VTI_STITCH_SELECTED) && (!near || (fl & VTI_STITCH_NEAR))) {
                fl |= F_FINAL;
                if (fl & F_CAND) fl |= VTI_STITCH_DIST;
            }
            s_fl[j] = fl;
        }
        __syncthreads();
    }
    // ordered lists of the distances and widths (measurement.py:433-468) into g0 / g1
    int n_d = 0, n_w = 0, n_sel = 0;
    for (int c0 = 0; c0 < n_st; c0 += 256) {
        const int j = c0 + tid;
        const int fl = j < n_st ? s_fl[j] : 0;
        int td, tw, ts;
        const bool fd = fl & VTI_STITCH_DIST, fw = fl & VTI_STITCH_WIDTH;
        const int pd = block_rank(fd, s_cnt, td);
        if (fd) g0[n_d + pd] = s_ds[j];
        const int pw = block_rank(fw, s_cnt, tw);
        if (fw) g1[n_w + pw] = s_wd[j];
        (void)block_rank(fl & VTI_STITCH_SELECTED, s_cnt, ts);
        n_d += td; n_w += tw; n_sel += ts;
        if (j < n_st) {
            const int s = s0 + s_idx[j];
            if (s >= 0 && s < a.capacity) {
                if (a.stitch_f64) {
                    double* o = a.stitch_f64 + (size_t)s * 7;
                    o[4] = s_wd[j]; o[5] = (fl & F_FINAL) ? s_ed[j] : NaN; o[6] = (fl & VTI_STITCH_DIST) ? s_ds[j] : NaN;
                }
                if (a.stitch_i32) { a.stitch_i32[(size_t)s * 2] = fl & 63; a.stitch_i32[(size_t)s * 2 + 1] = j; }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.frame_f64[2 * b] = n_d >= r.min_stitches ? np_pairwise_sum(g0, n_d) / (double)n_d : NaN;      // measurement.py:469-472
        a.frame_f64[2 * b + 1] = n_w >= r.min_stitches ? np_pairwise_sum(g1, n_w) / (double)n_w : NaN;
        int* o = a.frame_i32 + 6 * b;
        o[0] = status; o[1] = n_st; o[2] = n_fab; o[3] = n_sel; o[4] = n_d; o[5] = n_w;
    }
}

void measure_scratch_layout(int B, int capacity, int W0, size_t off[3], size_t& total) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    off[0] = 0;
    off[1] = up((size_t)capacity * 5 * sizeof(long long));
    off[2] = off[1] + up((size_t)capacity * sizeof(int));
    total = off[2] + up((size_t)B * W0 * sizeof(int));
}

size_t measure_camera_row_bytes() { return sizeof(CameraRow); }

// One validated vti_measure_params -> one table row (host).
void measure_pack_camera(const vti_measure_params& p, void* row) {
    CameraRow c;
    memset(&c, 0, sizeof c);
    c.g = make_geom(p.K, p.dist, p.R, p.t);
    c.max_px = p.max_px_distance; c.two_row = p.two_row_threshold_px;
    c.stitch_id = p.stitch_id; c.fabric_id = p.fabric_id; c.roi_enabled = p.roi_enabled ? 1 : 0;
    for (int k = 0; k < 4; ++k) c.roi[k] = p.roi[k];
    c.min_stitches = p.min_stitches; c.nb = p.envelope_neighborhood; c.skip_cluster = p.skip_cluster;
    c.kmeans_iters = p.kmeans_iters; c.drop_empty = p.drop_empty;
    memcpy(row, &c, sizeof c);
}

// ---- what launch_measure and launch_measure_checker do alike -----------------------------------------------------------------------
// The scratch carved as measure_scratch_layout, and the per-slot moments (and, for letterbox slots, the raw emptiness) launched into it.
// o.bases is dropped unless the masks are the ragged rows (frame table and native).
struct MeasureScratch { long long* stats; int* raw; int* env; };
static int native_words_per_row(int W0) { return 2 * ((W0 + 63) / 64); }       // 32-bit words of a frame-size mask row
static hipError_t measure_front(OutputSet& o, const Canvas& cv, const FrameSizes& fs, void* scratch, hipStream_t st, MeasureScratch& s) {
    const int H = cv.H, W = cv.W, H0 = fs.H0, W0 = fs.W0, B = o.B;
    const FrameRow* frames = fs.rows;
    if (frames && o.native && (!o.bases || o.capacity_bytes < 0)) return hipErrorInvalidValue;
    if (!(frames && o.native)) o.bases = nullptr;
    size_t off[3], total;
    measure_scratch_layout(B, o.capacity, W0, off, total);
    s.stats = (long long*)((char*)scratch + off[0]);
    s.raw = (int*)((char*)scratch + off[1]);
    s.env = (int*)((char*)scratch + off[2]);
    if (o.capacity == 0) return hipSuccess;
    const unsigned* masks = (const unsigned*)o.masks;
    const int* n_live = o.offsets + B;
    if (o.native && frames) {   // the ragged frame-size rows: H0, W0 and the words per row of the slot's own frame
        hipLaunchKernelGGL((mask_stats_bits_kernel<2, false, true, true>), dim3(o.capacity), dim3(256), 0, st, masks, n_live,
                           0, 0, 0, 0, s.stats, (int*)nullptr, o.offsets, frames, B, o.bases, o.capacity_bytes);
    } else if (o.native) {      // frame-size rows: the identity branch (H0 = H, W0 = W = 32 * wpr; the pad bits are 0), no tables
        const int wpr = native_words_per_row(W0);
        hipLaunchKernelGGL((mask_stats_bits_kernel<2, false>), dim3(o.capacity), dim3(256), 0, st, masks, n_live, H0,
                           32 * wpr, H0, 32 * wpr, s.stats, (int*)nullptr, (const int*)nullptr, (const FrameRow*)nullptr, 0);
    } else {
        if ((W & 31) || (H & 31) || ((uintptr_t)masks & 15) || (size_t)(4 * W + 2 * H) * 4 > 60 * 1024) return hipErrorInvalidValue;
        if (frames)
            hipLaunchKernelGGL((mask_stats_bits_kernel<4, true, true>), dim3(o.capacity), dim3(256), (size_t)(4 * W + 2 * H) * 4, st,
                               masks, n_live, H, W, H0, W0, s.stats, s.raw, o.offsets, frames, B);
        else
            hipLaunchKernelGGL((mask_stats_bits_kernel<4, true>), dim3(o.capacity), dim3(256), (size_t)(4 * W + 2 * H) * 4, st,
                               masks, n_live, H, W, H0, W0, s.stats, s.raw, (const int*)nullptr,
                               (const FrameRow*)nullptr, 0);
    }
    return hipGetLastError();
}

// The fields MeasureArgs and CheckerArgs have in common (everything but the one camera's row and CheckerArgs' ragged part).
template <class Args>
static void measure_fill(Args& a, const CameraChoice& cams, const OutputSet& o, const Canvas& cv, const FrameSizes& fs,
                         const MeasureResult& r, const MeasureScratch& s) {
    a.table = (const CameraRow*)cams.table; a.cam_of_frame = cams.cam_of_frame; a.n_cams = cams.n_cams;
    a.stats = s.stats; a.raw = o.native ? nullptr : s.raw; a.envelope = s.env;
    a.dets = o.dets; a.xyxy = o.xyxy; a.counts = o.counts; a.offsets = o.offsets;
    a.max_det = o.max_det; a.row = 6 + cv.nm; a.capacity = o.capacity; a.H0 = fs.H0; a.W0 = fs.W0; a.frames = fs.rows;
    a.frame_f64 = r.frame_f64; a.frame_i32 = r.frame_i32; a.stitch_f64 = r.stitch_f64; a.stitch_i32 = r.stitch_i32;
}

// p: the one camera (vti_measure), or nullptr with a device table of n_cams rows and the frames' indices (vti_measure_cameras).
hipError_t launch_measure(const vti_measure_params* p, const CameraChoice& cams, OutputSet o, const Canvas& cv, const FrameSizes& fs,
                          const MeasureResult& r, hipStream_t st) {
    if (o.B == 0) return hipSuccess;
    MeasureScratch s;
    hipError_t e = measure_front(o, cv, fs, r.scratch, st, s);
    if (e != hipSuccess) return e;
    MeasureArgs a;
    memset(&a, 0, sizeof a);
    if (p) measure_pack_camera(*p, &a.cam);
    measure_fill(a, p ? CameraChoice{} : cams, o, cv, fs, r, s);
    const EnvSel sel = {a.cam.fabric_id, a.cam.roi_enabled, {a.cam.roi[0], a.cam.roi[1], a.cam.roi[2], a.cam.roi[3]}};
    const unsigned* masks = (const unsigned*)o.masks;
    const dim3 egrid((fs.W0 + 63) / 64, o.B);
    if (o.native)
        hipLaunchKernelGGL(envelope_bits_kernel<true>, egrid, dim3(256), 0, st, masks, o.offsets, o.dets, o.max_det, a.row, o.capacity, sel,
                           fs.H0, fs.W0, fs.H0, fs.W0, s.env, o.xyxy, native_words_per_row(fs.W0), a.table, a.cam_of_frame, a.n_cams,
                           fs.rows, o.bases, o.capacity_bytes);
    else {
        if ((size_t)cv.H * 4 > 60 * 1024) return hipErrorInvalidValue;
        hipLaunchKernelGGL(envelope_bits_kernel<false>, egrid, dim3(256), (size_t)cv.H * 4, st, masks, o.offsets, o.dets, o.max_det, a.row,
                           o.capacity, sel, cv.H, cv.W, fs.H0, fs.W0, s.env, o.xyxy, 0, a.table, a.cam_of_frame, a.n_cams, fs.rows);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds = (size_t)o.max_det * (6 * sizeof(double) + 4 * sizeof(int));
    if (a.table) hipLaunchKernelGGL(measure_frames_kernel<true>, dim3(o.B), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(measure_frames_kernel<false>, dim3(o.B), dim3(256), lds, st, a);
    return hipGetLastError();
}

// ---- the stitch-distance checker's record (Utils/check_stitch_distance.py:281-553), batched ----------------------------------------
// The bench tool measures against the UPPER fabric edge and keeps another set of stitches than process_frame does; what differs:
//   * no ROI; every kept fabric-class instance joins the union, with its mask if the frame-size mask has a set pixel, else with the
//     filled rectangle of its int-truncated box, corners inclusive (:329-334);
//   * envelope[x] = the SMALLEST set row of column x (:238-251);
//   * rows: 2-means with the labels of the last assignment (kmeans1d2_serial<true>), the cluster whose mean is nearer to the mean
//     envelope row (strict <, so a tie is label 1); skip_cluster or a single stitch: every stitch (:408-429);
//   * proximity: 0 < cy - rint(median) < max_px, the stitch strictly below the edge (:431-444); nothing passes: the selected set;
//   * edge, distance and width for the final set only; a width whose end has no world point is estimated from the local scale,
//     px_width / 10 * |world(cx + 10, cy) - world(cx, cy)| (:465-507).
// Same inputs, scratch and output layout as vti_measure.

// A4 + A5 + A6 for the checker: per frame the upper envelope of the union above.  yf[sy] = first frame row that maps to source row
// sy (INT_MAX: none), monotone in sy, so a column's answer from one mask is yf of its smallest set source row that has a frame row;
// a box contributes max(y1, 0) to the columns it covers: one more `min`.  Needs the per-slot stats (m00 decides mask or box) and,
// for letterbox slots, the raw emptiness (drop_empty), so it runs after mask_stats_bits_kernel.  The instance list is walked by
// index i < counts[b]: a slot at or beyond `capacity` is an empty mask, which still has a box.
// RIG (vti_measure_checker_cameras / _frames / _frames_native): fabric_id and drop_empty come from row cam_of_frame[b] of the camera
// table, range-checked against n_cams before the row's address is formed (a frame whose index is outside gets an all -1 envelope);
// with `frames`, H0 and W0 are frame b's, the W0 passed is the largest one (the pitch of the envelope rows, which the grid covers)
// and a workgroup past the frame's columns returns without writing, as in envelope_bits_kernel.  With `bases` too (NATIVE) the
// masks are the ragged rows of vti_masks_native_frames: 2 ceil(W0 / 64) words per row from bases[b] on, and the frame's live slots
// are those that end at or before capacity_bytes; a later one is what a slot at or beyond `capacity` is, an empty mask with a box.
// Without RIG none of this is compiled in.
template <bool NATIVE, bool RIG = false>
__global__ __launch_bounds__(256) void upper_envelope_bits_kernel(const unsigned* __restrict__ bits, const int* __restrict__ offsets,
                                                                  const int* __restrict__ counts, const float* __restrict__ dets,
                                                                  int max_det, int row, int capacity, int cls, int drop_empty, int H,
                                                                  int W, int H0, int W0, const long long* __restrict__ stats,
                                                                  const int* __restrict__ raw, const float* __restrict__ xyxy,
                                                                  int native_wpr, int* __restrict__ envelope,
                                                                  const CameraRow* __restrict__ table = nullptr,
                                                                  const int* __restrict__ cam_of_frame = nullptr, int n_cams = 0,
                                                                  const FrameRow* __restrict__ frames = nullptr,
                                                                  const long long* __restrict__ bases = nullptr,
                                                                  long long capacity_bytes = 0) {
    extern __shared__ int yf[];             // [H] (not NATIVE)
    __shared__ int red[4][64];
    __shared__ int s_sel[256][5];           // slot (-1: a box), first row, last row, first column, last column
    __shared__ int s_nsel;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int pitch = W0;                   // of the envelope rows: W0, or the largest W0 of a frame table
    if (RIG) {
        if (frames) {
            H0 = frames[b].H0; W0 = frames[b].W0;
            if ((int)blockIdx.x * 64 >= W0) return;             // columns this frame does not have: nothing is written
        }
        const int ci = cam_of_frame[b];
        if (ci < 0 || ci >= n_cams) {                           // uniform over the workgroup
            const int xo = blockIdx.x * 64 + tid;
            if (tid < 64 && xo < W0) envelope[(size_t)b * pitch + xo] = -1;
            return;
        }
        cls = table[ci].fabric_id; drop_empty = table[ci].drop_empty;
    }
    if (!NATIVE) {
        for (int i = tid; i < H; i += 256) yf[i] = INT_MAX;
        __syncthreads();
        const double ify = 1.0 / ((double)H0 / (double)H);
        for (int y = tid; y < H0; y += 256) atomicMin(&yf[nn_src(y, ify, H)], y);
        __syncthreads();
    }
    const int x = blockIdx.x * 64 + (tid & 63), rg = tid >> 6;
    const int xc = x < W0 ? x : W0 - 1;
    const int sx = NATIVE ? xc : nn_src(xc, 1.0 / ((double)W0 / (double)W), W);
    const bool ragged = RIG && NATIVE && bases;
    const int wpr = NATIVE ? (ragged ? 2 * ((W0 + 63) / 64) : native_wpr) : W >> 5;
    const int Hm = NATIVE ? H0 : H;         // rows of a mask slot
    const int s0 = offsets[b], n = min(max(counts[b], 0), max_det);
    int srel = 0;                           // `bits` is where slot `srel` starts
    if (ragged) {                           // the instances whose slot ends at or before capacity_bytes; none if the base is no offset
        const long long base = bases[b], slot_bytes = (long long)Hm * wpr * 4;
        const long long fit = base >= 0 && !(base & 7) && capacity_bytes > base ? (capacity_bytes - base) / slot_bytes : 0;
        capacity = (int)min((long long)capacity, (long long)s0 + fit);
        if (fit > 0) bits += base >> 2;
        srel = s0;
    }
    int env = INT_MAX;
    for (int i0 = 0; i0 < n; i0 += 256) {
        __syncthreads();                                       // the previous round's list has been consumed
        if (tid == 0) s_nsel = 0;
        __syncthreads();
        const int i = i0 + tid, s = s0 + i;
        if (i < n) {
            const size_t di = (size_t)b * max_det + i;
            const float* d = dets + di * row;
            const bool live = s >= 0 && s < capacity;
            const long long m00 = live ? stats[(size_t)s * 5] : 0;
            const bool nonempty = live && (raw ? raw[s] != 0 : m00 > 0);
            if ((int)d[5] == cls && (!drop_empty || nonempty)) {
                const float* bx = xyxy + di * 4;
                int e0, e1, e2, e3, e4;
                if (m00 > 0) {
                    if (NATIVE) { e1 = (int)floorf(bx[1]); e2 = (int)ceilf(bx[3]); }
                    else { e1 = (int)floorf(d[1] - 8.f); e2 = (int)ceilf(d[3] + 8.f); }
                    e0 = s; e1 = max(e1, 0); e2 = min(e2, Hm - 1); e3 = 0; e4 = W0 - 1;
                } else {                                        // cv2.rectangle(tmp, (x1i, y1i), (x2i, y2i), 1, -1), clipped to the frame
                    const int x1 = (int)bx[0], y1 = (int)bx[1], x2 = (int)bx[2], y2 = (int)bx[3];
                    e0 = -1; e1 = max(min(y1, y2), 0); e2 = min(max(y1, y2), H0 - 1); e3 = max(min(x1, x2), 0); e4 = min(max(x1, x2), W0 - 1);
                }
                if (e1 <= e2 && e3 <= e4) {
                    const int pos = atomicAdd(&s_nsel, 1);
                    s_sel[pos][0] = e0; s_sel[pos][1] = e1; s_sel[pos][2] = e2; s_sel[pos][3] = e3; s_sel[pos][4] = e4;
                }
            }
        }
        __syncthreads();
        const int nsel = s_nsel;
        for (int j = 0; j < nsel; ++j) {
            const int s = s_sel[j][0], ya = s_sel[j][1], yb = s_sel[j][2];
            if (s < 0) {
                if (xc >= s_sel[j][3] && xc <= s_sel[j][4]) env = min(env, ya);
                continue;
            }
            const unsigned* m = bits + (size_t)(s - srel) * Hm * wpr + (sx >> 5);
            for (int sy = ya + rg; sy <= yb && (!NATIVE || sy < env); sy += 4) {    // top first: a lane's first hit is its smallest
                if ((m[(size_t)sy * wpr] >> (sx & 31)) & 1u) {
                    const int y = NATIVE ? sy : yf[sy];
                    if (y != INT_MAX) { env = min(env, y); break; }
                }
            }
        }
    }
    red[rg][tid & 63] = env;
    __syncthreads();
    if (rg == 0 && x < W0) {
        const int e = min(min(red[0][tid], red[1][tid]), min(red[2][tid], red[3][tid]));
        envelope[(size_t)b * pitch + x] = e == INT_MAX ? -1 : e;
    }
}

struct CheckerArgs {
    CameraRow cam;                                                  // the geometry and the settings the checker has (no ROI, no two_row)
    const long long* stats; const int* raw; const int* envelope;
    const float* dets; const float* xyxy; const int* counts; const int* offsets;
    int max_det, row, capacity, H0, W0;
    double* frame_f64; int* frame_i32; double* stitch_f64; int* stitch_i32;
    // the rig forms (checker_frames_kernel<true>): a.cam unused, the row is table[cam_of_frame[b]]
    const CameraRow* table; const int* cam_of_frame; int n_cams;
    const FrameRow* frames;                                         // per-frame H0, W0 (then W0 above is the envelope pitch), or nullptr
    const long long* bases; long long capacity_bytes;               // the ragged native rows (with frames), or nullptr
};

// Centroid and column extent of instance i of frame b (:365-391): the mask's moments and extent, else the int box.  true: from the mask.
// cap: the frame's first slot that is not live.
__device__ __forceinline__ bool checker_stitch_geometry(const CheckerArgs& a, int cap, int b, int i, int s, double& cx, double& cy,
                                                        double& left, double& right) {
    const long long* m = a.stats + (size_t)s * 5;
    if (s >= 0 && s < cap && m[0] > 0) {
        cx = (double)m[1] / (double)m[0]; cy = (double)m[2] / (double)m[0];
        left = (double)m[3]; right = (double)m[4];
        return true;
    }
    const float* bx = a.xyxy + ((size_t)b * a.max_det + i) * 4;
    const int x1 = (int)bx[0], y1 = (int)bx[1], x2 = (int)bx[2], y2 = (int)bx[3];
    cx = (double)((long long)x1 + x2) / 2.0; cy = (double)((long long)y1 + y2) / 2.0;
    left = (double)x1; right = (double)x2;
    return false;
}

// One workgroup per frame, as measure_frames_kernel: 1. stitch list and fabric count, 2. status, 3. centroids and the proximity
// flag, 4. row selection, 5. the final set, 6. a lane per final stitch: edge, distance, width, 7. the ordered lists and their means.
// TABLE: the frame's settings are row cam_of_frame[b] of the camera table, copied once before anything is stored (an index outside
// the table leaves by measure_frames_kernel's BAD_CAMERA path); W0 and the ragged rows' live slots per frame as in
// upper_envelope_bits_kernel.  Otherwise the row in the launch arguments and one size.  Either way the arithmetic below sees the
// same values in the same order.
template <bool TABLE>
__global__ __launch_bounds__(256) void checker_frames_kernel(CheckerArgs a) {
    extern __shared__ double csm[];        // M = max_det: cy | width | dist | g0 | g1 (f64), then idx | flags | lab0 | lab1 (i32)
    const int M = a.max_det;
    double* s_cy = csm; double* s_wd = s_cy + M; double* s_ds = s_wd + M; double* g0 = s_ds + M; double* g1 = g0 + M;
    int* s_idx = (int*)(g1 + M); int* s_fl = s_idx + M; int* lab0 = s_fl + M; int* lab1 = lab0 + M;
    __shared__ int s_cnt[4];
    __shared__ long long s_es[4];
    __shared__ int s_ec[4], s_pick[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const int* env = a.envelope + (size_t)b * a.W0;
    const double NaN = __builtin_nan("");
    int W0 = a.W0, cap = a.capacity;
    CameraRow row_b;
    if (TABLE) {
        if (a.frames) {
            W0 = a.frames[b].W0;
            if (a.bases) {                      // the ragged rows: the slots that end at or before capacity_bytes are live
                const long long base = a.bases[b], slot_bytes = (long long)a.frames[b].H0 * (2 * ((W0 + 63) / 64)) * 4;
                const long long fit = base >= 0 && !(base & 7) && a.capacity_bytes > base ? (a.capacity_bytes - base) / slot_bytes : 0;
                cap = (int)min((long long)cap, (long long)s0 + fit);
            }
        }
        const int ci = a.cam_of_frame[b];
        if (ci < 0 || ci >= a.n_cams) {         // uniform over the workgroup; no table address has been formed
            for (int i = tid; i < n; i += 256) {
                const int s = s0 + i;
                if (s < 0 || s >= cap) continue;
                if (a.stitch_f64) for (int k = 0; k < 7; ++k) a.stitch_f64[(size_t)s * 7 + k] = NaN;
                if (a.stitch_i32) { a.stitch_i32[(size_t)s * 2] = 0; a.stitch_i32[(size_t)s * 2 + 1] = -1; }
            }
            if (tid == 0) {
                a.frame_f64[2 * b] = NaN; a.frame_f64[2 * b + 1] = NaN;
                int* o = a.frame_i32 + 6 * b;
                o[0] = VTI_MEASURE_BAD_CAMERA; o[1] = o[2] = o[3] = o[4] = o[5] = 0;
            }
            return;
        }
        row_b = a.table[ci];
    }
    const CameraRow& r = TABLE ? row_b : a.cam;

    // 1. stitch list and fabric count (:310-336)
    int n_st = 0, n_fab = 0;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + tid, s = s0 + i;
        bool st = false, fab = false;
        if (i < n) {
            const bool live = s >= 0 && s < cap;
            const bool raw = live && (a.raw ? a.raw[s] != 0 : a.stats[(size_t)s * 5] > 0);
            const int cls = (int)a.dets[((size_t)b * M + i) * a.row + 5];
            const bool keep = !r.drop_empty || raw;
            st = keep && cls == r.stitch_id;
            fab = keep && cls == r.fabric_id;
            if (!st && live) {
                if (a.stitch_f64) for (int k = 0; k < 7; ++k) a.stitch_f64[(size_t)s * 7 + k] = NaN;
                if (a.stitch_i32) { a.stitch_i32[(size_t)s * 2] = 0; a.stitch_i32[(size_t)s * 2 + 1] = -1; }
            }
        }
        int tot_st, tot_fab;
        const int pos = block_rank(st, s_cnt, tot_st);
        if (st) s_idx[n_st + pos] = i;
        (void)block_rank(fab, s_cnt, tot_fab);
        n_st += tot_st; n_fab += tot_fab;
    }
    // 2. the envelope's valid columns: none is an empty union (:345); their mean is fabric_mean_y (:414-416: integer sum, exact)
    long long es = 0;
    int ec = 0;
    for (int x = tid; x < W0; x += 256) { const int v = env[x]; if (v >= 0) { es += v; ++ec; } }
    for (int o = 32; o > 0; o >>= 1) { es += __shfl_down(es, o); ec += __shfl_down(ec, o); }
    if ((tid & 63) == 0) { s_es[tid >> 6] = es; s_ec[tid >> 6] = ec; }
    __syncthreads();                        // also publishes s_idx
    es = (s_es[0] + s_es[1]) + (s_es[2] + s_es[3]);
    ec = (s_ec[0] + s_ec[1]) + (s_ec[2] + s_ec[3]);
    const int status = ec == 0 ? VTI_MEASURE_NO_FABRIC : (n_st == 0 ? VTI_MEASURE_NO_STITCHES : VTI_MEASURE_OK);

    // 3. per stitch: centroid, extents (:365-402) and the signed proximity test (:433-444)
    for (int j = tid; j < n_st; j += 256) {
        const int i = s_idx[j], s = s0 + i;
        double cx, cy, left, right;
        int fl = VTI_STITCH_KEPT | (checker_stitch_geometry(a, cap, b, i, s, cx, cy, left, right) ? VTI_STITCH_MASK : 0);
        if (status == VTI_MEASURE_OK) {
            double med;
            if (env_median(env, W0, (int)rint(cx), r.nb, med)) {           // python round(): half to even; the centre is not clipped
                const double d = cy - rint(med);
                if (0.0 < d && d < r.max_px) fl |= VTI_STITCH_NEAR;
            }
        }
        s_cy[j] = cy; s_wd[j] = NaN; s_ds[j] = NaN; s_fl[j] = fl;
        lab0[j] = 0;
        if (s >= 0 && s < cap && a.stitch_f64) {
            double* o = a.stitch_f64 + (size_t)s * 7;
            o[0] = cx; o[1] = cy; o[2] = left; o[3] = right; o[4] = NaN; o[5] = NaN; o[6] = NaN;
        }
    }
    __syncthreads();

    if (status == VTI_MEASURE_OK) {
        // 4. row selection (:408-429)
        if (n_st >= 2 && !r.skip_cluster) {
            if (tid == 0) {
                double c0, c1;
                const int which = kmeans1d2_serial<true>(s_cy, n_st, r.kmeans_iters, lab0, lab1, g0, g1, c0, c1);
                const int* L = which ? lab1 : lab0;
                int k0 = 0, k1 = 0;
                for (int j = 0; j < n_st; ++j) { if (L[j]) g1[k1++] = s_cy[j]; else g0[k0++] = s_cy[j]; }
                const double f = (double)es / (double)ec;
                const double m0 = k0 ? np_pairwise_sum(g0, k0) / (double)k0 : 1e9, m1 = k1 ? np_pairwise_sum(g1, k1) / (double)k1 : 1e9;
                s_pick[0] = fabs(m0 - f) < fabs(m1 - f) ? 0 : 1;
                s_pick[1] = which;
            }
            __syncthreads();
            const int* L = s_pick[1] ? lab1 : lab0;
            for (int j = tid; j < n_st; j += 256)
                if (L[j] == s_pick[0]) s_fl[j] |= VTI_STITCH_SELECTED;
        } else {
            for (int j = tid; j < n_st; j += 256) s_fl[j] |= VTI_STITCH_SELECTED;
        }
        __syncthreads();
        // 5. final set (:431-454): the selected stitches below and near the edge, else all selected ones
        bool near = false;
        for (int j = tid; j < n_st; j += 256)
            near |= (s_fl[j] & (VTI_STITCH_SELECTED | VTI_STITCH_NEAR)) == (VTI_STITCH_SELECTED | VTI_STITCH_NEAR);
        near = __syncthreads_or(near);
        // 6. per final stitch (:465-507)
        for (int j = tid; j < n_st; j += 256) {
            int fl = s_fl[j];
            if (!((fl & VTI_STITCH_SELECTED) && (!near || (fl & VTI_STITCH_NEAR)))) continue;
            const int i = s_idx[j], s = s0 + i;
            double cx, cy, left, right, ed = NaN, ds = NaN, wd = NaN, med;
            (void)checker_stitch_geometry(a, cap, b, i, s, cx, cy, left, right);
            double pc[3];
            const bool okc = pixel_to_world(r.g, cx, cy, pc);
            if (env_median(env, W0, min(max((int)rint(cx), 0), W0 - 1), r.nb, med)) {
                ed = med;
                double pe[3];
                if (pixel_to_world(r.g, cx, ed, pe) && okc) { ds = dist_mm(pc, pe); fl |= VTI_STITCH_DIST; }
            }
            double pl[3], pr[3];
            const bool okl = pixel_to_world(r.g, left, cy, pl), okr = pixel_to_world(r.g, right, cy, pr);
            if (okl && okr) { wd = dist_mm(pr, pl); fl |= VTI_STITCH_WIDTH; }
            else if (okc && pixel_to_world(r.g, cx + 10.0, cy, pr)) {       // the local scale: mm per 10 px at the centroid
                wd = ((right - left) / 10.0) * dist_mm(pr, pc); fl |= VTI_STITCH_WIDTH;
            }
            s_wd[j] = wd; s_ds[j] = ds; s_fl[j] = fl;
            if (s >= 0 && s < cap && a.stitch_f64) {
                double* o = a.stitch_f64 + (size_t)s * 7;
                o[4] = wd; o[5] = ed; o[6] = ds;
            }
        }
        __syncthreads();
    }
    // 7. ordered lists of the distances and widths (per_dists, per_widths) into g0 / g1, and the averages (:515-517)
    int n_d = 0, n_w = 0, n_sel = 0;
    for (int c0 = 0; c0 < n_st; c0 += 256) {
        const int j = c0 + tid;
        const int fl = j < n_st ? s_fl[j] : 0;
        int td, tw, ts;
        const bool fd = fl & VTI_STITCH_DIST, fw = fl & VTI_STITCH_WIDTH;
        const int pd = block_rank(fd, s_cnt, td);
        if (fd) g0[n_d + pd] = s_ds[j];
        const int pw = block_rank(fw, s_cnt, tw);
        if (fw) g1[n_w + pw] = s_wd[j];
        (void)block_rank(fl & VTI_STITCH_SELECTED, s_cnt, ts);
        n_d += td; n_w += tw; n_sel += ts;
        if (j < n_st && a.stitch_i32) {
            const int s = s0 + s_idx[j];
            if (s >= 0 && s < cap) { a.stitch_i32[(size_t)s * 2] = fl & 63; a.stitch_i32[(size_t)s * 2 + 1] = j; }
        }
    }
    __syncthreads();
    if (tid == 0) {
        a.frame_f64[2 * b] = n_d >= r.min_stitches ? np_pairwise_sum(g0, n_d) / (double)n_d : NaN;
        a.frame_f64[2 * b + 1] = n_w >= r.min_stitches ? np_pairwise_sum(g1, n_w) / (double)n_w : NaN;
        int* o = a.frame_i32 + 6 * b;
        o[0] = status; o[1] = n_st; o[2] = n_fab; o[3] = n_sel; o[4] = n_d; o[5] = n_w;
    }
}

// One validated vti_checker_params -> the row the kernels read (host).
void checker_pack(const vti_checker_params& p, void* row) {
    CameraRow c;
    memset(&c, 0, sizeof c);
    c.g = make_geom(p.K, p.dist, p.R, p.t);
    c.max_px = p.max_px_distance;
    c.stitch_id = p.stitch_id; c.fabric_id = p.fabric_id;
    c.min_stitches = p.min_stitches; c.nb = p.envelope_neighborhood; c.skip_cluster = p.skip_cluster;
    c.kmeans_iters = p.kmeans_iters; c.drop_empty = p.drop_empty;
    memcpy(row, &c, sizeof c);
}

// p: the one camera (vti_measure_checker), or nullptr with a device table of n_cams rows and the frames' indices; the frame table
// and the ragged rows as launch_measure takes them.  The one-struct, one-size call launches the instantiations without RIG / TABLE.
hipError_t launch_measure_checker(const vti_checker_params* p, const CameraChoice& cams, OutputSet o, const Canvas& cv,
                                  const FrameSizes& fs, const MeasureResult& r, hipStream_t st) {
    if (o.B == 0) return hipSuccess;
    if (!p && (!cams.table || !cams.cam_of_frame)) return hipErrorInvalidValue;
    if (p && fs.rows) return hipErrorInvalidValue;
    const int H = cv.H, W = cv.W, H0 = fs.H0, W0 = fs.W0;
    if (!o.native && ((W & 31) || (H & 31) || (size_t)(4 * W + 2 * H) * 4 > 60 * 1024)) return hipErrorInvalidValue;
    MeasureScratch s;
    hipError_t e = measure_front(o, cv, fs, r.scratch, st, s);
    if (e != hipSuccess) return e;
    CheckerArgs a;
    memset(&a, 0, sizeof a);
    if (p) checker_pack(*p, &a.cam);
    measure_fill(a, p ? CameraChoice{} : cams, o, cv, fs, r, s);
    a.bases = o.bases; a.capacity_bytes = o.capacity_bytes;
    const unsigned* masks = (const unsigned*)o.masks;
    const int wpr = native_words_per_row(W0);
    const dim3 egrid((W0 + 63) / 64, o.B);
    if (o.native && p)
        hipLaunchKernelGGL(upper_envelope_bits_kernel<true>, egrid, dim3(256), 0, st, masks, o.offsets, o.counts, o.dets, o.max_det, a.row,
                           o.capacity, a.cam.fabric_id, a.cam.drop_empty, H0, W0, H0, W0, s.stats, (const int*)nullptr, o.xyxy, wpr, s.env);
    else if (p)
        hipLaunchKernelGGL(upper_envelope_bits_kernel<false>, egrid, dim3(256), (size_t)H * 4, st, masks, o.offsets, o.counts, o.dets,
                           o.max_det, a.row, o.capacity, a.cam.fabric_id, a.cam.drop_empty, H, W, H0, W0, s.stats, s.raw, o.xyxy, 0, s.env);
    else if (o.native)
        hipLaunchKernelGGL((upper_envelope_bits_kernel<true, true>), egrid, dim3(256), 0, st, masks, o.offsets, o.counts, o.dets,
                           o.max_det, a.row, o.capacity, 0, 0, H0, W0, H0, W0, s.stats, (const int*)nullptr, o.xyxy, wpr, s.env, a.table,
                           a.cam_of_frame, a.n_cams, fs.rows, o.bases, o.capacity_bytes);
    else
        hipLaunchKernelGGL((upper_envelope_bits_kernel<false, true>), egrid, dim3(256), (size_t)H * 4, st, masks, o.offsets, o.counts,
                           o.dets, o.max_det, a.row, o.capacity, 0, 0, H, W, H0, W0, s.stats, s.raw, o.xyxy, 0, s.env, a.table,
                           a.cam_of_frame, a.n_cams, fs.rows, (const long long*)nullptr, 0ll);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t lds = (size_t)o.max_det * (5 * sizeof(double) + 4 * sizeof(int));
    if (p) hipLaunchKernelGGL(checker_frames_kernel<false>, dim3(o.B), dim3(256), lds, st, a);
    else hipLaunchKernelGGL(checker_frames_kernel<true>, dim3(o.B), dim3(256), lds, st, a);
    return hipGetLastError();
}

}  // namespace vti
