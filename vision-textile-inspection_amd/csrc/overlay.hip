// The model-check viewer's picture on the device (vti_overlay): Utils/check_model.py:155-256 -- every instance's mask tinted in its
// class colour, its contours, its box and a filled label plate, blended 0.30 / 0.70 with OpenCV's rounding -- on a SELECTION of the
// batch's frames, byte for byte what the host restatement overlay.py gives (render(...)).  DESIGN.md section 5i.
//
// Three launches on the stream, ordered by the kernel boundaries only (no flags between workgroups):
//   1. owner (a thread per 32-bit word of a mask row; BLEND and BOTH): which instance tints a pixel is decided in MASK space -- the
//      frame bitmap of an instance is a pure nearest-neighbour lookup of its mask, so the last instance that covers frame pixel
//      (y, x) is the last one that covers mask pixel (nn(y), nn(x)) (native rows: the same pixel).  The instances are walked from the
//      last to the first, a word leaves the walk once all its 32 bits are owned, and what is kept per word is the owned bits and the
//      four bit planes of the owner's colour index.  The kernel also resets the frame's counters.
//   2. contours (16 workgroups per selected frame, each taking every 16th instance; DRAW and BOTH): the instance's bitmap at the
//      frame size as 64-bit-word rows (letterbox bits stretched as vti_mask_to_frame does, native rows as they are) in LDS -- or in
//      the workgroup's part of the scratch when H0 * ceil(W0/64) * 8 exceeds 156 KiB -- then vti_mask_polygons' labelling and border
//      following (polygons_dev.h).  Every vertex is stored with the index of the next one of its contour and its painter's key; the
//      frame's vertex count is one atomic counter.  More than max_points vertices (or a loop bound reached): none of the frame's
//      contours is drawn and the status word says so.
//   3. raster (a workgroup per 8192 consecutive pixels of an output frame): vti_annotate's tile scheme -- a word per pixel in LDS holds
//      the LAST record that covers it (atomicMax of record index << 4 | colour index; the fixed record order is, per instance,
//      contours, box, plate), a thread per box, plate or contour edge paints the rows of its primitive that fall into the tile --
//      and the tile's final copy applies tint and blend in the same pass (16 pixels = three 16-byte vectors per thread).
//
// vti_overlay_frames (frames of differing sizes) runs the FRAMES instantiations of the same kernels: a workgroup takes H0, W0, the
// words per bitmap row and the places of its frame in dev_frames and of its picture in dev_out / dev_annotated from the rows of the
// two frame tables (frame_geo), and with native masks the frame's slots from bases[b] on (frame_slots).  The scratch regions are then
// PITCHED by the largest selected frame (a frame uses the head of its slice; what lies beyond is never read), the grids of the owner
// and the raster kernel are those of the largest mask slot and the largest frame (workgroups past a frame's own extent leave before
// the first barrier), and the contour kernel is launched in both instantiations when the selection needs both: each leaves the frames
// of the other alone, by the frame's own size.  The uniform instantiations read nothing of this.
#include <climits>
#include <cstring>

#include "annotate_dev.h"
#include "measure_dev.h"
#include "overlay_dev.h"
#include "polygons_dev.h"

namespace vti {

namespace {

using poly::u64;

constexpr int kThreads = 256;
constexpr int kTile = 8192;                 // pixels per raster workgroup: 32 KB of LDS, a multiple of 16
constexpr int kContourGroups = 16;          // contour workgroups (labelling areas) per selected frame
constexpr int kPlaneWords = 8;              // per mask word: four colour-index bit planes | the owned bits | three unused words
enum { META_TOTAL = 0, META_BAD = 1, META_INTS = 16 };
enum { T_CONTOUR = 0, T_RECT = 1, T_PLATE = 2 };

struct OvlArgs {
    const uint8_t* frames; const uint8_t* annotated; uint8_t* out; int* status_out;
    const int* select; int B, n_sel, H0, W0, WW;                // FRAMES: the largest selected H0, W0 and their WW (pitches)
    const FrameRow* rows_in; const FrameRow* rows_out;          // FRAMES: the device frame tables of dev_frames (B rows) and dev_out (n_sel rows)
    const long long* bases; long long capacity_bytes;           // FRAMES, native: i64 [B + 1] and the bytes of the ragged mask buffer
    const uint8_t* masks; const float* dets; const float* xyxy; const int* counts; const int* offsets;
    int max_det, row, capacity, native, Hm, wpr, Wm;           // a mask slot: Hm rows of wpr 32-bit words, Wm real columns
    const int* plates;
    unsigned pal[12]; int n_colours;                            // 16 BGR triplets, packed
    float alpha, beta; int mode, max_points;
    int* meta; int4* cont; unsigned* planes; size_t plane_words;       // plane_words: per selected frame
    unsigned char* areas; size_t area_bytes, off_runs, off_rows, off_img; int groups;
};

__device__ __forceinline__ int clampc(int v) { return min(max(v, -32768), 32767); }

// colour j of the packed palette as b | g << 8 | r << 16: constant indices only, so the table stays in the argument registers
__device__ __forceinline__ unsigned palette_entry(const OvlArgs& a, int j) {
    unsigned v = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int bit = 24 * q, w = bit >> 5, s = bit & 31;
        unsigned c = a.pal[w] >> s;
        if (s > 8) c |= a.pal[(w + 1) < 12 ? w + 1 : 11] << (32 - s);
        if (q == j) v = c & 0xffffffu;
    }
    return v;
}

// build_color: cls % n_colours (Python's %: never negative)
__device__ __forceinline__ int colour_index(const OvlArgs& a, int b, int i) {
    const int cls = (int)a.dets[((size_t)b * a.max_det + i) * a.row + 5];
    const int m = cls % a.n_colours;
    return m < 0 ? m + a.n_colours : m;
}

// Picture k = frame b: its size, the shape of one of its mask slots (Hm rows of wpr 32-bit words, Wm real columns) and the byte
// offsets of the frame in dev_frames and of the picture in dev_out / dev_annotated -- the launch arguments, or the table rows (never
// above the pitches; the nearest-neighbour factors follow from H0, W0 by the expression the uniform call uses).
struct Geo { int H0, W0, WW, Hm, wpr, Wm; size_t in, out; };
template <bool FRAMES>
__device__ __forceinline__ Geo frame_geo(const OvlArgs& a, int k, int b) {
    if (!FRAMES) {
        const size_t px = (size_t)a.H0 * a.W0 * 3;
        return Geo{a.H0, a.W0, a.WW, a.Hm, a.wpr, a.Wm, (size_t)b * px, (size_t)k * px};
    }
    const int H0 = min(max(a.rows_in[b].H0, 1), a.H0), W0 = min(max(a.rows_in[b].W0, 1), a.W0), WW = (W0 + 63) >> 6;
    const size_t in = (size_t)a.rows_in[b].offset, out = (size_t)a.rows_out[k].offset;
    if (a.native) return Geo{H0, W0, WW, H0, 2 * WW, W0, in, out};
    return Geo{H0, W0, WW, a.Hm, a.wpr, a.Wm, in, out};
}

// The mask slots of frame b (n instances, the first with slot index s0): the slot of instance i starts at 32-bit word
// word0 + i * Hm * wpr of dev_masks, and the instances lo <= i < hi have one ("live": slot index in [0, capacity), and with the ragged
// rows of vti_masks_native_frames a slot that ends at or before capacity_bytes; none if bases[b] is no offset of such a buffer).
struct Slots { long long word0; int lo, hi; };
template <bool FRAMES>
__device__ __forceinline__ Slots frame_slots(const OvlArgs& a, const Geo& g, int b, int n, int s0) {
    const long long slot_words = (long long)g.Hm * g.wpr;
    Slots sl{(long long)s0 * slot_words, (int)min((long long)n, max(0ll, -(long long)s0)), (int)min((long long)n, (long long)a.capacity - s0)};
    if (FRAMES && a.native) {
        const long long base = a.bases[b];
        const long long fit = base >= 0 && !(base & 7) && a.capacity_bytes > base ? (a.capacity_bytes - base) / (slot_words * 4) : 0;
        sl.word0 = base >> 2;
        sl.hi = (int)min((long long)sl.hi, fit);
    }
    return sl;
}

template <bool FRAMES>
__global__ __launch_bounds__(kThreads) void overlay_owner_kernel(OvlArgs a) {
    __shared__ unsigned char s_ci[VTI_MEASURE_MAX_DET];         // colour index of the instance, 255: no mask slot
    const int tid = threadIdx.x, k = blockIdx.y, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    if (blockIdx.x == 0 && tid < META_INTS) a.meta[(size_t)k * META_INTS + tid] = 0;
    if (!(a.mode & VTI_OVERLAY_BLEND)) return;                  // uniform: DRAW tints nothing
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const Geo g = frame_geo<FRAMES>(a, k, b);
    const int words = g.Hm * g.wpr;
    if (FRAMES && blockIdx.x * kThreads >= words) return;       // the grid is the largest slot's: past this frame's words (the whole workgroup)
    const Slots sl = frame_slots<FRAMES>(a, g, b, n, s0);
    for (int i = tid; i < n; i += kThreads) s_ci[i] = (i >= sl.lo && i < sl.hi) ? (unsigned char)colour_index(a, b, i) : 255;
    __syncthreads();
    const int idx = blockIdx.x * kThreads + tid;
    if (idx >= words) return;
    const unsigned* bits = (const unsigned*)a.masks + sl.word0;
    unsigned owned = 0, p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    for (int i = n - 1; i >= 0 && owned != 0xffffffffu; --i) {
        const unsigned ci = s_ci[i];
        if (ci == 255) continue;
        const unsigned w = bits[(size_t)i * words + idx], fresh = w & ~owned;
        if (!fresh) continue;
        owned |= fresh;
        p0 |= (ci & 1) ? fresh : 0; p1 |= (ci & 2) ? fresh : 0; p2 |= (ci & 4) ? fresh : 0; p3 |= (ci & 8) ? fresh : 0;
    }
    uint4* dst = (uint4*)(a.planes + (size_t)k * a.plane_words + (size_t)idx * kPlaneWords);
    dst[0] = make_uint4(p0, p1, p2, p3);
    dst[1] = make_uint4(owned, 0, 0, 0);
}

// word w (columns 64 w .. 64 w + 63) of row y of an instance's bitmap at the frame size; slot: the instance's mask slot
__device__ __forceinline__ u64 bitmap_word(const OvlArgs& a, const Geo& g, const unsigned* slot, int y, int w, double ify, double ifx,
                                           u64 last_valid) {
    u64 acc = 0;
    if (a.native) {
        acc = ((const u64*)slot)[(size_t)y * g.WW + w];
    } else {
        const int sy = nn_src(y, ify, g.Hm);
        const unsigned* srow = slot + (size_t)sy * g.wpr;
        const int c0 = w * 64, c1 = min(c0 + 63, g.W0 - 1);
        const int q0 = nn_src(c0, ifx, g.Wm) >> 5, q1 = nn_src(c1, ifx, g.Wm) >> 5;
        unsigned any = 0;
        for (int q = q0; q <= q1; ++q) any |= srow[q];
        if (!any) return 0;
        for (int x = c0; x <= c1; ++x) {
            const int sx = nn_src(x, ifx, g.Wm);
            acc |= (u64)((srow[sx >> 5] >> (sx & 31)) & 1u) << (x - c0);
        }
    }
    return w == g.WW - 1 ? acc & last_valid : acc;
}

// vertex `pos` of a contour that starts at `base`: (x | y << 16, index of the next vertex, painter's key, 0)
struct ContEmit {
    int4* out; int base, limit, key;
    __device__ __forceinline__ void operator()(int pos, int y, int x, bool& bad) const {
        if (pos >= limit) { bad = true; return; }
        out[base + pos] = make_int4(x | (y << 16), base + pos + 1, key, 0);
    }
};

template <bool IN_LDS, bool FRAMES>
__global__ __launch_bounds__(kThreads) void overlay_contour_kernel(OvlArgs a) {
    extern __shared__ u64 s_img[];
    __shared__ int s_w[kThreads / 64];
    __shared__ int s_bad;
    const int tid = threadIdx.x, g = blockIdx.x, k = blockIdx.y, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    const Geo geo = frame_geo<FRAMES>(a, k, b);
    const int H = geo.H0, W = geo.W0, WW = geo.WW;
    // frames of differing sizes: the instantiation that suits THIS frame's bitmap traces it (overlay_layout's rule), the other leaves
    if (FRAMES && ((size_t)H * WW * 8 <= (size_t)poly::kLdsBytes) != IN_LDS) return;
    unsigned char* area = a.areas + ((size_t)k * a.groups + g) * a.area_bytes;
    int* const parent_g = (int*)area;
    unsigned* runs = (unsigned*)(area + a.off_runs);
    int* row_start = (int*)(area + a.off_rows);
    u64* img = IN_LDS ? s_img : (u64*)(area + a.off_img);
    int* meta = a.meta + (size_t)k * META_INTS;
    int4* out = a.cont + (size_t)k * a.max_points;
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const Slots sl = frame_slots<FRAMES>(a, geo, b, n, s0);
    const unsigned* slot0 = (const unsigned*)a.masks + sl.word0;
    const size_t slot_words = (size_t)geo.Hm * geo.wpr;
    const double ify = 1.0 / ((double)H / (double)geo.Hm), ifx = 1.0 / ((double)W / (double)geo.Wm);
    const u64 last_valid = (W & 63) ? ((1ull << (W & 63)) - 1) : ~0ull;
    const int trace_bound = 4 * (H + 2) * (W + 2);
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int i = g; i < n; i += a.groups) {                     // every bound and branch of this loop is uniform
        if (i < sl.lo || i >= sl.hi) continue;                  // no mask slot: no bitmap
        const unsigned* slot = slot0 + (size_t)i * slot_words;
        int any = 0;
        for (int idx = tid; idx < H * WW; idx += kThreads) {
            const int y = idx / WW, w = idx - y * WW;
            const u64 word = bitmap_word(a, geo, slot, y, w, ify, ifx, last_valid);
            img[idx] = word;
            any |= word != 0;
        }
        if (!__syncthreads_or(any)) continue;                   // an empty bitmap: no contour
        int* parent;
        bool bad;
        (void)poly::label_runs<IN_LDS>(img, H, WW, runs, row_start, parent_g, s_img, s_w, parent, bad);
        if (bad) s_bad = 1;
        __threadfence();
        __syncthreads();
        bad = s_bad != 0;
        const int key = (3 * i + T_CONTOUR + 1) << 4 | colour_index(a, b, i);
        if (!bad) {
            for (int y = tid; y < H; y += kThreads) {
                for (int r = row_start[y]; r < row_start[y + 1]; ++r) {
                    if (poly::ld_p(parent + r) != r) continue;  // a component's root run starts at its top-most, left-most pixel
                    const int sx = (int)(runs[r] & 0xffff);
                    int c0 = 0;
                    ContEmit none{nullptr, 0, 0, 0};
                    const int cnt = poly::trace_outer<false>(WW, H, img, y, sx, trace_bound, c0, bad, none);
                    if (bad) break;
                    if (cnt < 1) continue;
                    const int base = atomicAdd(&meta[META_TOTAL], cnt);
                    if ((long long)base + cnt > a.max_points) continue;
                    ContEmit em{out, base, cnt, key};
                    poly::trace_outer<true>(WW, H, img, y, sx, trace_bound, c0, bad, em);
                    out[base + cnt - 1].y = base;               // the contour closes on its first vertex
                }
                if (bad) break;
            }
        }
        if (bad) s_bad = 1;
        __syncthreads();                                        // the image and parent[] are free for the next instance
        if (s_bad) break;
    }
    if (tid == 0 && s_bad) meta[META_BAD] = 1;
}

// the painter of one raster tile: pixels [p0, p1) of the frame in row-major order, rows ylo .. yhi
struct TilePaint {
    int ylo, yhi, W, p0, p1;
    unsigned* prio;
    unsigned key;
    __device__ __forceinline__ void span(int y, ann::i64 xa, ann::i64 xb) {
        if (y < ylo || y > yhi) return;
        const int x0 = (int)ann::imax(xa, 0), x1 = (int)ann::imin(xb, W - 1);
        const int q0 = max(y * W + x0, p0), q1 = min(y * W + x1, p1 - 1);
        if (x0 > x1) return;
        for (int q = q0; q <= q1; ++q) atomicMax(&prio[q - p0], key);
    }
};

// the colour index that tints mask pixel (sy, sx), or -1; the planes of the last word read stay in registers
struct OwnerWord { int idx; uint4 p; unsigned owned; };
__device__ __forceinline__ int owner_of(int wpr, const unsigned* planes, int sy, int sx, OwnerWord& c) {
    const int idx = sy * wpr + (sx >> 5);
    if (idx != c.idx) {
        const uint4* src = (const uint4*)(planes + (size_t)idx * kPlaneWords);
        c.p = src[0];
        c.owned = src[1].x;
        c.idx = idx;
    }
    const int bit = sx & 31;
    if (!((c.owned >> bit) & 1u)) return -1;
    return (int)(((c.p.x >> bit) & 1u) | ((c.p.y >> bit) & 1u) << 1 | ((c.p.z >> bit) & 1u) << 2 | ((c.p.w >> bit) & 1u) << 3);
}

// one output pixel: `fr` the frame's, `an` the caller's picture (BLEND), `pr` the tile's priority word, `own` the tint's colour index
__device__ __forceinline__ void out_pixel(const OvlArgs& a, const unsigned* s_pal, const unsigned char* fr, const unsigned char* an,
                                          unsigned pr, int own, unsigned char* o) {
    const unsigned dc = s_pal[pr & 15], tc = s_pal[own & 15];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned char drawn = pr ? (unsigned char)(dc >> (8 * ch)) : an[ch];
        const unsigned char tinted = own >= 0 ? (unsigned char)(tc >> (8 * ch)) : fr[ch];
        o[ch] = (a.mode & VTI_OVERLAY_BLEND) ? ovl::blend(tinted, drawn, a.alpha, a.beta) : drawn;
    }
}

template <bool FRAMES>
__global__ __launch_bounds__(kThreads) void overlay_raster_kernel(OvlArgs a) {
    extern __shared__ unsigned s_prio[];        // [kTile]
    __shared__ unsigned s_pal[16];
    const int tid = threadIdx.x, k = blockIdx.y, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    const Geo g = frame_geo<FRAMES>(a, k, b);
    const int H0 = g.H0, W0 = g.W0;
    const int npx = H0 * W0, p0 = blockIdx.x * kTile, p1 = min(p0 + kTile, npx);
    if (FRAMES && p0 >= npx) return;            // the grid is the largest frame's: past this frame's last tile (the whole workgroup)
    const int* meta = a.meta + (size_t)k * META_INTS;
    const bool draw = (a.mode & VTI_OVERLAY_DRAW) != 0, blend = (a.mode & VTI_OVERLAY_BLEND) != 0;
    const bool skipped = draw && (meta[META_BAD] != 0 || meta[META_TOTAL] > a.max_points);
    if (blockIdx.x == 0 && tid == 0) a.status_out[k] = skipped ? VTI_OVERLAY_OUTLINE_SKIPPED : 0;
    if (tid < 16) s_pal[tid] = palette_entry(a, tid);
    for (int i = tid; i < kTile; i += kThreads) s_prio[i] = 0;
    __syncthreads();
    if (draw) {
        const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
        const int n_cont = skipped ? 0 : min(max(meta[META_TOTAL], 0), a.max_points);
        const int4* cont = a.cont + (size_t)k * a.max_points;
        const int total = 2 * n + n_cont;
        TilePaint P{p0 / W0, (p1 - 1) / W0, W0, p0, p1, s_prio, 0};
        for (int it = tid; it < total; it += kThreads) {
            if (it < n) {                       // the box of instance it: the closed polyline of its corners (cv::rectangle), thickness 2
                const float* bx = a.xyxy + ((size_t)b * M + it) * 4;
                const int x0 = clampc((int)bx[0]), y0 = clampc((int)bx[1]), x1 = clampc((int)bx[2]), y1 = clampc((int)bx[3]);
                if (max(y0, y1) + 4 < P.ylo || min(y0, y1) - 4 > P.yhi) continue;
                P.key = (unsigned)((3 * it + T_RECT + 1) << 4 | colour_index(a, b, it));
                for (int e = 0; e < 4; ++e) {   // (x0,y1)-(x0,y0)-(x1,y0)-(x1,y1)-(x0,y1)
                    const int ax = e < 2 ? x0 : x1, ay = (e == 0 || e == 3) ? y1 : y0;
                    const int ex = (e == 0 || e == 3) ? x0 : x1, ey = e < 2 ? y0 : y1;
                    ann::thick_line(W0, H0, ax, ay, ex, ey, 2, P);
                }
            } else if (it < 2 * n) {            // its plate, when the caller gave plates and the instance has a slot
                const int i = it - n, s = s0 + i;
                if (!a.plates || s < 0 || s >= a.capacity) continue;
                const int4 r = ((const int4*)a.plates)[s];
                P.key = (unsigned)((3 * i + T_PLATE + 1) << 4 | colour_index(a, b, i));
                ovl::fill_rect(H0, clampc(r.x), clampc(r.y), clampc(r.z), clampc(r.w), P);
            } else {                            // the closed polylines of the contours: vertex j -> its successor
                const int4 u = cont[it - 2 * n];
                if (u.y < 0 || u.y >= n_cont) continue;
                const int4 v = cont[u.y];
                P.key = (unsigned)u.z;
                ann::thick_line(W0, H0, u.x & 0xffff, u.x >> 16, v.x & 0xffff, v.x >> 16, 2, P);
            }
        }
        __syncthreads();
    }
    // the tile of the output: drawn pixels over the frame (BLEND: over the caller's picture), blended with the tinted frame
    const size_t off_in = g.in + (size_t)p0 * 3, off_out = g.out + (size_t)p0 * 3;
    const uint8_t* src = a.frames + off_in;
    const uint8_t* pic = a.mode == VTI_OVERLAY_BLEND ? a.annotated + off_out : src;
    uint8_t* dst = a.out + off_out;
    const unsigned* planes = a.planes + (size_t)k * a.plane_words;
    const double ify = 1.0 / ((double)H0 / (double)g.Hm), ifx = 1.0 / ((double)W0 / (double)g.Wm);
    const int np = p1 - p0;
    int done = 0;
    if ((((uintptr_t)src | (uintptr_t)pic | (uintptr_t)dst) & 15) == 0) {     // 16 pixels = 48 bytes = three 16-byte vectors per thread
        const int units = np / 16;
        for (int u = tid; u < units; u += kThreads) {
            const uint4* s4 = (const uint4*)(src + (size_t)u * 48);
            const uint4* a4 = (const uint4*)(pic + (size_t)u * 48);
            uint4 v[3] = {s4[0], s4[1], s4[2]};
            uint4 w[3] = {a4[0], a4[1], a4[2]};
            uint4 res[3];
            const uint4* pr4 = (const uint4*)(s_prio + u * 16);
            unsigned pr[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 t = pr4[q];
                pr[4 * q] = t.x; pr[4 * q + 1] = t.y; pr[4 * q + 2] = t.z; pr[4 * q + 3] = t.w;
            }
            const int p = p0 + u * 16;
            int y = p / W0, x = p - y * W0;
            int sy = a.native ? y : nn_src(y, ify, g.Hm);
            OwnerWord cache{-1, make_uint4(0, 0, 0, 0), 0};
            const unsigned char* fb = (const unsigned char*)v;
            const unsigned char* ab = (const unsigned char*)w;
            unsigned char* ob = (unsigned char*)res;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                int own = -1;
                if (blend) own = owner_of(g.wpr, planes, sy, a.native ? x : nn_src(x, ifx, g.Wm), cache);
                out_pixel(a, s_pal, fb + 3 * q, ab + 3 * q, pr[q], own, ob + 3 * q);
                if (++x == W0) { x = 0; ++y; sy = a.native ? y : nn_src(y, ify, g.Hm); }
            }
            uint4* d4 = (uint4*)(dst + (size_t)u * 48);
            d4[0] = res[0]; d4[1] = res[1]; d4[2] = res[2];
        }
        done = units * 16;
    }
    for (int q = done + tid; q < np; q += kThreads) {           // frames whose bytes are not 16-byte aligned, and the last pixels
        const int p = p0 + q, y = p / W0, x = p - y * W0;
        int own = -1;
        if (blend) {
            OwnerWord cache{-1, make_uint4(0, 0, 0, 0), 0};
            own = owner_of(g.wpr, planes, a.native ? y : nn_src(y, ify, g.Hm), a.native ? x : nn_src(x, ifx, g.Wm), cache);
        }
        unsigned char fr[3], an[3], o[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { fr[ch] = src[(size_t)q * 3 + ch]; an[ch] = pic[(size_t)q * 3 + ch]; }
        out_pixel(a, s_pal, fr, an, s_prio[q], own, o);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) dst[(size_t)q * 3 + ch] = o[ch];
    }
}

}  // namespace

void overlay_layout(int n_sel, int max_det, int H0, int W0, int Hm, int Wm, int max_points, OverlayLayout& L) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    PolyLayout pl;
    mask_polygons_layout(H0, W0, 8 * ((W0 + 63) / 64), pl);
    L.WW = pl.WW;
    L.in_lds = pl.in_lds;
    L.groups = max_det < kContourGroups ? max_det : kContourGroups;
    L.off_runs = pl.off_runs; L.off_rows = pl.off_rows;
    L.off_img = pl.off_rows + al((size_t)(H0 + 1) * 4);
    L.area_bytes = L.off_img + al((size_t)H0 * L.WW * 8);       // parent | runs | row_start | the bitmap's word rows
    // the owner planes cover a mask slot in either form: frame-size rows (native) or the letterbox canvas
    const size_t native_words = (size_t)H0 * 2 * L.WW, letter_words = (size_t)Hm * (size_t)(Wm >> 5);
    L.plane_words = (native_words > letter_words ? native_words : letter_words) * kPlaneWords;
    L.off_meta = 0;
    L.off_cont = L.off_meta + al((size_t)n_sel * META_INTS * sizeof(int));
    L.off_planes = L.off_cont + al((size_t)n_sel * (size_t)max_points * sizeof(int4));
    L.off_areas = L.off_planes + al((size_t)n_sel * L.plane_words * sizeof(unsigned));
    L.total = L.off_areas + (size_t)n_sel * L.groups * L.area_bytes;
}

hipError_t launch_overlay(const uint8_t* frames, int B, int H0, int W0, const uint8_t* masks, int native, const float* dets,
                          const float* xyxy, const int* counts, const int* offsets, int max_det, int nm, int capacity, int H, int W,
                          const int* plates, const uint8_t* palette, int n_colours, float alpha, float beta, const int* select,
                          int n_sel, int mode, const uint8_t* annotated, int max_points, uint8_t* out, int* status, void* scratch,
                          hipStream_t st, const OverlayFrames* fr) {
    OverlayLayout L;
    overlay_layout(n_sel, max_det, H0, W0, H, W, max_points, L);
    unsigned char* ws = (unsigned char*)scratch;
    OvlArgs a;
    memset(&a, 0, sizeof a);
    a.frames = frames; a.annotated = annotated; a.out = out; a.status_out = status;
    a.select = select; a.B = B; a.n_sel = n_sel; a.H0 = H0; a.W0 = W0; a.WW = L.WW;
    if (fr) { a.rows_in = fr->rows_in; a.rows_out = fr->rows_out; a.bases = fr->bases; a.capacity_bytes = fr->capacity_bytes; }
    a.masks = masks; a.dets = dets; a.xyxy = xyxy; a.counts = counts; a.offsets = offsets;
    a.max_det = max_det; a.row = 6 + nm; a.capacity = capacity; a.native = native;
    a.Hm = native ? H0 : H; a.wpr = native ? 2 * L.WW : W >> 5; a.Wm = native ? W0 : W;
    a.plates = plates;
    unsigned char pal[48] = {0};
    memcpy(pal, palette, 3 * (size_t)n_colours);
    memcpy(a.pal, pal, sizeof pal);
    a.n_colours = n_colours; a.alpha = alpha; a.beta = beta; a.mode = mode; a.max_points = max_points;
    a.meta = (int*)(ws + L.off_meta); a.cont = (int4*)(ws + L.off_cont); a.planes = (unsigned*)(ws + L.off_planes);
    a.plane_words = L.plane_words;
    a.areas = ws + L.off_areas; a.area_bytes = L.area_bytes; a.off_runs = L.off_runs; a.off_rows = L.off_rows; a.off_img = L.off_img;
    a.groups = L.groups;
    // the owner grid: the words of a mask slot -- with native rows of differing sizes those of the largest selected frame's
    const long long slot_words = fr && native ? fr->max_slot_words : (long long)a.Hm * a.wpr;
    const int owner_blocks = (mode & VTI_OVERLAY_BLEND) ? (int)((slot_words + kThreads - 1) / kThreads) : 1;
    if (fr) hipLaunchKernelGGL(overlay_owner_kernel<true>, dim3(owner_blocks, n_sel), dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL(overlay_owner_kernel<false>, dim3(owner_blocks, n_sel), dim3(kThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (mode & VTI_OVERLAY_DRAW) {
        const dim3 grid(L.groups, n_sel);
        if (fr) {
            if (fr->any_lds) {
                e = launch_lds<overlay_contour_kernel<true, true>>(grid, dim3(kThreads), (size_t)poly::kLdsBytes, st, a);
                if (e != hipSuccess) return e;
            }
            if (fr->any_global) e = launch_lds<overlay_contour_kernel<false, true>>(grid, dim3(kThreads), 0, st, a);
        } else if (L.in_lds) {
            e = launch_lds<overlay_contour_kernel<true, false>>(grid, dim3(kThreads), (size_t)poly::kLdsBytes, st, a);
        } else {
            e = launch_lds<overlay_contour_kernel<false, false>>(grid, dim3(kThreads), 0, st, a);
        }
        if (e != hipSuccess) return e;
    }
    const int tiles = (int)(((fr ? fr->max_px : (long long)H0 * W0) + kTile - 1) / kTile);
    if (fr) hipLaunchKernelGGL(overlay_raster_kernel<true>, dim3(tiles, n_sel), dim3(kThreads), (size_t)kTile * sizeof(unsigned), st, a);
    else hipLaunchKernelGGL(overlay_raster_kernel<false>, dim3(tiles, n_sel), dim3(kThreads), (size_t)kTile * sizeof(unsigned), st, a);
    return hipGetLastError();
}

}  // namespace vti
