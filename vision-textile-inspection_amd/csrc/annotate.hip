// process_frame's annotated frame on the device (vti_annotate): the overlay of measurement.py:219-504 -- ROI, boxes, fabric edge,
// stitch markers, stitch-to-edge lines, fabric outline -- painted onto a SELECTION of the batch's frames, byte for byte what the
// host restatement annotate.py gives (rasterise(frame, display_list(...))).  DESIGN.md section 5e.
//
// Three launches on the stream, ordered by the kernel boundaries only (no flags between workgroups):
//   1. prep (one workgroup per selected frame): the frame's records are reset; then the ROI and box records, the union of the kept
//      fabric masks as frame-size bit rows (letterbox bits nearest-resized as measurement.py:79 does), its lower envelope as a point
//      list, and the marker records from vti_measure's per-slot rows.  A record has a FIXED place in the frame's list -- 0: ROI,
//      1 + i: the box of instance i, 1 + M: the envelope, 2 + M + 4 j: the four markers of stitch rank j, 2 + 5 M + 2 j: its edge
//      line and point, 2 + 7 M: the outline (M = max_det) -- which is the reference's drawing order, so nothing is sorted or scanned;
//      what a frame does not draw stays an empty record.
//   2. outline (one workgroup per selected frame with status OK): the outer contours of the union, traced by vti_mask_polygons'
//      labelling and border following (polygons_dev.h); every vertex is stored with the index of the next one of its contour, so the
//      closed polylines need no per-contour table.  More than max_points vertices (or a loop bound reached): the status bit, and the
//      outline record stays empty.
//   3. raster (a workgroup per 8192 consecutive pixels of an output frame): a word per pixel in LDS holds the LAST record that
//      covers it (atomicMax of record index << 3 | colour: painter's order without ordering the work), a thread per record, envelope
//      segment or outline edge paints the rows of its primitive that fall into the tile from the closed forms of annotate_dev.h, and
//      the tile is then copied from the frame with the covered pixels replaced (16 pixels = three 16-byte vectors per thread).
//
// vti_annotate_frames (frames of differing sizes) runs the same kernels: with frame tables in AnnArgs a workgroup takes H0, W0, the
// words per union row and the frame's place in dev_frames / dev_out from the table rows of its frame instead of the launch arguments.
// The scratch regions are then PITCHED by the largest selected frame (a frame uses the head of its slice, laid out for its own size;
// what lies beyond is never read), the outline is launched in both instantiations when the selection needs both (each leaves the
// frames of the other alone, by the frame's own size), and the raster grid is the largest frame's: workgroups past a frame's last
// tile leave before the first barrier.  vti_annotate_frames_native / vti_annotate_checker_frames_native put the RAGGED form of the
// two prep kernels in front of them: the masks are then the ragged frame-size rows of vti_masks_native_frames (frame_run below).
//
// vti_annotate_checker (the stitch-distance checker's picture, Utils/check_stitch_distance.py:293-545) puts a prep kernel of its own,
// annotate_checker_prep_kernel, in front of the same outline and raster kernels: the same records, meta, envelope points and union,
// other contents (no ROI, box fall-backs filled into the union, the upper envelope, the six records of a final stitch together at
// 2 + M + 6 j).  The one thing the shared kernels take from the caller is the colour index of the outline's polylines.
#include <climits>
#include <cstring>

#include "annotate_dev.h"
#include "measure_dev.h"
#include "polygons_dev.h"

namespace vti {

namespace {

using poly::u64;

constexpr int kThreads = 256;
constexpr int kTile = 8192;                 // pixels per raster workgroup: 32 KB of LDS, a multiple of 16

enum { K_NOP = 0, K_LINE = 1, K_RECT = 2, K_CIRCLE = 3, K_POLY = 4, K_CONTOURS = 5 };
enum { C_ROI = 0, C_STITCH_BOX, C_FABRIC_BOX, C_ENVELOPE, C_WIDTH, C_CENTRE, C_DIST, C_OUTLINE };
// BGR, annotate.py's COLOURS (measurement.py:268, 272, 296, 360-364, 460-462, 499; config.py ROI_BORDER_COLOR)
static __constant__ unsigned char kColour[8][4] = {{144, 238, 144, 0}, {255, 255, 0, 0}, {255, 0, 255, 0}, {255, 128, 0, 0},
                                                   {200, 200, 0, 0},   {200, 0, 0, 0},   {0, 255, 0, 0},   {0, 0, 255, 0}};

// LINE / RECT: the two points; CIRCLE: centre (x0, y0), radius x1; POLY / CONTOURS: n points of the frame's point list
struct Rec { int kind, colour, thick, n, x0, y0, x1, y1; };
static_assert(sizeof(Rec) == 32, "records are two 16-byte vectors");
enum { META_N_ENV = 0, META_N_CONT = 1, META_OUTLINE = 2, META_INTS = 16 };

struct AnnArgs {
    const uint8_t* frames; uint8_t* out; int* status_out;
    const int* select; int B, n_sel, H0, W0, WW;               // with frame tables: the largest selected H0, W0 and their WW (pitches)
    const FrameRow* rows_in; const FrameRow* rows_out;          // device frame tables of dev_frames (B rows) and dev_out (n_sel rows), or null
    const CameraRow* table; const int* cam_of_frame; int n_cams;
    const uint8_t* masks; const float* dets; const float* xyxy; const int* counts; const int* offsets;
    int max_det, row, capacity, H, W;
    const int* frame_i32; const double* stitch_f64; const int* stitch_i32;
    int max_points, outline_colour;         // the colour index of the outline's polylines (C_OUTLINE; the checker's: C_ENVELOPE)
    Rec* recs; int* meta; int2* env_pts; int2* cont; u64* uni;
    unsigned char* areas; size_t area_bytes, off_runs, off_rows;
    const long long* bases; long long capacity_bytes;           // the ragged native rows (the RAGGED prep kernels only), or null
};

__device__ __forceinline__ int nrec(int max_det) { return 3 + 7 * max_det; }
// H0, W0 and the 64-bit words per union row of frame b: the launch arguments, or row b of the frame table (never above the pitches)
struct Geo { int H0, W0, WW; };
__device__ __forceinline__ Geo frame_geo(const AnnArgs& a, int b) {
    if (!a.rows_in) return Geo{a.H0, a.W0, a.WW};
    const int H0 = min(max(a.rows_in[b].H0, 1), a.H0), W0 = min(max(a.rows_in[b].W0, 1), a.W0);
    return Geo{H0, W0, (W0 + 63) >> 6};
}
// RAGGED (vti_annotate_frames_native): frame b's run of slots in the ragged rows of vti_masks_native_frames.  Instance i starts at byte
// bases[b] + i * slot_bytes, slot_bytes = H0 * WW * 8 (64-bit arithmetic: bases exceed 2^31), and its mask may be read iff i < fit,
// the slots that end at or before capacity_bytes (none when the base is no offset: negative, or no multiple of 8).  A later one is an
// all-zero mask whose per-slot rows exist in annotate_prep_kernel (vti_measure_frames_native's rule: it wrote them for an empty mask),
// and in annotate_checker_prep_kernel what a slot at or beyond `capacity` is (vti_measure_checker_frames_native's rule: it wrote no
// row for it); no byte at or beyond capacity_bytes is loaded.
struct Run { const u64* at; long long fit; };
__device__ __forceinline__ Run frame_run(const AnnArgs& a, int b, int H0, int WW) {
    const long long base = a.bases[b], slot_bytes = (long long)H0 * WW * 8;
    const long long fit = base >= 0 && !(base & 7) && a.capacity_bytes > base ? (a.capacity_bytes - base) / slot_bytes : 0;
    return Run{fit > 0 ? (const u64*)(a.masks + base) : (const u64*)a.masks, fit};
}
// coordinates far outside any frame change nothing that is drawn; the clamp keeps the fixed-point arithmetic in range
__device__ __forceinline__ int clampc(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int round_px(double v) { return (int)rint(fmin(fmax(v, -32768.0), 32767.0)); }   // python round(): half to even

template <bool NATIVE, bool RAGGED = false>
__global__ __launch_bounds__(kThreads) void annotate_prep_kernel(AnnArgs a) {
    static_assert(NATIVE || !RAGGED, "the ragged rows are frame-size masks");
    extern __shared__ int s_env[];              // [W0]: the nearest-resize column table, then the envelope
    __shared__ int s_fab[VTI_MEASURE_MAX_DET][3];
    __shared__ int s_nfab, s_w[kThreads / 64];
    const int tid = threadIdx.x, k = blockIdx.x, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    const Geo geo = frame_geo(a, b);
    const int H0 = geo.H0, W0 = geo.W0, WW = geo.WW;
    Rec* recs = a.recs + (size_t)k * nrec(M);
    int* meta = a.meta + (size_t)k * META_INTS;
    for (int i = tid; i < nrec(M); i += kThreads) recs[i] = Rec{K_NOP, 0, 0, 0, 0, 0, 0, 0};
    if (tid < META_INTS) meta[tid] = 0;
    if (tid == 0) { a.status_out[k] = 0; s_nfab = 0; }
    __syncthreads();
    const int ci = a.cam_of_frame ? a.cam_of_frame[b] : 0;
    if (ci < 0 || ci >= a.n_cams) return;       // uniform; no table address has been formed: the frame is copied as it is
    const CameraRow* c = a.table + ci;
    const int status = a.frame_i32[6 * (size_t)b];
    if (status != VTI_MEASURE_OK && status != VTI_MEASURE_NO_FABRIC && status != VTI_MEASURE_NO_STITCHES) return;
    const int stitch_id = c->stitch_id, fabric_id = c->fabric_id, drop_empty = c->drop_empty;
    int rr[4] = {c->roi[0], c->roi[1], c->roi[2], c->roi[3]};
    int4 roi;
    const bool roi_on = roi_clamp(c->roi_enabled, rr, H0, W0, roi);
    // 1. the ROI (measurement.py:222-238)
    if (tid == 0 && roi_on) recs[0] = Rec{K_RECT, C_ROI, 2, 0, roi.x, roi.y, roi.z, roi.w};
    // 2. boxes in detection order (measurement.py:249-272); the kept fabric instances that have a mask are listed for the union
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const int Hm = NATIVE ? H0 : a.H, wpr = NATIVE ? 2 * WW : a.W >> 5;       // rows and 32-bit words per row of a mask slot
    Run run{nullptr, 0};
    if (RAGGED) run = frame_run(a, b, H0, WW);
    for (int i = tid; i < n; i += kThreads) {
        const int s = s0 + i;
        const bool live = s >= 0 && s < a.capacity;
        const size_t di = (size_t)b * M + i;
        const float* d = a.dets + di * a.row;
        const float* bx = a.xyxy + di * 4;
        const int cls = (int)d[5];
        const bool roi_ok = !roi_on || roi_keeps(bx, roi);
        const int x1 = clampc((int)bx[0]), y1 = clampc((int)bx[1]), x2 = clampc((int)bx[2]), y2 = clampc((int)bx[3]);
        if (cls == stitch_id) {
            const bool keep = live ? (a.stitch_i32[2 * (size_t)s] & VTI_STITCH_KEPT) != 0 : (roi_ok && !drop_empty);
            if (keep) recs[1 + i] = Rec{K_RECT, C_STITCH_BOX, 1, 0, x1, y1, x2, y2};
        } else if (cls == fabric_id && roi_ok) {
            if (!live) {
                if (!drop_empty) recs[1 + i] = Rec{K_RECT, C_FABRIC_BOX, 2, 0, x1, y1, x2, y2};
            } else {
                int ya, yb;         // a mask is zero outside these rows of its slot (as vti_measure's envelope kernel reads it)
                if (NATIVE) { ya = (int)floorf(bx[1]); yb = (int)ceilf(bx[3]); }
                else { ya = (int)floorf(d[1] - 8.f); yb = (int)ceilf(d[3] + 8.f); }
                const int pos = atomicAdd(&s_nfab, 1);
                s_fab[pos][0] = i; s_fab[pos][1] = max(ya, 0); s_fab[pos][2] = min(yb, Hm - 1);
                if (RAGGED && i >= run.fit) { s_fab[pos][1] = 1; s_fab[pos][2] = 0; }    // cut by capacity_bytes: all zeros, no row is read
            }
        }
    }
    __syncthreads();
    const int nfab = s_nfab;
    const unsigned* bits = (const unsigned*)a.masks;
    for (int f = 0; f < nfab; ++f) {            // drop_empty: a fabric instance whose mask has no set bit does not exist
        const int i = s_fab[f][0], ya = s_fab[f][1], yb = s_fab[f][2];
        int any = 1;
        if (drop_empty) {
            any = 0;
            const unsigned* m = RAGGED ? (const unsigned*)run.at + ((size_t)i * Hm + ya) * wpr : bits + ((size_t)(s0 + i) * Hm + ya) * wpr;
            const int nw = yb >= ya ? (yb - ya + 1) * wpr : 0;
            for (int j = tid; j < nw; j += kThreads) any |= m[j] != 0;
            any = __syncthreads_or(any);
        }
        if (tid == 0) {
            if (any) {
                const float* bx = a.xyxy + ((size_t)b * M + i) * 4;
                recs[1 + i] = Rec{K_RECT, C_FABRIC_BOX, 2, 0, clampc((int)bx[0]), clampc((int)bx[1]), clampc((int)bx[2]), clampc((int)bx[3])};
            } else {
                s_fab[f][1] = 1; s_fab[f][2] = 0;       // an empty row range: nothing for the union
            }
        }
    }
    if (status == VTI_MEASURE_NO_FABRIC) return;        // 3. the reference returns here (measurement.py:280-287)
    __syncthreads();
    // 4a. the union of the kept fabric masks at the frame size: u64 [H0, WW], bits at columns >= W0 clear
    u64* uni = a.uni + (size_t)k * a.H0 * a.WW;
    const double ify = 1.0 / ((double)H0 / (double)a.H), ifx = 1.0 / ((double)W0 / (double)a.W);
    if (!NATIVE) {
        for (int x = tid; x < W0; x += kThreads) s_env[x] = nn_src(x, ifx, a.W);
        __syncthreads();
    }
    const u64 last_valid = (W0 & 63) ? ((1ull << (W0 & 63)) - 1) : ~0ull;
    for (int idx = tid; idx < H0 * WW; idx += kThreads) {
        const int y = idx / WW, w = idx - y * WW;
        u64 acc = 0;
        if (RAGGED) {
            for (int f = 0; f < nfab; ++f)
                if (y >= s_fab[f][1] && y <= s_fab[f][2]) acc |= run.at[(size_t)s_fab[f][0] * H0 * WW + idx];
        } else if (NATIVE) {
            for (int f = 0; f < nfab; ++f)
                if (y >= s_fab[f][1] && y <= s_fab[f][2]) acc |= ((const u64*)a.masks)[(size_t)(s0 + s_fab[f][0]) * H0 * WW + idx];
        } else {
            const int sy = nn_src(y, ify, a.H);
            const int c0 = w * 64, c1 = min(c0 + 63, W0 - 1), w0 = s_env[c0] >> 5, w1 = s_env[c1] >> 5;
            for (int f = 0; f < nfab; ++f) {
                if (sy < s_fab[f][1] || sy > s_fab[f][2]) continue;
                const unsigned* srow = bits + ((size_t)(s0 + s_fab[f][0]) * a.H + sy) * wpr;
                unsigned any = 0;
                for (int q = w0; q <= w1; ++q) any |= srow[q];
                if (!any) continue;
                for (int x = c0; x <= c1; ++x) {
                    const int sx = s_env[x];
                    acc |= (u64)((srow[sx >> 5] >> (sx & 31)) & 1u) << (x - c0);
                }
            }
        }
        if (w == WW - 1) acc &= last_valid;
        uni[idx] = acc;
    }
    __syncthreads();
    // 4b. the lower envelope per column (measurement.py:170-185): a thread per 64 columns and band of rows, bottom row first
    for (int x = tid; x < W0; x += kThreads) s_env[x] = -1;
    __syncthreads();
    {
        const int G = max(1, kThreads / WW), chunk = (H0 + G - 1) / G;
        for (int t = tid; t < WW * G; t += kThreads) {
            const int w = t % WW, g = t / WW, r_lo = g * chunk, r_hi = min(H0, r_lo + chunk);
            const u64 full = w == WW - 1 ? last_valid : ~0ull;
            u64 seen = 0;
            for (int y = r_hi - 1; y >= r_lo && seen != full; --y) {
                const u64 word = uni[(size_t)y * WW + w];
                u64 m = word & ~seen;
                while (m) {
                    atomicMax(&s_env[w * 64 + __builtin_ctzll(m)], y);
                    m &= m - 1;
                }
                seen |= word;
            }
        }
    }
    __syncthreads();
    // 4c. its valid columns, every step-th of them (measurement.py:292-296), as the envelope's point list
    int nv = 0;
    for (int x0 = 0; x0 < W0; x0 += kThreads) {
        int tot;
        (void)poly::block_excl_scan(x0 + tid < W0 && s_env[x0 + tid] >= 0, s_w, tot);
        nv += tot;
    }
    if (nv > 0) {
        const int step = max(1, nv / 1000);
        int2* pts = a.env_pts + (size_t)k * a.W0;
        int carry = 0;
        for (int x0 = 0; x0 < W0; x0 += kThreads) {
            const int x = x0 + tid;
            const int f = x < W0 && s_env[x] >= 0;
            int tot;
            const int rank = carry + poly::block_excl_scan(f, s_w, tot);
            if (f && rank % step == 0) pts[rank / step] = make_int2(x, s_env[x]);
            carry += tot;
        }
        if (tid == 0) {
            const int ne = (nv + step - 1) / step;
            meta[META_N_ENV] = ne;
            recs[1 + M] = Rec{K_POLY, C_ENVELOPE, 2, ne, 0, 0, 0, 0};
        }
    }
    if (status == VTI_MEASURE_NO_STITCHES) return;      // 5. (measurement.py:332-337)
    // 6 + 7. the markers of stitch rank j and, when it gave a distance, its edge line and point (measurement.py:359-364, 460-462)
    for (int i = tid; i < n; i += kThreads) {
        const int s = s0 + i;
        if (s < 0 || s >= a.capacity) continue;
        const int fl = a.stitch_i32[2 * (size_t)s], j = a.stitch_i32[2 * (size_t)s + 1];
        if (!(fl & VTI_STITCH_KEPT) || j < 0 || j >= M) continue;
        const double* v = a.stitch_f64 + (size_t)s * 7;
        const int cx = round_px(v[0]), cy = round_px(v[1]), lx = round_px(v[2]), rx = round_px(v[3]);
        Rec* r = recs + 2 + M + 4 * j;
        r[0] = Rec{K_CIRCLE, C_WIDTH, 0, 0, lx, cy, 3, 0};
        r[1] = Rec{K_CIRCLE, C_WIDTH, 0, 0, rx, cy, 3, 0};
        r[2] = Rec{K_LINE, C_WIDTH, 1, 0, lx, cy, rx, cy};
        r[3] = Rec{K_CIRCLE, C_CENTRE, 0, 0, cx, cy, 3, 0};
        if (fl & VTI_STITCH_DIST) {
            const int ex = min(max(cx, 0), W0 - 1), ey = round_px(v[5]);
            Rec* q = recs + 2 + 5 * M + 2 * j;
            q[0] = Rec{K_LINE, C_DIST, 1, 0, ex, ey, cx, cy};
            q[1] = Rec{K_CIRCLE, C_FABRIC_BOX, 0, 0, ex, ey, 2, 0};
        }
    }
    if (tid == 0) meta[META_OUTLINE] = 1;
}

// vti_annotate_checker's prep: the display list of Utils/check_stitch_distance.py:293-545 in the same records, meta, envelope points
// and union as annotate_prep_kernel writes, so that the outline and raster kernels serve both.  What differs: no ROI and no keep test
// (a box per existing instance); every existing fabric instance joins the union, with its mask when the mask at the frame size has a
// set bit, else with its int-truncated box filled, corners inclusive, clipped to the frame (upper_envelope_bits_kernel's rule, from
// the mask's own bits here: a source bit counts when some frame row AND some frame column map to it); the UPPER envelope; markers for
// the final set only, the six records of stitch rank j together at 2 + M + 6 j: edge line, edge point, the two width ends, the width
// line, the centroid (r = 4).  The width markers need both world points (a width from the local-scale estimate sets VTI_STITCH_WIDTH
// too), so the two ends go through the pixel_to_world that vti_measure_checker used.  c: checker_pack's row, by value.
// TABLE (vti_annotate_checker_cameras / _frames): c is row cam_of_frame[b] (null: row 0) of the camera table instead, range-checked
// before the row's address is formed (a frame whose index is outside is copied as it is), and the frame's size and the placement of
// the in and out frames come from the frame tables when there are any (frame_geo; the union and the point lists keep the pitches of
// the largest selected frame).
// RAGGED (vti_annotate_checker_frames_native): the masks are the ragged rows (frame_run); an instance is live when its slot index is
// below `capacity` AND its slot ends at or before capacity_bytes, the liveness of vti_measure_checker_frames_native.
template <bool NATIVE, bool TABLE = false, bool RAGGED = false>
__global__ __launch_bounds__(kThreads) void annotate_checker_prep_kernel(AnnArgs a, CameraRow c) {
    static_assert(!RAGGED || (NATIVE && TABLE), "the ragged rows are frame-size masks of a frame table");
    extern __shared__ int s_env[];              // [W0]: the nearest-resize column table, then the envelope | hit bits [W / 32], [H / 32]
    __shared__ int s_fab[VTI_MEASURE_MAX_DET][5];       // instance i (< 0: a filled box), first and last row, first and last column
    __shared__ int s_nfab, s_w[kThreads / 64];
    const int tid = threadIdx.x, k = blockIdx.x, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    const Geo geo = TABLE ? frame_geo(a, b) : Geo{a.H0, a.W0, a.WW};
    const int H0 = geo.H0, W0 = geo.W0, WW = geo.WW;
    Rec* recs = a.recs + (size_t)k * nrec(M);
    int* meta = a.meta + (size_t)k * META_INTS;
    for (int i = tid; i < nrec(M); i += kThreads) recs[i] = Rec{K_NOP, 0, 0, 0, 0, 0, 0, 0};
    if (tid < META_INTS) meta[tid] = 0;
    if (tid == 0) { a.status_out[k] = 0; s_nfab = 0; }
    if (TABLE) {
        const int ci = a.cam_of_frame ? a.cam_of_frame[b] : 0;
        if (ci < 0 || ci >= a.n_cams) return;   // uniform; no table address has been formed: a plain copy
        c = a.table[ci];
    }
    const int status = a.frame_i32[6 * (size_t)b];
    if (status != VTI_MEASURE_OK && status != VTI_MEASURE_NO_FABRIC && status != VTI_MEASURE_NO_STITCHES) return;   // a plain copy
    const int stitch_id = c.stitch_id, fabric_id = c.fabric_id, drop_empty = c.drop_empty;
    const int n = min(max(a.counts[b], 0), M), s0 = a.offsets[b];
    const int Hm = NATIVE ? H0 : a.H, wpr = NATIVE ? 2 * WW : a.W >> 5;       // rows and 32-bit words per row of a mask slot
    const double ify = 1.0 / ((double)H0 / (double)a.H), ifx = 1.0 / ((double)W0 / (double)a.W);
    Run run{nullptr, 0};
    if (RAGGED) {                               // the frame's first slot that is not live, as vti_measure_checker_frames_native cuts it
        run = frame_run(a, b, H0, WW);
        a.capacity = (int)min((long long)a.capacity, (long long)s0 + run.fit);
    }
    unsigned* s_col = (unsigned*)(s_env + W0);          // source columns / rows that a frame column / row is resized from
    unsigned* s_row = s_col + ((a.W + 31) >> 5);
    if (!NATIVE) {
        for (int j = tid; j < ((a.W + 31) >> 5) + ((a.H + 31) >> 5); j += kThreads) s_col[j] = 0;
        __syncthreads();
        for (int x = tid; x < W0; x += kThreads) {
            const int sx = nn_src(x, ifx, a.W);
            s_env[x] = sx;
            atomicOr(&s_col[sx >> 5], 1u << (sx & 31));
        }
        for (int y = tid; y < H0; y += kThreads) {
            const int sy = nn_src(y, ify, a.H);
            atomicOr(&s_row[sy >> 5], 1u << (sy & 31));
        }
    }
    __syncthreads();
    // cv2.rectangle(tmp, (x1i, y1i), (x2i, y2i), 1, -1) clipped to the frame (:332-333); an empty range when nothing is left
    auto box_entry = [&](int pos, const float* bx) {
        const int x1 = clampc((int)bx[0]), y1 = clampc((int)bx[1]), x2 = clampc((int)bx[2]), y2 = clampc((int)bx[3]);
        s_fab[pos][0] = -1;
        s_fab[pos][1] = max(min(y1, y2), 0); s_fab[pos][2] = min(max(y1, y2), H0 - 1);
        s_fab[pos][3] = max(min(x1, x2), 0); s_fab[pos][4] = min(max(x1, x2), W0 - 1);
    };
    // a. boxes in detection order (:323-336); the fabric instances are listed for the union
    for (int i = tid; i < n; i += kThreads) {
        const int s = s0 + i;
        const bool live = s >= 0 && s < a.capacity;
        const size_t di = (size_t)b * M + i;
        const float* d = a.dets + di * a.row;
        const float* bx = a.xyxy + di * 4;
        const int cls = (int)d[5];
        const int x1 = clampc((int)bx[0]), y1 = clampc((int)bx[1]), x2 = clampc((int)bx[2]), y2 = clampc((int)bx[3]);
        if (cls == stitch_id) {                 // a live stitch exists when vti_measure_checker listed it
            const bool exists = live ? (a.stitch_i32[2 * (size_t)s] & VTI_STITCH_KEPT) != 0 : !drop_empty;
            if (exists) recs[1 + i] = Rec{K_RECT, C_STITCH_BOX, 1, 0, x1, y1, x2, y2};
        } else if (cls == fabric_id) {
            if (!live) {                        // past the capacity: an empty mask
                if (!drop_empty) {
                    recs[1 + i] = Rec{K_RECT, C_FABRIC_BOX, 2, 0, x1, y1, x2, y2};
                    box_entry(atomicAdd(&s_nfab, 1), bx);
                }
            } else {
                int ya, yb;         // a mask is zero outside these rows of its slot (as vti_measure_checker's envelope kernel reads it)
                if (NATIVE) { ya = (int)floorf(bx[1]); yb = (int)ceilf(bx[3]); }
                else { ya = (int)floorf(d[1] - 8.f); yb = (int)ceilf(d[3] + 8.f); }
                const int pos = atomicAdd(&s_nfab, 1);
                s_fab[pos][0] = i; s_fab[pos][1] = max(ya, 0); s_fab[pos][2] = min(yb, Hm - 1); s_fab[pos][3] = 0; s_fab[pos][4] = 0;
            }
        }
    }
    __syncthreads();
    const int nfab = s_nfab;
    const unsigned* bits = (const unsigned*)a.masks;
    for (int f = 0; f < nfab; ++f) {            // per live fabric instance: does it exist (drop_empty), and has its frame-size mask a bit
        const int i = s_fab[f][0], ya = s_fab[f][1], yb = s_fab[f][2];
        if (i < 0) continue;                    // uniform
        int raw = 0, res = 0;
        const unsigned* m = RAGGED ? (const unsigned*)run.at + ((size_t)i * Hm + ya) * wpr : bits + ((size_t)(s0 + i) * Hm + ya) * wpr;
        const int nw = yb >= ya ? (yb - ya + 1) * wpr : 0;
        for (int j = tid; j < nw; j += kThreads) {
            const unsigned word = m[j];
            if (!word) continue;
            raw = 1;
            if (NATIVE) res = 1;
            else {
                const int r = j / wpr, q = j - r * wpr, sy = ya + r;
                res |= ((s_row[sy >> 5] >> (sy & 31)) & 1u) != 0 && (word & s_col[q]) != 0;
            }
        }
        raw = __syncthreads_or(raw);
        res = __syncthreads_or(res);
        if (tid == 0) {
            const float* bx = a.xyxy + ((size_t)b * M + i) * 4;
            const bool exists = !drop_empty || raw;
            if (exists) recs[1 + i] = Rec{K_RECT, C_FABRIC_BOX, 2, 0, clampc((int)bx[0]), clampc((int)bx[1]), clampc((int)bx[2]), clampc((int)bx[3])};
            if (exists && !res) box_entry(f, bx);
            else if (!exists) { s_fab[f][0] = -1; s_fab[f][1] = 1; s_fab[f][2] = 0; }      // an empty row range: nothing for the union
        }
    }
    if (status == VTI_MEASURE_NO_FABRIC) return;        // b. (:345-347)
    __syncthreads();
    // c. the union at the frame size: u64 [H0, WW], bits at columns >= W0 clear (annotate_prep_kernel's 4a, and the filled boxes)
    u64* uni = a.uni + (size_t)k * a.H0 * a.WW;
    const u64 last_valid = (W0 & 63) ? ((1ull << (W0 & 63)) - 1) : ~0ull;
    for (int idx = tid; idx < H0 * WW; idx += kThreads) {
        const int y = idx / WW, w = idx - y * WW;
        const int c0 = w * 64, c1 = min(c0 + 63, W0 - 1);
        const int sy = NATIVE ? y : nn_src(y, ify, a.H);
        const int w0 = NATIVE ? 0 : s_env[c0] >> 5, w1 = NATIVE ? 0 : s_env[c1] >> 5;
        u64 acc = 0;
        for (int f = 0; f < nfab; ++f) {
            const int i = s_fab[f][0];
            if (i < 0) {
                const int lo = max(s_fab[f][3], c0), hi = min(s_fab[f][4], c1);
                if (y >= s_fab[f][1] && y <= s_fab[f][2] && lo <= hi) acc |= (~0ull >> (63 - (hi - lo))) << (lo - c0);
                continue;
            }
            if (sy < s_fab[f][1] || sy > s_fab[f][2]) continue;
            if (RAGGED) {
                acc |= run.at[(size_t)i * H0 * WW + idx];
            } else if (NATIVE) {
                acc |= ((const u64*)a.masks)[(size_t)(s0 + i) * H0 * WW + idx];
            } else {
                const unsigned* srow = bits + ((size_t)(s0 + i) * a.H + sy) * wpr;
                unsigned any = 0;
                for (int q = w0; q <= w1; ++q) any |= srow[q];
                if (!any) continue;
                for (int x = c0; x <= c1; ++x) {
                    const int sx = s_env[x];
                    acc |= (u64)((srow[sx >> 5] >> (sx & 31)) & 1u) << (x - c0);
                }
            }
        }
        if (w == WW - 1) acc &= last_valid;
        uni[idx] = acc;
    }
    __syncthreads();
    // the upper envelope per column (:238-251): a thread per 64 columns and band of rows, top row first
    for (int x = tid; x < W0; x += kThreads) s_env[x] = INT_MAX;
    __syncthreads();
    {
        const int G = max(1, kThreads / WW), chunk = (H0 + G - 1) / G;
        for (int t = tid; t < WW * G; t += kThreads) {
            const int w = t % WW, g = t / WW, r_lo = g * chunk, r_hi = min(H0, r_lo + chunk);
            const u64 full = w == WW - 1 ? last_valid : ~0ull;
            u64 seen = 0;
            for (int y = r_lo; y < r_hi && seen != full; ++y) {
                const u64 word = uni[(size_t)y * WW + w];
                u64 m = word & ~seen;
                while (m) {
                    atomicMin(&s_env[w * 64 + __builtin_ctzll(m)], y);
                    m &= m - 1;
                }
                seen |= word;
            }
        }
    }
    __syncthreads();
    for (int x = tid; x < W0; x += kThreads) if (s_env[x] == INT_MAX) s_env[x] = -1;
    __syncthreads();
    // its valid columns, every step-th of them (:352-360), as the envelope's point list
    int nv = 0;
    for (int x0 = 0; x0 < W0; x0 += kThreads) {
        int tot;
        (void)poly::block_excl_scan(x0 + tid < W0 && s_env[x0 + tid] >= 0, s_w, tot);
        nv += tot;
    }
    if (nv > 0) {
        const int step = max(1, nv / 1000);
        int2* pts = a.env_pts + (size_t)k * a.W0;
        int carry = 0;
        for (int x0 = 0; x0 < W0; x0 += kThreads) {
            const int x = x0 + tid;
            const int f = x < W0 && s_env[x] >= 0;
            int tot;
            const int rank = carry + poly::block_excl_scan(f, s_w, tot);
            if (f && rank % step == 0) pts[rank / step] = make_int2(x, s_env[x]);
            carry += tot;
        }
        if (tid == 0) {
            const int ne = (nv + step - 1) / step;
            meta[META_N_ENV] = ne;
            recs[1 + M] = Rec{K_POLY, C_ENVELOPE, 2, ne, 0, 0, 0, 0};
        }
    }
    if (status == VTI_MEASURE_NO_STITCHES) return;      // d. (:404-406)
    // e. the final set (:431-454): the selected stitches that are near, or every selected one when none is
    const int sel_near = VTI_STITCH_KEPT | VTI_STITCH_SELECTED | VTI_STITCH_NEAR;
    int near = 0;
    for (int i = tid; i < n; i += kThreads) {
        const int s = s0 + i;
        if (s < 0 || s >= a.capacity) continue;
        near |= (a.stitch_i32[2 * (size_t)s] & sel_near) == sel_near && a.stitch_i32[2 * (size_t)s + 1] >= 0;
    }
    near = __syncthreads_or(near);
    for (int i = tid; i < n; i += kThreads) {
        const int s = s0 + i;
        if (s < 0 || s >= a.capacity) continue;
        const int fl = a.stitch_i32[2 * (size_t)s], j = a.stitch_i32[2 * (size_t)s + 1];
        if (!(fl & VTI_STITCH_KEPT) || j < 0 || j >= M) continue;
        if (!(fl & VTI_STITCH_SELECTED) || (near && !(fl & VTI_STITCH_NEAR))) continue;
        const double* v = a.stitch_f64 + (size_t)s * 7;
        const int cx = round_px(v[0]), cy = round_px(v[1]);
        Rec* r = recs + 2 + M + 6 * j;
        if (fl & VTI_STITCH_DIST) {             // :485-486
            const int ex = min(max(cx, 0), W0 - 1), ey = round_px(v[5]);
            r[0] = Rec{K_LINE, C_DIST, 1, 0, ex, ey, cx, cy};
            r[1] = Rec{K_CIRCLE, C_FABRIC_BOX, 0, 0, ex, ey, 2, 0};
        }
        if (fl & VTI_STITCH_WIDTH) {            // :493-499: only a width between two world points is drawn
            double pl[3], pr[3];
            const bool okl = pixel_to_world(c.g, v[2], v[1], pl), okr = pixel_to_world(c.g, v[3], v[1], pr);
            if (okl && okr) {
                const int lx = round_px(v[2]), rx = round_px(v[3]);
                r[2] = Rec{K_CIRCLE, C_WIDTH, 0, 0, lx, cy, 3, 0};
                r[3] = Rec{K_CIRCLE, C_WIDTH, 0, 0, rx, cy, 3, 0};
                r[4] = Rec{K_LINE, C_WIDTH, 1, 0, lx, cy, rx, cy};
            }
        }
        r[5] = Rec{K_CIRCLE, C_DIST, 0, 0, cx, cy, 4, 0};       // :510
    }
    if (tid == 0) meta[META_OUTLINE] = 1;       // f. (:543-545)
}

// vertex `pos` of a contour that starts at `base`: (x | y << 16, index of the next vertex)
struct ContEmit {
    int2* out; int base, limit;
    __device__ __forceinline__ void operator()(int pos, int y, int x, bool& bad) const {
        if (pos >= limit) { bad = true; return; }
        out[base + pos] = make_int2(x | (y << 16), base + pos + 1);
    }
};

template <bool IN_LDS>
__global__ __launch_bounds__(kThreads) void annotate_outline_kernel(AnnArgs a) {
    extern __shared__ u64 s_img[];
    __shared__ int s_w[kThreads / 64];
    __shared__ int s_bad, s_total;
    const int tid = threadIdx.x, k = blockIdx.x, M = a.max_det;
    const Geo geo = frame_geo(a, min(max(a.select[k], 0), a.B - 1));
    const int H = geo.H0, W = geo.W0, WW = geo.WW;
    const int* meta = a.meta + (size_t)k * META_INTS;
    if (!meta[META_OUTLINE]) return;            // uniform: only a frame with status OK draws its outline
    // frames of differing sizes: the instantiation that suits THIS frame's union traces it (annotate_layout's rule), the other leaves
    if (a.rows_in && ((size_t)H * WW * 8 <= (size_t)poly::kLdsBytes) != IN_LDS) return;
    unsigned char* area = a.areas + (size_t)k * a.area_bytes;
    int* const parent_g = (int*)area;
    unsigned* runs = (unsigned*)(area + a.off_runs);
    int* row_start = (int*)(area + a.off_rows);
    const u64* uni = a.uni + (size_t)k * a.H0 * a.WW;
    const u64* img = uni;
    if (tid == 0) { s_bad = 0; s_total = 0; }
    if (IN_LDS) {
        for (int i = tid; i < H * WW; i += kThreads) s_img[i] = uni[i];
        img = s_img;
    }
    __syncthreads();
    int* parent;
    bool bad;
    (void)poly::label_runs<IN_LDS>(img, H, WW, runs, row_start, parent_g, s_img, s_w, parent, bad);
    if (bad) s_bad = 1;
    __threadfence();
    __syncthreads();
    bad = s_bad != 0;
    const int trace_bound = 4 * (H + 2) * (W + 2);
    int2* out = a.cont + (size_t)k * a.max_points;
    if (!bad) {
        for (int y = tid; y < H; y += kThreads) {
            for (int r = row_start[y]; r < row_start[y + 1]; ++r) {
                if (poly::ld_p(parent + r) != r) continue;      // a component's root run starts at its top-most, left-most pixel
                const int sx = (int)(runs[r] & 0xffff);
                int c0 = 0;
                ContEmit none{nullptr, 0, 0};
                const int cnt = poly::trace_outer<false>(WW, H, img, y, sx, trace_bound, c0, bad, none);
                if (bad) break;
                const int base = atomicAdd(&s_total, cnt);
                if (cnt < 1 || (long long)base + cnt > a.max_points) continue;
                ContEmit em{out, base, cnt};
                poly::trace_outer<true>(WW, H, img, y, sx, trace_bound, c0, bad, em);
                out[base + cnt - 1].y = base;                   // the contour closes on its first vertex
            }
            if (bad) break;
        }
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0) {
        if (s_bad || s_total > a.max_points) {
            a.status_out[k] = 1;
        } else {
            a.meta[(size_t)k * META_INTS + META_N_CONT] = s_total;
            a.recs[(size_t)k * nrec(M) + 2 + 7 * M] = Rec{K_CONTOURS, a.outline_colour & 7, 2, s_total, 0, 0, 0, 0};
        }
    }
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

__global__ __launch_bounds__(kThreads) void annotate_raster_kernel(AnnArgs a) {
    extern __shared__ unsigned s_prio[];        // [kTile]
    const int tid = threadIdx.x, k = blockIdx.y, M = a.max_det;
    const int b = min(max(a.select[k], 0), a.B - 1);
    const Geo geo = frame_geo(a, b);
    const int H0 = geo.H0, W0 = geo.W0;
    const int npx = H0 * W0, p0 = blockIdx.x * kTile, p1 = min(p0 + kTile, npx);
    if (p0 >= npx) return;                      // the grid is the largest frame's: past this frame's last tile (the whole workgroup)
    for (int i = tid; i < kTile; i += kThreads) s_prio[i] = 0;
    __syncthreads();
    const Rec* recs = a.recs + (size_t)k * nrec(M);
    const int* meta = a.meta + (size_t)k * META_INTS;
    const int2* env = a.env_pts + (size_t)k * a.W0;
    const int2* cont = a.cont + (size_t)k * a.max_points;
    const int n_env = min(max(meta[META_N_ENV], 0), W0), n_cont = min(max(meta[META_N_CONT], 0), a.max_points);
    const int n_fixed = nrec(M), n_seg = max(n_env - 1, 0), total = n_fixed + n_seg + n_cont;
    TilePaint P{p0 / W0, (p1 - 1) / W0, W0, p0, p1, s_prio, 0};
    for (int it = tid; it < total; it += kThreads) {
        // every work item is a circle or 1 .. 4 line segments of one thickness (one inlined copy of the segment painter)
        int nseg = 0, thick = 2, x0 = 0, y0 = 0, x1 = 0, y1 = 0;
        if (it < n_fixed) {
            const Rec r = recs[it];
            if (r.kind == K_NOP || r.kind > K_CIRCLE) continue;
            P.key = (unsigned)(it + 1) << 3 | (unsigned)(r.colour & 7);
            if (r.kind == K_CIRCLE) {
                const int rad = min(max(r.x1, 0), 64);
                if (r.y0 + rad >= P.ylo && r.y0 - rad <= P.yhi) ann::circle(r.x0, r.y0, rad, P);
                continue;
            }
            if (max(r.y0, r.y1) + 4 < P.ylo || min(r.y0, r.y1) - 4 > P.yhi) continue;
            nseg = r.kind == K_RECT ? 4 : 1;
            thick = r.thick; x0 = r.x0; y0 = r.y0; x1 = r.x1; y1 = r.y1;
        } else if (it < n_fixed + n_seg) {      // the open polyline of the envelope: segment j -> j + 1
            const int j = it - n_fixed;
            const int2 u = env[j], v = env[j + 1];
            P.key = (unsigned)(1 + M + 1) << 3 | C_ENVELOPE;
            nseg = 1; x0 = u.x; y0 = u.y; x1 = v.x; y1 = v.y;
        } else {                                // the closed polylines of the outline: vertex j -> its successor
            const int j = it - n_fixed - n_seg;
            const int2 u = cont[j];
            if (u.y < 0 || u.y >= n_cont) continue;
            const int2 v = cont[u.y];
            P.key = (unsigned)(2 + 7 * M + 1) << 3 | (unsigned)(a.outline_colour & 7);
            nseg = 1; x0 = u.x & 0xffff; y0 = u.x >> 16; x1 = v.x & 0xffff; y1 = v.x >> 16;
        }
        for (int e = 0; e < nseg; ++e) {
            // a rectangle is the closed polyline of its corners (cv::rectangle): (x0,y1)-(x0,y0)-(x1,y0)-(x1,y1)-(x0,y1)
            int ax = x0, ay = y0, bx = x1, by = y1;
            if (nseg == 4) {
                ax = e < 2 ? x0 : x1; ay = (e == 0 || e == 3) ? y1 : y0;
                bx = (e == 0 || e == 3) ? x0 : x1; by = e < 2 ? y0 : y1;
            }
            ann::thick_line(W0, H0, ax, ay, bx, by, thick, P);
        }
    }
    __syncthreads();
    // the tile of the frame with the covered pixels replaced
    const uint8_t* src = a.frames + (a.rows_in ? (size_t)a.rows_in[b].offset : (size_t)b * npx * 3) + (size_t)p0 * 3;
    uint8_t* dst = a.out + (a.rows_out ? (size_t)a.rows_out[k].offset : (size_t)k * npx * 3) + (size_t)p0 * 3;
    const int np = p1 - p0;
    int done = 0;
    if ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0) {        // 16 pixels = 48 bytes = three 16-byte vectors per thread
        const int units = np / 16;
        for (int u = tid; u < units; u += kThreads) {
            const uint4* s4 = (const uint4*)(src + (size_t)u * 48);
            uint4 v[3] = {s4[0], s4[1], s4[2]};
            const uint4* pr4 = (const uint4*)(s_prio + u * 16);
            unsigned pr[16];
            unsigned any = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 t = pr4[q];
                pr[4 * q] = t.x; pr[4 * q + 1] = t.y; pr[4 * q + 2] = t.z; pr[4 * q + 3] = t.w;
                any |= t.x | t.y | t.z | t.w;
            }
            if (any) {
                unsigned char* bytes = (unsigned char*)v;
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (!pr[q]) continue;
                    const unsigned char* col = kColour[pr[q] & 7];
                    bytes[3 * q] = col[0]; bytes[3 * q + 1] = col[1]; bytes[3 * q + 2] = col[2];
                }
            }
            uint4* d4 = (uint4*)(dst + (size_t)u * 48);
            d4[0] = v[0]; d4[1] = v[1]; d4[2] = v[2];
        }
        done = units * 16;
    }
    for (int q = done + tid; q < np; q += kThreads) {           // frames whose bytes are not 16-byte aligned, and the last pixels
        const unsigned pr = s_prio[q];
        const unsigned char* col = kColour[pr & 7];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) dst[(size_t)q * 3 + ch] = pr ? col[ch] : src[(size_t)q * 3 + ch];
    }
}

}  // namespace

void annotate_layout(int n_sel, int max_det, int H0, int W0, int max_points, AnnotateLayout& L) {
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    PolyLayout pl;
    mask_polygons_layout(H0, W0, 8 * ((W0 + 63) / 64), pl);
    L.WW = pl.WW;
    L.in_lds = pl.in_lds;
    L.off_runs = pl.off_runs; L.off_rows = pl.off_rows;
    L.area_bytes = pl.off_rows + al((size_t)(H0 + 1) * 4);      // parent | runs | row_start: the image is the union itself
    L.off_recs = 0;
    L.off_meta = L.off_recs + al((size_t)n_sel * (3 + 7 * (size_t)max_det) * sizeof(Rec));
    L.off_env = L.off_meta + al((size_t)n_sel * META_INTS * sizeof(int));
    L.off_cont = L.off_env + al((size_t)n_sel * W0 * sizeof(int2));
    L.off_union = L.off_cont + al((size_t)n_sel * (size_t)max_points * sizeof(int2));
    L.off_areas = L.off_union + al((size_t)n_sel * H0 * L.WW * 8);
    L.total = L.off_areas + (size_t)n_sel * L.area_bytes;
}

// The layout of the scratch and the launch arguments both entry points share: the scratch carved, every field but the checker's row.
static AnnArgs annotate_args(AnnotateLayout& L, const uint8_t* frames, int H0, int W0, const CameraChoice& cams, const OutputSet& o,
                             const Canvas& cv, const DrawInputs& d, int outline_colour, const AnnotateFrames* fr) {
    annotate_layout(d.n_sel, o.max_det, H0, W0, d.max_points, L);
    unsigned char* ws = (unsigned char*)d.scratch;
    AnnArgs a;
    memset(&a, 0, sizeof a);
    a.frames = frames; a.out = d.out; a.status_out = d.status;
    a.select = d.dev_select; a.B = o.B; a.n_sel = d.n_sel; a.H0 = H0; a.W0 = W0; a.WW = L.WW;
    if (fr) { a.rows_in = fr->rows_in; a.rows_out = fr->rows_out; }
    a.table = (const CameraRow*)cams.table; a.cam_of_frame = cams.cam_of_frame; a.n_cams = cams.n_cams;
    a.masks = o.masks; a.dets = o.dets; a.xyxy = o.xyxy; a.counts = o.counts; a.offsets = o.offsets;
    a.max_det = o.max_det; a.row = 6 + cv.nm; a.capacity = o.capacity; a.H = o.native ? H0 : cv.H; a.W = o.native ? W0 : cv.W;
    a.frame_i32 = d.frame_i32; a.stitch_f64 = d.stitch_f64; a.stitch_i32 = d.stitch_i32;
    a.max_points = d.max_points; a.outline_colour = outline_colour;
    a.recs = (Rec*)(ws + L.off_recs); a.meta = (int*)(ws + L.off_meta); a.env_pts = (int2*)(ws + L.off_env);
    a.cont = (int2*)(ws + L.off_cont); a.uni = (u64*)(ws + L.off_union);
    a.areas = ws + L.off_areas; a.area_bytes = L.area_bytes; a.off_runs = L.off_runs; a.off_rows = L.off_rows;
    if (fr && o.native) { a.bases = o.bases; a.capacity_bytes = o.capacity_bytes; }     // the ragged rows: with frame tables only
    return a;
}

// The outline and raster launches that follow either prep kernel.
static hipError_t launch_outline_raster(const AnnArgs& a, const AnnotateLayout& L, const AnnotateFrames* fr, hipStream_t st) {
    hipError_t e;
    if (fr ? fr->any_lds : L.in_lds) {
        e = launch_lds<annotate_outline_kernel<true>>(dim3(a.n_sel), dim3(kThreads), (size_t)poly::kLdsBytes, st, a);
        if (e != hipSuccess) return e;
    }
    if (fr ? fr->any_global : !L.in_lds) {
        e = launch_lds<annotate_outline_kernel<false>>(dim3(a.n_sel), dim3(kThreads), 0, st, a);
        if (e != hipSuccess) return e;
    }
    const int tiles = (int)(((fr ? fr->max_px : (long long)a.H0 * a.W0) + kTile - 1) / kTile);
    hipLaunchKernelGGL(annotate_raster_kernel, dim3(tiles, a.n_sel), dim3(kThreads), (size_t)kTile * sizeof(unsigned), st, a);
    return hipGetLastError();
}

hipError_t launch_annotate(const uint8_t* frames, int H0, int W0, const CameraChoice& cams, const OutputSet& o, const Canvas& cv,
                           const DrawInputs& d, hipStream_t st, const AnnotateFrames* fr) {
    if (fr && o.native && (!o.bases || o.capacity_bytes < 0)) return hipErrorInvalidValue;      // native with tables needs bases
    AnnotateLayout L;
    const AnnArgs a = annotate_args(L, frames, H0, W0, cams, o, cv, d, C_OUTLINE, fr);
    const size_t env_lds = (size_t)W0 * sizeof(int);
    if (a.bases) hipLaunchKernelGGL((annotate_prep_kernel<true, true>), dim3(d.n_sel), dim3(kThreads), env_lds, st, a);
    else if (o.native) hipLaunchKernelGGL(annotate_prep_kernel<true>, dim3(d.n_sel), dim3(kThreads), env_lds, st, a);
    else hipLaunchKernelGGL(annotate_prep_kernel<false>, dim3(d.n_sel), dim3(kThreads), env_lds, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_outline_raster(a, L, fr, st);
}

hipError_t launch_annotate_checker(const vti_checker_params* p, const uint8_t* frames, int H0, int W0, const CameraChoice& cams,
                                   const OutputSet& o, const Canvas& cv, const DrawInputs& d, hipStream_t st,
                                   const AnnotateFrames* fr) {
    if (!p && !cams.table) return hipErrorInvalidValue;
    if (fr && (p || (o.native && (!o.bases || o.capacity_bytes < 0)))) return hipErrorInvalidValue;     // native with tables needs bases
    AnnotateLayout L;
    const AnnArgs a = annotate_args(L, frames, H0, W0, p ? CameraChoice{} : cams, o, cv, d, C_ENVELOPE, fr);
    CameraRow c;
    memset(&c, 0, sizeof c);
    if (p) checker_pack(*p, &c);
    // not native: the envelope table and the bits of the source columns and rows the resize reads
    const size_t lds = o.native ? (size_t)W0 * sizeof(int)
                                : ((size_t)W0 + (size_t)((cv.W + 31) / 32) + (size_t)((cv.H + 31) / 32)) * sizeof(int);
    const dim3 grid(d.n_sel), block(kThreads);
    if (a.bases) hipLaunchKernelGGL((annotate_checker_prep_kernel<true, true, true>), grid, block, lds, st, a, c);
    else if (p && o.native) hipLaunchKernelGGL(annotate_checker_prep_kernel<true>, grid, block, lds, st, a, c);
    else if (p) hipLaunchKernelGGL(annotate_checker_prep_kernel<false>, grid, block, lds, st, a, c);
    else if (o.native) hipLaunchKernelGGL((annotate_checker_prep_kernel<true, true>), grid, block, lds, st, a, c);
    else hipLaunchKernelGGL((annotate_checker_prep_kernel<false, true>), grid, block, lds, st, a, c);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_outline_raster(a, L, fr, st);
}

}  // namespace vti
