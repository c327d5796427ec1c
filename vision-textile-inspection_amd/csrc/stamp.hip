// The text of the annotated pictures on the device (vti_stamp, vti_stamp_frames): 1-bit stamps, rasterised once per string by the
// host, painted in one solid colour each onto the pictures vti_annotate / vti_annotate_frames / vti_annotate_checker drew, in place,
// byte for byte what the host restatement annotate.stamp gives.  DESIGN.md section 5j.
//
// One launch, a workgroup per 8192 consecutive pixels of a picture (annotate_raster_kernel's tiling):
//   1. filter: the records of the workgroup's picture, 256 at a time (a record per thread), are tested against the rows of the tile;
//      the indices of those that reach it go into a list in LDS.  Nothing is listed in any chunk: the workgroup leaves without having
//      read or written a byte of the picture, so the cost of a launch follows the text and not the pictures.
//   2. paint: a word per pixel in LDS holds the LAST record that covers it (atomicMax of the record's index in its picture, plus one:
//      painter's order whatever the order of the work, across chunks too).  A wave per listed record, a lane per (row, word) of its
//      part of the tile: one 32-bit read of the bit buffer, the columns outside the stamp's width and the picture masked off.
//   3. write: the thread that owns a pixel looks up the colour of the record its word names and stores the three bytes, once.
//      Pixels that no set bit covers are neither read nor written.
// Every rectangle is clamped to its picture, every word address to [0, n_words) and every record index to the table, so a device
// table that differs from the host copy the call validated may paint wrong pixels, but only pixels of the pictures.
#include "vti_internal.h"

namespace vti {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 8192;                 // pixels per workgroup: 32 KB of LDS
constexpr int kChunk = kThreads;            // records filtered at a time

struct StampArgs {
    uint8_t* pictures; int n, H0, W0;       // with rows: the largest frame's H0, W0
    const FrameRow* rows; long long total_bytes;
    const StampPicture* pics; const StampRec* recs; int n_stamps;
    const uint32_t* bits; long long n_words;
};

// the part of record r that lies in the picture: columns [cx0, cx1), rows [cy0, cy1)
struct Clip { int cx0, cx1, cy0, cy1; };
__device__ __forceinline__ Clip clip_rec(const StampRec& r, int H0, int W0) {
    return Clip{r.x, min(r.x + r.w, W0), r.y, min(r.y + r.h, H0)};
}
// record i with every field brought into the range the host checked it to be in (a no-op on a table that equals its host copy)
__device__ __forceinline__ StampRec load_rec(const StampRec* recs, int i) {
    StampRec r = recs[i];
    r.x = min(max(r.x, 0), kStampMaxSide); r.y = min(max(r.y, 0), kStampMaxSide);
    r.w = min(max(r.w, 0), kStampMaxSide); r.h = min(max(r.h, 0), kStampMaxSide);
    r.pitch = min(max(r.pitch, 0), kStampMaxPitch);
    return r;
}

__global__ __launch_bounds__(kThreads) void stamp_kernel(StampArgs a) {
    extern __shared__ unsigned s_prio[];    // [kTile]
    __shared__ int s_list[kChunk];
    __shared__ int s_n;
    const int tid = threadIdx.x, k = blockIdx.y;
    int H0 = a.H0, W0 = a.W0;
    size_t base = (size_t)k * a.H0 * a.W0 * 3;
    if (a.rows) {
        const FrameRow fr = a.rows[k];
        H0 = min(max(fr.H0, 1), a.H0); W0 = min(max(fr.W0, 1), a.W0);
        if (fr.offset < 0 || fr.offset > a.total_bytes || 3ll * H0 * W0 > a.total_bytes - fr.offset) return;     // uniform
        base = (size_t)fr.offset;
    }
    const int npx = H0 * W0, p0 = blockIdx.x * kTile, p1 = min(p0 + kTile, npx);
    if (p0 >= npx) return;                  // the grid is the largest picture's: past this picture's last tile (the whole workgroup)
    const StampPicture pic = a.pics[k];
    const int begin = min(max(pic.begin, 0), a.n_stamps), end = min(max(pic.end, begin), a.n_stamps);
    if (begin == end) return;               // a picture without text costs its workgroups this one 16-byte read
    const int ylo = p0 / W0, yhi = (p1 - 1) / W0;
    const int lane = tid & 63, wave = tid >> 6;
    bool painted = false;
    for (int c0 = begin; c0 < end; c0 += kChunk) {
        if (tid == 0) s_n = 0;
        __syncthreads();
        const int i = c0 + tid;
        if (i < end) {
            const Clip c = clip_rec(load_rec(a.recs, i), H0, W0);
            if (c.cx0 < c.cx1 && c.cy0 <= yhi && c.cy1 - 1 >= ylo) s_list[atomicAdd(&s_n, 1)] = i;
        }
        __syncthreads();
        const int nl = s_n;                 // uniform
        if (nl > 0 && !painted) {
            for (int q = tid; q < kTile; q += kThreads) s_prio[q] = 0;
            painted = true;
            __syncthreads();
        }
        for (int e = wave; e < nl; e += kThreads / 64) {      // nl = 0: straight to the barrier below
            const int idx = s_list[e];
            const StampRec r = load_rec(a.recs, idx);
            const Clip c = clip_rec(r, H0, W0);
            const unsigned key = (unsigned)(idx - begin) + 1u;
            const int r0 = max(c.cy0, ylo), r1 = min(c.cy1 - 1, yhi);               // rows of the stamp in the tile
            const int q0 = (c.cx0 - r.x) >> 5, q1 = (c.cx1 - 1 - r.x) >> 5;         // words of a row that hold a column of the picture
            const int nq = q1 - q0 + 1, items = (r1 - r0 + 1) * nq;
            const long long pitch = r.pitch;
            for (int it = lane; it < items; it += 64) {
                const int rr = it / nq, q = q0 + (it - rr * nq), y = r0 + rr;
                const long long at = r.offset + (long long)(y - r.y) * pitch + q;
                if (at < 0 || at >= a.n_words || q >= pitch) continue;
                unsigned word = a.bits[at];
                const int xw = r.x + 32 * q;                                        // the column of bit 0
                const int jlo = max(c.cx0 - xw, 0), jhi = min(c.cx1 - xw, 32);
                if (jhi <= jlo) continue;
                word &= (jhi - jlo == 32 ? ~0u : ((1u << (jhi - jlo)) - 1u) << jlo);
                while (word) {
                    const int p = y * W0 + xw + __builtin_ctz(word);
                    if (p >= p0 && p < p1) atomicMax(&s_prio[p - p0], key);
                    word &= word - 1;
                }
            }
        }
        // the next chunk's filter rewrites s_n and s_list behind its first barrier; the atomics above are ordered by it too
        __syncthreads();
    }
    if (!painted) return;                   // no record of the picture reaches this tile: no picture traffic
    uint8_t* dst = a.pictures + base + (size_t)p0 * 3;
    const int np = p1 - p0;
    for (int q = tid; q < np; q += kThreads) {
        const unsigned pr = s_prio[q];
        if (!pr) continue;
        const unsigned col = a.recs[min(begin + (int)pr - 1, end - 1)].colour;
        dst[(size_t)q * 3] = (uint8_t)col; dst[(size_t)q * 3 + 1] = (uint8_t)(col >> 8); dst[(size_t)q * 3 + 2] = (uint8_t)(col >> 16);
    }
}

}  // namespace

hipError_t launch_stamp(uint8_t* pictures, int n, int H0, int W0, const FrameRow* rows, long long total_bytes, long long max_px,
                        const void* table, int n_stamps, const uint32_t* bits, long long n_words, hipStream_t st) {
    if (n_stamps < 1) return hipSuccess;    // nothing to paint: nothing is launched
    StampArgs a;
    a.pictures = pictures; a.n = n; a.H0 = H0; a.W0 = W0; a.rows = rows; a.total_bytes = total_bytes;
    a.pics = (const StampPicture*)((const char*)table + sizeof(StampHeader));
    a.recs = (const StampRec*)(a.pics + n);
    a.n_stamps = n_stamps; a.bits = bits; a.n_words = n_words;
    const int tiles = (int)((max_px + kTile - 1) / kTile);
    hipLaunchKernelGGL(stamp_kernel, dim3(tiles, n), dim3(kThreads), (size_t)kTile * sizeof(unsigned), st, a);
    return hipGetLastError();
}

}  // namespace vti
