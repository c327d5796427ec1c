// vti_convert_raw / vti_convert_raw_frames: raw camera frames (YUYV, UYVY, NV12, NV21, I420, YV12) -> u8 [H0,W0,3] BGR or RGB, byte
// for byte the package's rawframes.to_bgr.  One launch, no scratch buffer, no memset, no host synchronisation.  The work of a lane
// (rawframes_dev.h: raw::item) is 16 raw bytes -> 24 output bytes of a 4:2:2 frame, or 16 columns of a row pair of a 4:2:0 frame
// (2 x 16 luma and 16 chroma bytes -> 2 x 48 output bytes, every chroma sample loaded once for its 2x2 block); accesses whose
// address is a multiple of their size are 8- or 16-byte vector accesses, the others and the partial items at a frame's end or right
// edge go byte by byte, both exact: a frame's bytes are written and no other.
#include <hip/hip_runtime.h>

#include "vti_internal.h"
#include "rawframes_dev.h"

namespace vti {

struct RawUniform {
    long long raw_stride, out_stride;
    int H0, W0, fmt;
};

// grid (ceil(items of the largest frame / 256), frames).  MODE 0: frames of one size, 4:2:2; 1: one size, 4:2:0; 2: frame b from row
// b of the raw table and its place in `out` from row b of the frame table.
template <int MODE>
__global__ __launch_bounds__(256) void raw_convert_kernel(const uint8_t* __restrict__ raw_buf, uint8_t* __restrict__ out,
                                                          const RawRow* __restrict__ rows, const FrameRow* __restrict__ frames,
                                                          RawUniform U, int rgb) {
    const int b = blockIdx.y;
    raw::Frame F;
    if (MODE == 2) {
        const RawRow r = rows[b];
        F.H0 = r.H0; F.W0 = r.W0; F.fmt = r.fmt;
        F.raw = raw_buf + r.raw_off;
        F.out = out + frames[b].offset;
    } else {
        F.H0 = U.H0; F.W0 = U.W0; F.fmt = U.fmt;
        F.raw = raw_buf + b * U.raw_stride;
        F.out = out + b * U.out_stride;
    }
    const int items = raw::items_of(F.fmt, F.H0, F.W0);
    if ((int)(blockIdx.x * 256u) >= items) return;          // the whole workgroup: this frame is smaller than the largest one
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= items) return;
    if (MODE == 0) raw::item_422(F, rgb, i);
    else if (MODE == 1) raw::item_420(F, rgb, i);
    else raw::item(F, rgb, i);
}

hipError_t launch_convert_raw(const uint8_t* raw_buf, int fmt, int B, int H0, int W0, int rgb, uint8_t* out, hipStream_t st) {
    RawUniform U;
    U.raw_stride = raw::frame_bytes(fmt, H0, W0);
    U.out_stride = 3LL * H0 * W0;
    U.H0 = H0; U.W0 = W0; U.fmt = fmt;
    const unsigned gx = (unsigned)((raw::items_of(fmt, H0, W0) + 255) / 256);
    if (raw::fmt_420(fmt))
        hipLaunchKernelGGL(raw_convert_kernel<1>, dim3(gx, B), dim3(256), 0, st, raw_buf, out, (const RawRow*)nullptr,
                           (const FrameRow*)nullptr, U, rgb);
    else
        hipLaunchKernelGGL(raw_convert_kernel<0>, dim3(gx, B), dim3(256), 0, st, raw_buf, out, (const RawRow*)nullptr,
                           (const FrameRow*)nullptr, U, rgb);
    return hipGetLastError();
}

hipError_t launch_convert_raw_frames(const uint8_t* raw_buf, const void* dev_raw_table, const FrameRow* dev_frame_rows, int n, int max_items,
                                     int rgb, uint8_t* out, hipStream_t st) {
    RawUniform U = {};
    hipLaunchKernelGGL(raw_convert_kernel<2>, dim3((unsigned)((max_items + 255) / 256), n), dim3(256), 0, st, raw_buf, out,
                       (const RawRow*)((const uint8_t*)dev_raw_table + sizeof(RawTableHeader)), dev_frame_rows, U, rgb);
    return hipGetLastError();
}

}  // namespace vti
