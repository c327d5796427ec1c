// What vti_measure (consumer.hip) and vti_annotate (annotate.hip) share on the device: the nearest-resize index of measurement.py:79,
// the camera-table row (private to the library build that packed it) and the ROI test of measurement.py:220-260.
#pragma once
#include "vti_internal.h"

namespace vti {

// cv2.resize(INTER_NEAREST): src index of destination index d = min(floor(d * (1 / (dst / src))), src - 1), in double.
__device__ __forceinline__ int nn_src(int d, double inv_scale, int ssize) {
    const int s = (int)floor((double)d * inv_scale);
    return s < ssize - 1 ? s : ssize - 1;
}

// One camera of vti_measure: the pixel -> world model (section N3a below) and config.py's settings.  vti_measure passes one row by
// value in the launch arguments; vti_measure_cameras keeps a table of rows in device memory (vti_measure_pack_cameras) and an index
// per frame.  The ROI is stored as given: roi_clamp applies the frame size where it is known.
struct GeomParams { double fx, fy, cx, cy, k1, k2, p1, p2, k3; double R[9]; double t[3]; double n[3]; double d; };
struct CameraRow {
    GeomParams g;
    double max_px, two_row;
    int stitch_id, fabric_id, roi_enabled, roi[4];
    int min_stitches, nb, skip_cluster, kmeans_iters, drop_empty;
    int pad[2];                             // rows are a multiple of 16 bytes; zero, so that equal settings pack to equal bytes
};
static_assert(sizeof(CameraRow) % 16 == 0, "camera table rows keep 16-byte alignment");

// measurement.py:220-238: the ROI clamped to the frame, inactive (false) when disabled or degenerate
__device__ __forceinline__ bool roi_clamp(int enabled, const int* r, int H0, int W0, int4& roi) {
    roi = make_int4(max(0, min(r[0], W0 - 1)), max(0, min(r[1], H0 - 1)), max(0, min(r[2], W0 - 1)), max(0, min(r[3], H0 - 1)));
    return enabled && roi.x < roi.z && roi.y < roi.w;
}

__device__ __forceinline__ bool roi_keeps(const float* bx, int4 roi) {
    const long long x1 = (int)bx[0], y1 = (int)bx[1], x2 = (int)bx[2], y2 = (int)bx[3];    // python int(): truncation
    return 2LL * roi.x <= x1 + x2 && x1 + x2 <= 2LL * roi.z && 2LL * roi.y <= y1 + y2 && y1 + y2 <= 2LL * roi.w;
}

}  // namespace vti
