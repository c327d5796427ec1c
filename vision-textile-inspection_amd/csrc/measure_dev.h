// What vti_measure (consumer.hip) and vti_annotate (annotate.hip) share on the device: the nearest-resize index of measurement.py:79,
// the camera-table row (private to the library build that packed it), the ROI test of measurement.py:220-260 and the pixel -> world
// point of measurement.py:44-65.
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

// One point; false where the reference returns None.  consumer.hip's section N3a has the
// formulas.  Shared by pixels_to_world_kernel, measure_frames_kernel, checker_frames_kernel and annotate_checker_prep_kernel.
__device__ __forceinline__ bool pixel_to_world(const GeomParams& g, double u, double v, double o[3]) {
    const double ifx = 1.0 / g.fx, ify = 1.0 / g.fy;
    double x = (u - g.cx) * ifx, y = (v - g.cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; ++j) {
        const double r2 = x * x + y * y;
        const double icdist = 1.0 / (1.0 + ((g.k3 * r2 + g.k2) * r2 + g.k1) * r2);
        if (icdist < 0) { x = (u - g.cx) * ifx; y = (v - g.cy) * ify; break; }
        const double dX = 2.0 * g.p1 * x * y + g.p2 * (r2 + 2.0 * x * x);
        const double dY = g.p1 * (r2 + 2.0 * y * y) + 2.0 * g.p2 * x * y;
        x = (x0 - dX) * icdist;
        y = (y0 - dY) * icdist;
    }
    const double denom = (g.n[0] * x + g.n[1] * y) + g.n[2];            // n . (x, y, 1)
    const bool ok = fabs(denom) >= 1e-9;
    const double s = -g.d / denom;
    const double c0 = s * x - g.t[0], c1 = s * y - g.t[1], c2 = s - g.t[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)                                          // R^T row k = column k of R
        o[k] = ok ? (g.R[k] * c0 + g.R[3 + k] * c1) + g.R[6 + k] * c2 : 0.0;
    return ok;
}

}  // namespace vti
