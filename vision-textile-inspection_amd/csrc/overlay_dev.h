// The two per-pixel rules of vti_overlay that are not vti_annotate's: the weighted blend with OpenCV's rounding and the coverage of
// a filled rectangle (overlay.py: add_weighted, fill_rect).  Plain C++ behind VTI_HD, so they compile for the host too and are
// compared with overlay.py there (tests/overlay_host_cover.cpp).
#pragma once
#include <cmath>
#include <cstdint>

#ifndef VTI_HD
#define VTI_HD __host__ __device__
#endif

namespace vti {
namespace ovl {

// cv2.addWeighted(a, alpha, b, beta, 0) on uint8, OpenCV 4's v_fma form: the product b * beta rounded to float32, the fused
// multiply-add rounded once, then round half to even and saturate.  The operations are spelled out (no a * alpha + p expression), so
// the compiler's contraction setting cannot change them.  alpha and beta are finite (checked by the caller).
VTI_HD inline uint8_t blend(uint8_t a, uint8_t b, float alpha, float beta) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fmaf_rn((float)a, alpha, __fmul_rn((float)b, beta));
    const int r = __float2int_rn(fminf(fmaxf(t, 0.f), 255.f));
#else
    volatile float p = (float)b * beta;         // volatile: rounded to float32 here, never kept wider or contracted
    const float t = std::fmaf((float)a, alpha, p);
    const int r = (int)std::nearbyintf(std::fmin(std::fmax(t, 0.f), 255.f));     // the default rounding mode: half to even
#endif
    return (uint8_t)r;
}

// cv2.rectangle(..., -1) on (xa, ya) - (xb, yb) with xa <= xb and ya <= yb: every in-frame pixel of those columns and rows; a
// rectangle with xb < xa or yb < ya draws nothing.  Paints the rows the painter P wants (P.ylo .. P.yhi), one span(y, x0, x1) each;
// the painter clips the columns to the frame.
template <class P>
VTI_HD inline void fill_rect(int H, int xa, int ya, int xb, int yb, P& p) {
    if (xb < xa || yb < ya) return;
    const int y0 = ya > p.ylo ? ya : p.ylo, y1 = yb < p.yhi ? yb : p.yhi;
    for (int y = y0 < 0 ? 0 : y0; y <= y1 && y < H; ++y) p.span(y, xa, xb);
}

}  // namespace ovl
}  // namespace vti
