// csrc/overlay_dev.h compiled for the HOST: the blend and the filled-rectangle coverage vti_overlay's raster kernel uses, behind one
// C entry point, so that tests/test_overlay_host.py can compare them with overlay.py without a GPU.
#define VTI_HD
#include "overlay_dev.h"

namespace {
struct Paint {
    int ylo, yhi, W, H;
    unsigned char* m;
    void span(int y, long long xa, long long xb) {
        if (y < ylo || y > yhi || y < 0 || y >= H) return;
        if (xa < 0) xa = 0;
        if (xb > W - 1) xb = W - 1;
        for (long long x = xa; x <= xb; ++x) m[(size_t)y * W + x] += 1;
    }
};
}  // namespace

// kind 0: m[a * 256 + b] = blend(a, b, alpha, beta) for every pair.  kind 1: the rows ylo .. yhi of the filled rectangle
// (a, b) - (c, d) on a W x H mask (every painted pixel is incremented, so a pixel painted twice shows).
extern "C" void cover(int kind, int W, int H, int a, int b, int c, int d, float alpha, float beta, int ylo, int yhi, unsigned char* m) {
    if (kind == 0) {
        for (int x = 0; x < 256; ++x)
            for (int y = 0; y < 256; ++y) m[x * 256 + y] = vti::ovl::blend((uint8_t)x, (uint8_t)y, alpha, beta);
        return;
    }
    Paint p{ylo < 0 ? 0 : ylo, yhi > H - 1 ? H - 1 : yhi, W, H, m};
    vti::ovl::fill_rect(H, a, b, c, d, p);
}
