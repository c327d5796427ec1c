// csrc/annotate_dev.h compiled for the HOST: the closed-form coverage functions vti_annotate's raster kernel paints with, behind one
// C entry point, so that tests/test_annotate_host.py can compare them with annotate.py's rasteriser without a GPU.
#define VTI_HD
#include "annotate_dev.h"

using namespace vti::ann;

namespace {
struct Paint {
    int ylo, yhi, W, H;
    unsigned char* m;
    void span(int y, i64 xa, i64 xb) {
        if (y < ylo || y > yhi || y < 0 || y >= H) return;
        xa = imax(xa, 0);
        xb = imin(xb, W - 1);
        for (i64 x = xa; x <= xb; ++x) m[(size_t)y * W + x] = 1;
    }
};
}  // namespace

// kind 0: thick_line (a, b) -> (c, d) of thickness t; kind 1: circle at (a, b) of radius t.  Only rows ylo .. yhi are painted.
extern "C" void cover(int kind, int W, int H, long long a, long long b, long long c, long long d, int t, int ylo, int yhi,
                      unsigned char* m) {
    Paint p{ylo < 0 ? 0 : ylo, yhi > H - 1 ? H - 1 : yhi, W, H, m};
    if (kind == 0) thick_line(W, H, a, b, c, d, t, p);
    else circle(a, b, t, p);
}
