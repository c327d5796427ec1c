// Pixel coverage of vti_annotate's primitives: annotate.py's rasteriser (OpenCV's drawing.cpp for LINE_8, shift = 0) in closed
// form, so that a workgroup that owns a few rows of a frame can paint its part of a primitive without walking the rest of it.
//   line8       Line(): pixel k of the LineIterator walk sits at major + k, minor + floor((2 d k + D - 1) / (2 D)) (D, d = the
//               larger and smaller of |dx|, |dy| of the clipped segment): the error term of the walk, summed.  A painter enters
//               the walk at the first step of its own rows (the inverse of that closed form), not at the line's start.
//   line2       Line2(): pixel k of the 16.16 fixed-point DDA sits at (x + k, (y + k * y_step) >> 16) (or its transpose).
//   fill4       FillConvexPoly() on four points: the scanline loop changes an edge only on the rows where one ends, so its state
//               is replayed over those <= 4 events and row y's span follows from the last event at or above it.
//   circle      Circle(): the spans of the midpoint walk.
//   thick_line  ThickLine(): fill4 + line2 x 4 + a circle at both ends; thickness <= 1: line8.
// Every function takes a painter P with the inclusive row range [ylo, yhi] it wants and span(y, xa, xb), which clips to the frame.
// The functions are plain C++ (host and device), so they can be compiled for the host and compared with annotate.py there.
#pragma once
#include <cmath>
#include <cstdint>

#ifndef VTI_HD
#define VTI_HD __host__ __device__
#endif

namespace vti {
namespace ann {

typedef long long i64;
constexpr int kShift = 16;
constexpr i64 kOne = 1 << kShift, kHalf = kOne >> 1;

VTI_HD inline i64 imin(i64 a, i64 b) { return a < b ? a : b; }
VTI_HD inline i64 imax(i64 a, i64 b) { return a > b ? a : b; }

// cv::clipLine(Size2l, Point2l&, Point2l&): the intersections in double, truncated
VTI_HD inline bool clip_line(i64 width, i64 height, i64& x1, i64& y1, i64& x2, i64& y2) {
    const i64 right = width - 1, bottom = height - 1;
    if (width <= 0 || height <= 0) return false;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        i64 a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (i64)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (i64)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (i64)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (i64)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

template <class P>
VTI_HD inline void line8(int W, int H, i64 x1, i64 y1, i64 x2, i64 y2, P& p) {
    if (x1 < 0 || x1 >= W || x2 < 0 || x2 >= W || y1 < 0 || y1 >= H || y2 < 0 || y2 >= H)
        if (!clip_line(W, H, x1, y1, x2, y2)) return;
    i64 dx = x2 - x1, dy = y2 - y1, sy = 1;
    if (dx < 0) { dx = -dx; dy = -dy; x1 = x2; y1 = y2; }       // left to right
    if (dy < 0) { dy = -dy; sy = -1; }
    const bool vert = dy > dx;
    const i64 D = vert ? dy : dx, d = vert ? dx : dy;
    if (vert) {                                                 // one pixel per row: only the rows the painter wants
        i64 k0, k1;
        if (sy > 0) { k0 = imax(0, p.ylo - y1); k1 = imin(D, p.yhi - y1); }
        else { k0 = imax(0, y1 - p.yhi); k1 = imin(D, y1 - p.ylo); }
        for (i64 k = k0; k <= k1; ++k) {
            const i64 x = x1 + (2 * d * k + D - 1) / (2 * D);
            p.span((int)(y1 + sy * k), x, x);
        }
    } else if (d == 0) {
        p.span((int)y1, x1, x1 + D);
    } else {
        // only the steps whose row the painter wants: the minor offset c(k) = floor((2 d k + D - 1) / (2 D)) is monotone in k, and
        // c(k) >= c  <=>  k >= ceil((2 D c - D + 1) / (2 d)); consecutive steps on one row are painted as one span
        const i64 c_lo = sy > 0 ? imax(0, p.ylo - y1) : imax(0, y1 - p.yhi), c_hi = sy > 0 ? p.yhi - y1 : y1 - p.ylo;
        if (c_hi < c_lo) return;
        const i64 k0 = c_lo == 0 ? 0 : (2 * D * c_lo - D + 1 + 2 * d - 1) / (2 * d);
        const i64 k1 = imin(D, (2 * D * (c_hi + 1) - D + 1 + 2 * d - 1) / (2 * d) - 1);
        i64 k = k0;
        while (k <= k1) {
            const i64 c = (2 * d * k + D - 1) / (2 * D);
            const i64 ke = imin(k1, (2 * D * (c + 1) - D + 1 + 2 * d - 1) / (2 * d) - 1);     // the last step on this row
            p.span((int)(y1 + sy * c), x1 + k, x1 + ke);
            k = ke + 1;
        }
    }
}

template <class P>
VTI_HD inline void put(i64 x, i64 y, P& p) {
    if (y >= p.ylo && y <= p.yhi) p.span((int)y, x, x);
}

// (x1, y1) -> (x2, y2) in 16.16 fixed point
template <class P>
VTI_HD inline void line2(int W, int H, i64 x1, i64 y1, i64 x2, i64 y2, P& p) {
    if (!clip_line((i64)W << kShift, (i64)H << kShift, x1, y1, x2, y2)) return;
    i64 dx = x2 - x1, dy = y2 - y1;
    const i64 ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax > ay) {
        if (dx < 0) { dy = -dy; i64 t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        const i64 y_step = dy * kOne / (ax | 1), ecount = (x2 - x1) >> kShift;
        x1 += kHalf; y1 += kHalf;
        put((x2 + kHalf) >> kShift, (y2 + kHalf) >> kShift, p);
        const i64 X0 = x1 >> kShift;
        for (i64 k = 0; k <= ecount; ++k) put(X0 + k, (y1 + k * y_step) >> kShift, p);
    } else {
        if (dy < 0) { dx = -dx; i64 t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        const i64 x_step = dx * kOne / (ay | 1), ecount = (y2 - y1) >> kShift;
        x1 += kHalf; y1 += kHalf;
        put((x2 + kHalf) >> kShift, (y2 + kHalf) >> kShift, p);
        const i64 Y0 = y1 >> kShift;
        const i64 k0 = imax(0, p.ylo - Y0), k1 = imin(ecount, p.yhi - Y0);
        for (i64 k = k0; k <= k1; ++k) p.span((int)(Y0 + k), (x1 + k * x_step) >> kShift, (x1 + k * x_step) >> kShift);
    }
}

template <class P>
VTI_HD inline void fill4(int W, int H, const i64* vx, const i64* vy, P& p) {
    i64 xmin = vx[0], xmax = vx[0], ymin = vy[0], ymax = vy[0];
    int im = 0;
    for (int i = 0; i < 4; ++i) {
        if (vy[i] < ymin) { ymin = vy[i]; im = i; }
        ymax = imax(ymax, vy[i]); xmax = imax(xmax, vx[i]); xmin = imin(xmin, vx[i]);
        line2(W, H, vx[(i + 3) & 3], vy[(i + 3) & 3], vx[i], vy[i], p);
    }
    xmin = (xmin + kHalf) >> kShift; xmax = (xmax + kHalf) >> kShift;
    ymin = (ymin + kHalf) >> kShift; ymax = (ymax + kHalf) >> kShift;
    if (xmax < 0 || ymax < 0 || xmin >= W || ymin >= H) return;
    ymax = imin(ymax, H - 1);
    // the events of the scanline loop: (chain, row it starts on, x there, dx per row), in row order
    int a_chain[4];
    i64 a_y[4], a_x[4], a_dx[4];
    int n_act = 0, edges = 4, e_idx[2] = {im, im};
    i64 e_ye[2] = {ymin, ymin}, y = ymin, y_stop;
    for (;;) {
        for (int i = 0; i < 2; ++i) {
            if (y < e_ye[i]) continue;
            int idx0 = e_idx[i];
            const int di = i ? 3 : 1;
            int idx = (idx0 + di) & 3;
            for (;;) {
                const bool go = edges > 0;      // `for (; edges-- > 0; )`
                --edges;
                if (!go) break;
                const i64 ty = (vy[idx] + kHalf) >> kShift;
                if (ty > y) {
                    const i64 xs = vx[idx0], xe = vx[idx];
                    a_chain[n_act] = i; a_y[n_act] = y; a_x[n_act] = xs;
                    a_dx[n_act] = ((xe - xs) * 2 + (ty - y)) / (2 * (ty - y));
                    ++n_act;
                    e_ye[i] = ty; e_idx[i] = idx;
                    break;
                }
                idx0 = idx;
                idx = (idx + di) & 3;
            }
        }
        if (edges < 0) { y_stop = y; break; }
        const i64 yn = imin(e_ye[0], e_ye[1]);
        if (yn > ymax) { y_stop = ymax + 1; break; }
        y = yn;
    }
    const i64 r0 = imax(imax(ymin, 0), p.ylo), r1 = imin(y_stop - 1, p.yhi);
    for (i64 r = r0; r <= r1; ++r) {
        i64 x[2] = {-kOne, -kOne};
        for (int k = 0; k < n_act; ++k)
            if (a_y[k] <= r) x[a_chain[k]] = a_x[k] + (r - a_y[k]) * a_dx[k];
        const i64 xl = x[0] > x[1] ? x[1] : x[0], xr = x[0] > x[1] ? x[0] : x[1];
        const i64 xx1 = (xl + kHalf) >> kShift, xx2 = (xr + kHalf) >> kShift;
        if (xx2 >= 0 && xx1 < W) p.span((int)r, imax(xx1, 0), imin(xx2, W - 1));
    }
}

template <class P>
VTI_HD inline void circle(i64 cx, i64 cy, int radius, P& p) {
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
        if (cy - dy >= p.ylo && cy - dy <= p.yhi) p.span((int)(cy - dy), cx - dx, cx + dx);
        if (cy + dy >= p.ylo && cy + dy <= p.yhi) p.span((int)(cy + dy), cx - dx, cx + dx);
        if (cy - dx >= p.ylo && cy - dx <= p.yhi) p.span((int)(cy - dx), cx - dy, cx + dy);
        if (cy + dx >= p.ylo && cy + dx <= p.yhi) p.span((int)(cy + dx), cx - dy, cx + dy);
        ++dy;
        err += plus;
        plus += 2;
        if (err > 0) { err -= minus; --dx; minus -= 2; }
    }
}

// integer pixel end points; thickness >= 1
template <class P>
VTI_HD inline void thick_line(int W, int H, i64 px0, i64 py0, i64 px1, i64 py1, int thickness, P& p) {
    if (thickness <= 1) { line8(W, H, px0, py0, px1, py1, p); return; }
    const i64 m = thickness / 2 + 2;        // the quad, its outline and the caps stay within this many rows of the end points
    if (imax(py0, py1) + m < p.ylo || imin(py0, py1) - m > p.yhi) return;
    const i64 x0 = px0 << kShift, y0 = py0 << kShift, x1 = px1 << kShift, y1 = py1 << kShift;
    const double dx = (double)(x0 - x1) * (1.0 / 65536.0), dy = (double)(y1 - y0) * (1.0 / 65536.0);
    double r = dx * dx + dy * dy;
    const int odd = thickness & 1;
    const i64 th = (i64)thickness << (kShift - 1);
    if (fabs(r) > 2.220446049250313e-16) {
        r = ((double)th + odd * 65536.0 * 0.5) / sqrt(r);
        const i64 dpx = (i64)rint(dy * r), dpy = (i64)rint(dx * r);         // cvRound: half to even
        const i64 vx[4] = {x0 + dpx, x0 - dpx, x1 - dpx, x1 + dpx}, vy[4] = {y0 + dpy, y0 - dpy, y1 - dpy, y1 + dpy};
        fill4(W, H, vx, vy, p);
    }
    const int rad = (int)((th + kHalf) >> kShift);
    circle(px0, py0, rad, p);
    circle(px1, py1, rad, p);
}

}  // namespace ann
}  // namespace vti
