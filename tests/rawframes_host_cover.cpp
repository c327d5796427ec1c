// csrc/rawframes_dev.h compiled for the HOST: the work item one lane of vti_convert_raw's kernel does (raw::item), run item by item
// on buffers of exactly the frame's size, so tests/test_rawframes_host.py can hold both the vector and the byte path to
// rawframes.to_bgr without a GPU.  A stand-alone program:
//   rawframes_host_cover                                   self-test: every format, both rgb values, the test shapes, aligned and
//                                                          misaligned buffers, against the scalar rule written out below
//   rawframes_host_cover IN OUT fmt H0 W0 rgb n raw_off out_off
//                                                          n frames from file IN -> n * 3*H0*W0 bytes to file OUT; every frame is
//                                                          converted in its own heap buffers, which start raw_off / out_off bytes
//                                                          past an allocation boundary (0: vector path, 1: byte path) and end
//                                                          exactly where the frame ends
#define VTI_HD
#include "rawframes_dev.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace vti;

static const unsigned char kPoison = 0xA5;

// one frame through the kernel's items; false when a byte in front of either buffer changed
static bool convert(const uint8_t* src, int fmt, int H0, int W0, int rgb, int raw_off, int out_off, uint8_t* dst) {
    const size_t rb = (size_t)raw::frame_bytes(fmt, H0, W0), ob = (size_t)3 * H0 * W0;
    uint8_t* rbuf = (uint8_t*)malloc(rb + raw_off);
    uint8_t* obuf = (uint8_t*)malloc(ob + out_off);
    memset(rbuf, kPoison, raw_off);
    memset(obuf, kPoison, ob + out_off);
    memcpy(rbuf + raw_off, src, rb);
    raw::Frame F;
    F.raw = rbuf + raw_off; F.out = obuf + out_off; F.H0 = H0; F.W0 = W0; F.fmt = fmt;
    const int items = raw::items_of(fmt, H0, W0);
    for (int i = items - 1; i >= 0; --i) raw::item(F, rgb, i);          // any order: the items are independent
    bool ok = memcmp(rbuf + raw_off, src, rb) == 0;
    for (int k = 0; k < raw_off; ++k) ok = ok && rbuf[k] == kPoison;
    for (int k = 0; k < out_off; ++k) ok = ok && obuf[k] == kPoison;
    memcpy(dst, obuf + out_off, ob);
    free(rbuf);
    free(obuf);
    return ok;
}

// the rule, pixel by pixel, in the plainest form
static void reference(const uint8_t* r, int fmt, int H0, int W0, int rgb, uint8_t* out) {
    for (int y = 0; y < H0; ++y)
        for (int x = 0; x < W0; ++x) {
            int Y, U, V;
            if (fmt < kRawNV12) {
                const uint8_t* q = r + ((size_t)y * W0 + (x & ~1)) * 2;
                Y = fmt == kRawYUYV ? q[2 * (x & 1)] : q[1 + 2 * (x & 1)];
                U = fmt == kRawYUYV ? q[1] : q[0];
                V = fmt == kRawYUYV ? q[3] : q[2];
            } else {
                Y = r[(size_t)y * W0 + x];
                const uint8_t* c = r + (size_t)H0 * W0;
                const size_t plane = (size_t)(H0 / 2) * (W0 / 2), at = (size_t)(y / 2) * (W0 / 2) + x / 2;
                if (fmt == kRawNV12) { U = c[2 * at]; V = c[2 * at + 1]; }
                else if (fmt == kRawNV21) { V = c[2 * at]; U = c[2 * at + 1]; }
                else if (fmt == kRawI420) { U = c[at]; V = c[plane + at]; }
                else { V = c[at]; U = c[plane + at]; }
            }
            const long long yy = (long long)(Y > 16 ? Y - 16 : 0) * 1220542, u = U - 128, v = V - 128;
            long long R = (yy + (1 << 19) + 1673527 * v) >> 20, G = (yy + (1 << 19) - 852492 * v - 409993 * u) >> 20,
                      B = (yy + (1 << 19) + 2116026 * u) >> 20;
            R = R < 0 ? 0 : R > 255 ? 255 : R; G = G < 0 ? 0 : G > 255 ? 255 : G; B = B < 0 ? 0 : B > 255 ? 255 : B;
            uint8_t* o = out + ((size_t)y * W0 + x) * 3;
            o[0] = (uint8_t)(rgb ? R : B); o[1] = (uint8_t)G; o[2] = (uint8_t)(rgb ? B : R);
        }
}

static int self_test() {
    static const int shapes[][2] = {{2, 2}, {2, 4}, {4, 6}, {6, 10}, {18, 34}, {34, 66}, {64, 130}, {4, 32}, {2, 16}, {2, 48}};
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    int bad = 0, runs = 0;
    for (const auto& hw : shapes)
        for (int fmt = 0; fmt < kRawFormats; ++fmt)
            for (int rgb = 0; rgb < 2; ++rgb)
                for (int mis = 0; mis < 4; ++mis) {
                    const int H0 = hw[0], W0 = hw[1], ro = (mis & 1) ? 1 : 0, oo = (mis & 2) ? 3 : 0;
                    std::vector<uint8_t> r((size_t)raw::frame_bytes(fmt, H0, W0)), got((size_t)3 * H0 * W0), want(got.size());
                    for (auto& b : r) { s = s * 6364136223846793005ull + 1442695040888963407ull; b = (uint8_t)(s >> 56); }
                    const bool ok = convert(r.data(), fmt, H0, W0, rgb, ro, oo, got.data());
                    reference(r.data(), fmt, H0, W0, rgb, want.data());
                    ++runs;
                    if (!ok || got != want) {
                        ++bad;
                        fprintf(stderr, "MISMATCH fmt %d %dx%d rgb %d raw_off %d out_off %d\n", fmt, H0, W0, rgb, ro, oo);
                    }
                }
    printf("rawframes_host_cover: %d conversions, %d mismatches\n", runs, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 1) return self_test();
    if (argc != 10) {
        fprintf(stderr, "usage: %s [IN OUT fmt H0 W0 rgb n raw_off out_off]\n", argv[0]);
        return 2;
    }
    const int fmt = atoi(argv[3]), H0 = atoi(argv[4]), W0 = atoi(argv[5]), rgb = atoi(argv[6]), n = atoi(argv[7]);
    const int raw_off = atoi(argv[8]), out_off = atoi(argv[9]);
    const size_t rb = (size_t)raw::frame_bytes(fmt, H0, W0), ob = (size_t)3 * H0 * W0;
    if (!rb || n < 1 || raw_off < 0 || out_off < 0 || raw_off > 64 || out_off > 64) return 2;
    std::vector<uint8_t> in(rb * n), out(ob * n);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 3;
    fclose(f);
    bool ok = true;
    for (int k = 0; k < n; ++k) ok = convert(in.data() + rb * k, fmt, H0, W0, rgb, raw_off, out_off, out.data() + ob * k) && ok;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) return 3;
    fclose(f);
    return ok ? 0 : 1;
}
