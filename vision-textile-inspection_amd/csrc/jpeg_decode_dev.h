// vti_decode_jpeg's arithmetic as plain C++ for host and device: the descriptor rows, the bit reader and the decode of one segment
// of the scan (jdhuff.c), jidctint.c's pass, jdsample.c's fancy upsampling at one pixel and jdcolor.c.  csrc/jpeg_decode.hip builds
// its kernels from these; tests/jpeg_decode_host_cover.cpp compiles them for the host and runs the entropy stage's rounds lane by
// lane, so the scheme is held to jpeg.decode without a GPU.
#pragma once
#include <stdint.h>

#ifndef VTI_HD
#define VTI_HD __host__ __device__
#endif

namespace vti {

struct JpegDHuff {              // jdhuff.c's derived table
    uint16_t look[512];         // the next 9 bits -> length << 8 | symbol; 0: the code is longer
    int32_t maxcode[18];        // largest code of length l, -1 if none; [17] ends every search
    int32_t valoff[18];         // index of the first value of length l minus its first code
    uint8_t val[256];
};
static_assert(sizeof(JpegDHuff) == 1424, "packed Huffman tables are copied to LDS word by word");
struct JpegDecRow {
    long long file_off, file_len;         // the file in dev_files
    long long scan_start, scan_end;       // the entropy-coded bytes, as offsets in dev_files
    long long out_off;                    // the frame's first byte in dev_out
    long long off_seg, off_coef, off_planes;   // in the scratch
    int H0, W0, hs, vs, mcu_rows, mcu_cols, bpm, nblk, ri, seg_bytes, nseg, pad;
    uint16_t quant[3][64];                // per component, zigzag order
    JpegDHuff huff[6];                    // DC of component 0..2, AC of component 0..2
};
static_assert(sizeof(JpegDecRow) == 9040 && sizeof(JpegDecRow) % 16 == 0, "descriptor rows stay 16-byte aligned");
constexpr int kJpegDecMagic = 0x3144504a;       // "JPD1"
constexpr int kJpegDecDefaultSegment = 256;
constexpr int kJpegDecMaxFiles = 4096;
struct JpegDecHeader {
    int magic, n, layout, seg_bytes;
    long long files_bytes, out_bytes, scratch_bytes;
    int pad[6];
};
static_assert(sizeof(JpegDecHeader) == 64, "the rows of a descriptor table stay 64-byte aligned");

namespace jpd {

VTI_HD inline int popc32(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}

// The scan's bits, MSB first.  Positions are raw: bit 8 * i + j is bit 7 - j of byte i of the scan, the stuffed 0x00 after a 0xFF
// and the RSTn markers included, so a position names a place in the file whatever lies before it.
struct BitReader {
    const uint8_t* d;           // the scan's first byte
    long long len;              // the scan's bytes
    long long bi;               // the next byte to load
    unsigned long long acc;     // the low nbits bits are the unread ones
    int nbits;
    unsigned smask;             // bit j: the j-th most recently loaded byte was a 0xFF with its stuffed 0x00 behind it
    bool stop;                  // the next byte is a marker's 0xFF or the end of the scan: nothing more is loaded

    VTI_HD void start(long long pos) {
        bi = pos >> 3;
        acc = 0;
        nbits = 0;
        smask = 0;
        stop = false;
        refill();
        const int o = (int)(pos & 7);
        nbits = nbits >= o ? nbits - o : 0;
    }
    VTI_HD void refill() {
        while (nbits <= 56 && !stop) {
            if (bi >= len) { stop = true; break; }
            const unsigned c = d[bi];
            unsigned st = 0;
            if (c == 0xFF) {
                if (bi + 1 < len && d[bi + 1] == 0) st = 1;
                else { stop = true; break; }
            }
            bi += 1 + st;
            acc = (acc << 8) | c;
            nbits += 8;
            smask = (smask << 1) | st;
        }
    }
    VTI_HD long long pos() const {
        const int nb = (nbits + 7) >> 3;                                     // buffered bytes, the partly read one included
        return bi * 8 - nbits - 8 * popc32(smask & ((1u << nb) - 1u));
    }
    // the next n <= 32 bits, zeros where the data has ended
    VTI_HD unsigned peek(int n) const {
        const unsigned long long m = (1ull << n) - 1;
        return (unsigned)((nbits >= n ? acc >> (nbits - n) : acc << (n - nbits)) & m);
    }
};

struct SegSum { unsigned nrst, cnt; };      // restart markers passed; blocks begun since the last of them (or since the entry)

// One segment from entry state (pos, block in MCU, zigzag index) to the first symbol boundary at or beyond its end.  WRITE = false:
// the exit state and the block counts.  WRITE = true: `begun` blocks were begun and `nrst` markers passed before the entry; the
// coefficients are stored and every inconsistency sets err.
template <bool WRITE>
VTI_HD inline void decode_segment(const JpegDecRow* R, const JpegDHuff* huff, const uint8_t* scan, long long scan_len, long long seg_end,
                                      unsigned long long entry, unsigned long long& exit_state, SegSum& sum, long long begun, long long nrst,
                                      int16_t* coef, int& err, int& done) {
    long long pos = (long long)(entry >> 16);
    int bim = (int)((entry >> 8) & 0xFF), k = (int)(entry & 0xFF);
    const int bpm = R->bpm, nblk = R->nblk;
    const long long IB = (long long)R->ri * bpm;
    sum.nrst = 0;
    sum.cnt = 0;
    BitReader br;
    br.d = scan;
    br.len = scan_len;
    const long long end_bits = scan_len * 8;
    if (pos < seg_end && pos < end_bits) {
        br.start(pos);
        const int max_steps = (int)(seg_end - pos) + 64;                    // every step consumes a bit or passes a marker
        for (int step = 0; step < max_steps; ++step) {
            br.refill();
            pos = br.pos();
            if (WRITE && k == 0 && begun >= nblk) {                          // the frame is complete: only padding may follow
                if (end_bits - pos > 16) err = 1;
                done = 1;
                pos = end_bits;
                break;
            }
            if (pos >= seg_end) break;
            const bool pad = br.stop && br.nbits < 8 && br.peek(br.nbits) == (1u << br.nbits) - 1u;
            if (pad) {                                                       // at a marker or at the end of the data
                long long j = br.bi;
                while (j + 1 < scan_len && scan[j + 1] == 0xFF) ++j;         // fill bytes
                const unsigned m = j + 1 < scan_len ? scan[j + 1] : 0xD9;
                if (j >= scan_len || m < 0xD0 || m > 0xD7) { pos = end_bits; break; }
                if (WRITE) {
                    const long long expect = IB ? (nrst + 1) * IB : begun;
                    if (IB == 0 || begun != expect || (long long)(m & 7) != (nrst & 7) || k != 0 || bim != 0) err = 1;
                    begun = expect < nblk ? expect : nblk;
                    ++nrst;
                }
                sum.nrst++;
                sum.cnt = 0;
                bim = 0;
                k = 0;
                br.start((j + 2) * 8);
                continue;
            }
            const int comp = bim < bpm - 2 ? 0 : bim - (bpm - 2) + 1;
            const JpegDHuff& T = huff[k == 0 ? comp : 3 + comp];
            const unsigned w = br.peek(16);
            const unsigned e = T.look[w >> 7];
            int len = (int)(e >> 8), sym = (int)(e & 255);
            if (len > 9) len = 9;
            if (!len) {
                for (int l = 10; l <= 16; ++l) {
                    const int c = (int)(w >> (16 - l));
                    if (c <= T.maxcode[l]) {
                        sym = T.val[(c + T.valoff[l]) & 255];
                        len = l;
                        break;
                    }
                }
                if (!len) {                                                  // no such code
                    len = 16;
                    sym = 0;
                    if (WRITE) err = 1;
                }
            }
            const int s = sym & 15, total = len + s;
            const unsigned extra = br.peek(total) & ((1u << s) - 1u);
            if (total > br.nbits) {                                          // the symbol runs into a marker or past the end
                if (WRITE) err = 1;
                br.nbits = 0;
                continue;
            }
            br.nbits -= total;
            const int v = s && extra < (1u << (s - 1)) ? (int)extra - (1 << s) + 1 : (int)extra;
            if (k == 0) {
                ++begun;
                ++sum.cnt;
                if (WRITE && (unsigned long long)(begun - 1) < (unsigned long long)nblk) coef[(begun - 1) * 64] = (int16_t)v;
                k = 1;
            } else if (s) {
                k += sym >> 4;
                if (k > 63) {                                                // a run past coefficient 63 is dropped
                    if (WRITE) err = 1;
                    k = 64;
                } else {
                    if (WRITE && (unsigned long long)(begun - 1) < (unsigned long long)nblk) coef[(begun - 1) * 64 + k] = (int16_t)v;
                    ++k;
                }
            } else if ((sym >> 4) == 15) {
                k += 16;
                if (k > 64) {
                    if (WRITE) err = 1;
                    k = 64;
                }
            } else {
                k = 64;
            }
            if (k >= 64) {
                k = 0;
                bim = bim + 1 >= bpm ? 0 : bim + 1;
            }
        }
        if (pos < seg_end && pos < end_bits) pos = br.pos();                 // the step bound was reached: wherever the reader stands
    }
    if (pos > end_bits) pos = end_bits;
    exit_state = ((unsigned long long)pos << 16) | ((unsigned long long)bim << 8) | (unsigned long long)k;
}

// One 1-D pass of jidctint.c on d[0], d[s], .. d[7s], descaled by N bits
template <int N>
VTI_HD inline void idct_pass(int* d, int s) {
    const int i0 = d[0], i1 = d[s], i2 = d[2 * s], i3 = d[3 * s], i4 = d[4 * s], i5 = d[5 * s], i6 = d[6 * s], i7 = d[7 * s];
    int z1 = (i2 + i6) * 4433;
    const int e2 = z1 - i6 * 15137, e3 = z1 + i2 * 6270;
    const int e0 = (int)((unsigned)(i0 + i4) << 13), e1 = (int)((unsigned)(i0 - i4) << 13);
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const int z5 = (z3 + z4) * 9633;
    t0 *= 2446;
    t1 *= 16819;
    t2 *= 25172;
    t3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    constexpr int r = 1 << (N - 1);
    d[0] = (t10 + t3 + r) >> N;
    d[7 * s] = (t10 - t3 + r) >> N;
    d[s] = (t11 + t2 + r) >> N;
    d[6 * s] = (t11 - t2 + r) >> N;
    d[2 * s] = (t12 + t1 + r) >> N;
    d[5 * s] = (t12 - t1 + r) >> N;
    d[3 * s] = (t13 + t0 + r) >> N;
    d[4 * s] = (t13 - t0 + r) >> N;
}


// the range-limit table behind RANGE_MASK, centred on 128
VTI_HD inline int range_limit(int x) {
    const int v = x & 1023;
    return v < 128 ? v + 128 : v < 512 ? 255 : v < 896 ? 0 : v - 896;
}

constexpr int fix16d(double x) { return (int)(x * 65536 + 0.5); }
constexpr int kCrR = fix16d(1.40200), kCbB = fix16d(1.77200), kCbG = fix16d(0.34414), kCrG2 = fix16d(0.71414);

// jdsample.c at output pixel (y, x) of a chroma plane P (pitch CW) whose real size is ch x cw
VTI_HD inline int chroma_at(const uint8_t* P, int CW, int ch, int cw, int hs, int vs, int y, int x) {
    if (hs == 1) return P[(long long)y * CW + x];
    const int cx = x >> 1;
    if (vs == 1) {
        const uint8_t* row = P + (long long)y * CW;
        const int c = row[cx];
        if (cw <= 2) return c;
        if (x & 1) return cx == cw - 1 ? c : (3 * c + row[cx + 1] + 2) >> 2;
        return cx == 0 ? c : (3 * c + row[cx - 1] + 1) >> 2;
    }
    const int cy = y >> 1;
    const uint8_t* r0 = P + (long long)cy * CW;
    if (cw <= 2) return r0[cx];
    const int ny = (y & 1) ? (cy + 1 < ch - 1 ? cy + 1 : ch - 1) : (cy > 1 ? cy - 1 : 0);
    const uint8_t* r1 = P + (long long)ny * CW;
    const int t = 3 * r0[cx] + r1[cx];
    if (x & 1) return cx == cw - 1 ? (4 * t + 7) >> 4 : (3 * t + 3 * r0[cx + 1] + r1[cx + 1] + 7) >> 4;
    return cx == 0 ? (4 * t + 8) >> 4 : (3 * t + 3 * r0[cx - 1] + r1[cx - 1] + 8) >> 4;
}


// jdcolor.c: (Y, Cb - 128, Cr - 128) -> p[0..2], R G B when rgb, else B G R
VTI_HD inline void store_pixel(int yy, int cb, int cr, int rgb, uint8_t* p) {
    int r = yy + ((kCrR * cr + 32768) >> 16);
    int g = yy + ((-kCbG * cb - kCrG2 * cr + 32768) >> 16);
    int b = yy + ((kCbB * cb + 32768) >> 16);
    r = r < 0 ? 0 : r > 255 ? 255 : r;
    g = g < 0 ? 0 : g > 255 ? 255 : g;
    b = b < 0 ? 0 : b > 255 ? 255 : b;
    p[0] = (uint8_t)(rgb ? r : b);
    p[1] = (uint8_t)g;
    p[2] = (uint8_t)(rgb ? b : r);
}

}  // namespace jpd
}  // namespace vti
