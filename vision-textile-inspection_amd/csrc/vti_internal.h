// Internal declarations shared by the host-side plan/API (vti_api.cpp, plan.cpp, weights.cpp)
// and the gfx950 kernels (conv.hip, misc.hip, post.hip).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/vti.h"
#include "jpeg_decode_dev.h"

namespace vti {

// hipFuncSetAttribute (the > 64 KB dynamic-LDS opt-in) is a per-device setting: the "already done" state of the launchers is kept
// per device, so a process that holds contexts on several GPUs sets it on each of them.
constexpr int kMaxDevices = 64;
inline int current_device_slot() { int d = 0; (void)hipGetDevice(&d); return (unsigned)d < (unsigned)kMaxDevices ? d : 0; }

// Launch kernel K with `lds` bytes of dynamic LDS.  Above 64 KB the kernel has to opt in: once per (device, kernel), and again only
// when a later launch needs more than the attribute already allows (static + dynamic LDS must fit the CU's 160 KB).
template <auto K, typename... A>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    static size_t opted_dev[kMaxDevices] = {};
    size_t& opted = opted_dev[current_device_slot()];
    if (lds > 64 * 1024 && lds > opted) {
        hipError_t e = hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        opted = lds;
    }
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    return hipGetLastError();
}

// Resident workgroups per CU of kernel K (`threads` wide, no dynamic LDS), at most `cap`; `fallback` when the query fails.
// Cached per (device, kernel).
template <auto K>
int resident_per_cu(int threads, int fallback, int cap) {
    static int per_cu_dev[kMaxDevices] = {};
    int& per_cu = per_cu_dev[current_device_slot()];
    if (!per_cu) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)K, threads, 0) != hipSuccess || nb < 1) nb = fallback;
        per_cu = nb > cap ? cap : nb;
    }
    return per_cu;
}

// Workgroups of a persistent launch: as many as fit the chip (wgpc per CU, 256 CUs, shared by gy n-groups), at most one per tile,
// lowered to `cap` when given (RunOptions.pk_max_wgs), and a multiple of 8 from 8 on (each XCD then walks a contiguous range of tiles).
inline int pk_grid(long tiles, int wgpc, int gy, int cap = 0) {
    long G = std::min<long>(tiles, std::max(1, 256 * wgpc / gy));
    if (cap) G = std::max<long>(1, std::min<long>(G, cap));
    return (int)(G >= 8 ? G & ~7L : G);
}

// ---- switches (options.cpp) -----------------------------------------------------------
// The VTI_* environment switches, parsed.  options.cpp names each of them once (name, parse rule, default, meaning) and is the only
// place that reads the environment: vti_create reads them once and keeps them in the context, vti_debug_conv2d once per call.
struct PlanOptions {         // what the planner reads (Plan::build, choose_conv_cfg)
    bool no_pk = false, no_pk1 = false, no_pk2 = false, pk_wide16 = false, no_pk_wstat = false, h2_no_n5 = false, pk1_all = false;
    bool pk1_no_wgpc2 = false, pk1_force_wgpc2 = false, conv1_wreg = true, p3_lanes = false;
    bool no_fuse = false, no_fold = false, no_bneck = false, no_bneck_tail = false, no_stem_fuse = false, no_stem_fuse3 = false;
    bool no_pred_scatter = false, no_dfl_fuse = false, no_upfuse = false, no_pk_fold = false, no_t512 = false, no_fold512 = false;
    int fold512 = -1;                        // -1: unset (on for h2 unless no_fold512), else 1 / 0
    int pk_fused = -1;                       // -1: unset (h2 box towers), 1: every fused op, 2: those with NREP <= 4, 0: none
    int pk_depth = 2, pk_fold_depth = 3;     // ring-depth caps, 2..4
    size_t pk_limit_bytes = 0x80000000ull;   // tensors from this size on stay off the persistent kernels
    size_t pk1_wstat_bytes = 96 * 1024;      // conv1_pk: weights stationary in LDS up to this size
    double pk1_inflight_bytes = 50e3;        // conv1_pk cost model: bytes in flight per CU that saturate the ingest
};
struct RunOptions {          // what the launch path reads
    int pk_max_wgs = 0;                      // cap of a persistent launch's workgroups (>= 1), 0: none
    int pk_stagger = -1;                     // delay units of the staggered 3x3 launches (0..255), -1: the dtype's default
    bool pk_linear_map = false, single_stream = false, list_ops = false, stem_not_persistent = false;
    int mask_wgs_per_cu = 0;                 // cap of launch_masks' resident workgroups per CU (>= 1), 0: none
    std::string stamp_op;                    // diagnostic build (VTI_STAMPS): the conv whose launch is stamped
};
struct Options { PlanOptions plan; RunOptions run; };
// `get` returns a switch's text or nullptr (unset); the same parse rules whichever source it reads
Options parse_options(const char* (*get)(const char* name, void* user), void* user);
Options options_from_env();

// ---- plan ---------------------------------------------------------------------------
enum ElemKind { EL_T = 0, EL_F32 = 1, EL_U8 = 2 };   // EL_T = ctx dtype (fp16, fp32, or h2 = split-fp16 pairs, 4 bytes)

struct Buf {             // one NHWC activation tensor [max_batch, H, W, C]
    int C, H, W;
    int elem;            // ElemKind
    size_t off;          // byte offset inside the workspace
    size_t bytes;        // for max_batch frames
};

struct View {            // channel slice of a Buf (concat-free C2f / neck)
    int buf = -1, coff = 0, C = 0;
};

struct ConvRow {         // fused conv table, Ultralytics order
    std::string name;
    int c1, c2, k, s, kind;
    int h_in, w_in, h_out, w_out;
    int64_t macs() const {
        const int64_t hw = (kind == 2) ? (int64_t)h_in * w_in : (int64_t)h_out * w_out;
        return hw * c1 * c2 * k * k;
    }
    int64_t fused_params() const { return (int64_t)c1 * c2 * k * k + c2; }
};

enum OpKind { OP_CONV0, OP_CONV, OP_POOL, OP_UP2, OP_DECODE, OP_FORK, OP_JOIN };
constexpr int kNumLanes = 10;         // lane 0 = the caller's stream; 1..9 = ctx-owned side streams

struct ConvCfg {         // launch geometry chosen at plan time
    int TH = 0, TW = 0;  // output tile (pixels)
    int WN = 1;          // waves along Cout (1,2,4); 4/WN waves along pixels
    int NREP = 1;        // 16-wide cout tiles per wave
    int nchunks = 0;     // K chunks (32 ch fp16 / 16 ch fp32)
    int ntiles_n = 0;    // ceil(gemmN/16)
    int gemm_n = 0;      // Cout (deconv: 4*Cout)
    size_t lds = 0;
    size_t wpk_off = 0;  // byte offset of this conv's packed weights
    size_t bias_off = 0; // float offset of this conv's bias
    // fused second stage (a 1x1 conv applied to this conv's register tile), 0 tiles = none
    int ntiles2 = 0, gemm_n2 = 0;
    size_t wpk_off2 = 0, bias_off2 = 0;
    size_t wpk_off3 = 0, bias_off3 = 0;   // stem_l1_kernel with a fused 1x1 third conv: that conv's stage-2 pack (offsets 2 = layer 1)
    // persistent LDS-DMA kernel (conv_pk.hip): TW = 20, TH = 4 * M-waves; wgpc = co-resident workgroups per CU
    int pk = 0, pk_wgpc = 1;         // pk: 1 = conv3_pk, 2 = conv1_pk (TH = compute waves along M, TW = 80), 3 = bneck_pk (fused 3x3 -> 3x3 pair), 4 = conv3_pk stride 2
    int pk_depth = 2, pk_wstat = 0;  // conv1_pk: stage-ring depth, weights stationary in LDS (1) or in the compute waves' registers (2)
    int pk_cps = 1;                  // conv1_pk: K chunks per step
    int threads = 256;               // per-tile kernel: 256, or 512 (fused towers on wide maps: one 8-wave workgroup per CU, 16 x 40 tiles)
    int wreg = 0;                    // 1x1 kernels: weight fragments feed the MFMAs from registers, no weight image in LDS (VTI_CONV1_WREG=0: off)
};

struct Op {
    OpKind kind;
    int conv = -1;       // index into convs (OP_CONV0 / OP_CONV)
    View in, out, res;
    bool has_res = false;
    bool out_f32 = false;
    int fused = -1;      // conv index of a 1x1 conv fused into this op's epilogue (its own op is dropped)
    int tail = -1;       // bneck_pk only: conv index of the C2f's closing 1x1 computed in the same kernel (out2 = its output; y2 is not stored)
    int pair = -1;       // conv index of the SECOND 3x3 of a fused C2f Bottleneck (bneck_pk): this op is the first; out/res are the second's
    int fold = -1;       // conv index of a ConvTranspose2d(2,2) FOLDED into this 3x3 conv (convfold_kernel): `in` is then the deconv's input
    int fused_l1 = -1;   // OP_CONV0 only: conv index of layer 1 computed by the same kernel (stem_l1_kernel); out/out2 = layer 1's view
    int pred_mode = 0, pred_cbase = 0, pred_a0 = 0;   // fused stage writes into pred instead of a head buffer (1 raw, 2 sigmoid, 3 DFL boxes)
    int dfl_stride = 0;      // pred_mode 3: the level's stride (box tower: DFL expectation + dist2bbox in the epilogue)
    int nat2 = 0;            // fused stage with an fp32 NHWC output: natural channel order (lane group g owns channels 16n+4g..+3: one
                             // store instruction then covers 64 contiguous bytes per pixel instead of four 16-byte pieces 64 B apart)
    View out2;           // where the fused conv writes
    bool out2_f32 = false;
    View up_src; int up_C = 0;   // conv1_pk only: channels [0, up_C) of `in` are read as the nearest-2x upsample of up_src (no UP2 op)
    int lane = 0;        // stream the op is enqueued on (OP_FORK/OP_JOIN: the side lane that starts/finishes)
    ConvCfg cfg;
};

struct Level { int C, H, W, stride; int box_buf, cls_buf, mc_buf; };

struct Plan {
    vti_desc desc;
    int esize = 2;                       // bytes per EL_T element
    std::vector<ConvRow> convs;
    std::vector<View> conv_out;          // where each conv's result lives (debug hook)
    std::vector<Buf> bufs;
    std::vector<Op> ops;
    std::vector<Level> levels;
    int proto_buf_c = 0;                 // npr
    View proto_src;                      // input of proto.cv3 (so cv3 writes straight to the caller's proto)
    int num_anchors = 0;
    bool pred_scatter = false;           // class/coefficient towers write pred directly; decode handles boxes only
    bool dfl_fused = false;              // ... and the box towers decode their own boxes: no decode op at all
    size_t ws_bytes = 0;
    size_t wpk_bytes = 0, bias_floats = 0;
    int64_t macs = 0, fused_params = 0;
    std::string build(const vti_desc& d, const PlanOptions& opt);     // returns "" or an error message
};

// ---- kernel parameter blocks ------------------------------------------------------------
struct ConvParams {
    const void* in; void* out; const void* res; const void* wpk; const float* bias;
    int B, Hin, Win, Hout, Wout;         // Hout/Wout: conv output grid (deconv: == Hin/Win, stores on the 2x grid)
    int Cin, in_ld, in_coff;
    int Cout;                            // GEMM N
    int out_ld, out_coff, res_ld, res_coff;
    int TH, TW, tiles_y, tiles_x, WN;
    int act, out_f32, deconv_c, swap_rb, nchunks, ntiles_n, has_res, scalar_store;
    unsigned pw_magic, rw_magic, tw_magic;   // ceil(2^32 / {PW, raw-row-bytes, TW}): division-free indexing
    unsigned wpk_bytes;                  // bytes of this conv's packed weights (buffer-load range check)
    // fused 1x1 second stage: out2 = act2(W2 . silu(conv + bias) + bias2), never touching HBM in between
    const void* w2; const float* bias2; void* out2;
    int Cout2, ntiles2, out2_ld, out2_coff, act2 /*0 none, 1 SiLU, 2 sigmoid, 3 DFL + dist2bbox*/, out2_f32, scalar_store2, nat2, out2_bstride;
    int nt;           // threads per workgroup of the per-tile kernel (256 / 512)
    int wreg;         // 1x1: weight fragments from registers (ConvCfg.wreg)
    float* best;      // act2 == 2 (class scores into pred): also (max score, its first class) per anchor -> best[(b * out2_bstride + pixel) * 2], or null
    float dfl_stride;
    // persistent kernel (conv_pk.hip): tile count, workgroups along x, XCD-contiguous tile ranges, tensor sizes
    int pk, pk_tiles, pk_wgs, pk_xcd, pk_depth, pk_wstat, pk_lin /* 1: linear pixel -> column-tile map (A/B aid) */;
    int pk_cps;                          // conv1_pk: K chunks per step (1 fp16, 2 for 4-byte storage)
    int pk_stagger;                      // conv3_pk: the upper half of every XCD's workgroups starts its compute waves this many x 1024 cycles late (0: off)
    unsigned in_bytes, out_bytes, res_bytes, out2_bytes;
    // conv1_pk: channels [0, up_C) come from in2 [B, Hout/2, Wout/2, in2_ld] at (y >> 1, x >> 1): the neck's Upsample + Concat folded into the loads
    const void* in2; int in2_ld, in2_coff, up_C; unsigned in2_bytes;
    int fold;                            // convfold_kernel: stage-2 output grid is 2 Hout x 2 Wout, stage-1 bias = p.bias[border class][64]
    const void* w0; const float* bias0;  // stem_l1_kernel: the stem's packed weights / bias (wpk/bias = layer 1, w2/bias2 = the fused 1x1 third conv)
    // VTI_H2 only: accumulator scales 1 / (SW * 16) of the weights behind wpk / w2 / w0 (weights.cpp: emit_packed); 1 otherwise
    float alpha, alpha2, alpha0;
    unsigned long long* stamps;          // diagnostic build only (VTI_STAMPS): 16 s_memtime slots per workgroup
};

// dtype: VTI_F16/VTI_F32; mode 0 = NHWC conv, 1 = conv0 (u8 input, im2col K=27->32)
hipError_t launch_conv(int dtype, int ks, int stride, int nrep, int mode, const ConvParams& p,
                       size_t lds_bytes, hipStream_t st);
bool conv_fusable(int nrep, int nrep2);   // is there a (3x3 NREP) + (1x1 NREP2) fused instantiation
size_t conv_lds_bytes(int ks, int stride, int mode, int TH, int TW, int WN, int NREP, int wreg = 0);
bool conv_wreg_ok(int ks, int stride, int mode, int WN, int NREP, int threads = 256);   // per-tile 1x1 with register-fed weights: is there an instantiation
bool conv_cfg_fits(int ks, int stride, int mode, int TH, int TW, int WN, int NREP, int threads = 256);
// stem (3->16, k3 s2) + layer 1 (16->32, k3 s2) in one kernel: 16 x 20 layer-1 output tiles
hipError_t launch_stem_l1(int dtype, const ConvParams& p, hipStream_t st, bool persistent = true);
size_t stem_l1_lds_bytes(int dtype);
void stem_l1_tile(int* th, int* tw);
int stem_l1_grid(int dtype, int ntiles, bool persistent = true);     // workgroups of the launch (not persistent: one per tile, an A/B aid)
void pack_stem_toeplitz(int dtype, const ConvRow& r0, const float* w, const float* b, uint8_t* dst_w, float* dst_b, float* alpha = nullptr);
size_t packed_stem_toeplitz_bytes(int dtype);
// ConvTranspose2d(C,C,2,2) folded into the following 3x3 conv (+ its fused 1x1): four 2x2 convs on the low-resolution map
hipError_t launch_convfold(int dtype, const ConvParams& p, size_t lds_bytes, hipStream_t st);
size_t convfold_lds_bytes(int TH, int TW);
bool convfold_supported(int c_in, int c_mid, int c_out, int ntiles2);
void pack_conv_fold(int dtype, const ConvRow& rU, const ConvRow& rV, const ConvCfg& c, const float* wU, const float* bU,
                    const float* wV, const float* bV, uint8_t* dst_w, float* dst_b, float* alpha = nullptr);
size_t packed_fold_bytes(const ConvCfg& c);
hipError_t launch_conv_pk_fold(int dtype, const ConvParams& p, size_t lds_bytes, hipStream_t st);   // the same on the persistent schedule
size_t conv_pk_fold_lds_bytes(int nchunks, int depth);
int conv_pk_fold_depth(int nchunks, int maxd = 3);
void pack_conv_l1pairs(int dtype, const ConvRow& r1, const float* w, const float* b, uint8_t* dst_w, float* dst_b, float* alpha = nullptr);
size_t packed_l1pairs_bytes(int dtype);
// conv_pk.hip: persistent 3x3 kernel of stride S (1: ConvCfg.pk == 1, 2: ConvCfg.pk == 4)
hipError_t launch_conv_pk(int dtype, int S, int nrep, const ConvParams& p, size_t lds_bytes, hipStream_t st);
size_t conv_pk_lds_bytes(int S, int TH, int WN, int NREP, int nchunks, int depth, int wstat = 0);   // wstat: all K chunks' weights resident in LDS
int conv_pk_depth(int S, int TH, int WN, int NREP, int nchunks, int wstat = 0, int maxd = 2);     // maxd: PlanOptions.pk_depth; 0 = does not fit
bool conv_pk_fits(int S, int TH, int WN, int NREP, int nchunks, int wstat = 0);
bool conv_pk_instantiated(int S, int nrep, int wn);
hipError_t launch_conv1_pk(int dtype, int nrep, const ConvParams& p, size_t lds_bytes, hipStream_t st);
size_t conv1_pk_lds_bytes(int nwm, int WN, int NREP, int nchunks, int depth, int wstat, int cps = 1);   // cps: K chunks per step
bool conv1_pk_fits(int nwm, int WN, int NREP, int nchunks, int depth, int wstat, int cps = 1);
bool conv1_pk_instantiated(int nrep, int wn);
bool conv1_pk_wreg_instantiated(int dtype, int nrep, int wn, int nchunks);   // wstat == 2: the n-group's weights in the compute waves' registers
hipError_t launch_bneck_pk(int dtype, int nrep, const ConvParams& p, size_t lds_bytes, hipStream_t st);
size_t bneck_pk_lds_bytes(int TH, int NREP, int depth = 2);
int bneck_pk_depth(int TH, int NREP, int maxd = 2);
bool bneck_pk_fits(int TH, int NREP);

struct PoolParams { const void* in; void* out; int B, H, W, C, ld, in_coff, out_coff; };
hipError_t launch_sppf_pool(int dtype, const PoolParams& p, hipStream_t st);
// The kernel launch_sppf_pool runs for a map (its only decision; vti_debug_sppf_pool reports it): 4 / 1 = the LDS kernel with four /
// one 16-byte pieces per lane group, 0 = the global-memory kernel.
int sppf_pool_path(int dtype, int H, int W, int C);

struct Up2Params { const void* in; void* out; int B, H, W, C, in_ld, in_coff, out_ld, out_coff; };
hipError_t launch_upsample2x(int dtype, const Up2Params& p, hipStream_t st);

struct DecodeParams {
    const float* box[3]; const float* cls[3]; const float* mc[3];
    int H[3], W[3], stride[3], a0[3];
    int B, A, nc, nm, reg_max;
    float* pred;                          // [B, 4+nc+nm, A]
};
hipError_t launch_decode(const DecodeParams& p, hipStream_t st);         // nc + nm <= VTI_DECODE_MAX_CHANNELS (its LDS tile)
hipError_t launch_box_decode(const DecodeParams& p, hipStream_t st);   // DFL + dist2bbox only (pred_scatter plans)

// ---- launch parameters (launch.cpp; host only, nothing there sees a context, a stream or an event) ----------------------------
// The plan decides per conv, once: kernel family, tile, waves, LDS, ring depth, weight offsets (ConvCfg).  Per call, from B, swap_rb,
// the RunOptions and the tensors of that call: the tile counts, the persistent grid, the byte ranges with their 2^31 fallback, the
// pointers -- a LaunchRec per op, built on every call.
struct Bindings {            // the device tensors the parameter blocks of one forward point into
    char* ws; const void* wpk; const float* bias;      // workspace, packed weights, biases
    const float* alpha;                                // per conv: accumulator scale of its packed weights (host array)
    const void* input; float* pred; void* proto; float* best;      // the caller's (best: may be null)
};
enum Launcher { LAUNCH_STEM_L1, LAUNCH_CONV, LAUNCH_CONVFOLD, LAUNCH_CONV_PK_FOLD, LAUNCH_POOL, LAUNCH_UP2, LAUNCH_DECODE, LAUNCH_BOX_DECODE };
struct LaunchRec {           // one launch: the launcher, its selector arguments (those it takes), its block
    Launcher fn;
    const char* name;        // conv launchers: the op's conv (names the op in an error and for VTI_STAMP_OP), else null
    int dtype, ks, stride, nrep, mode;
    size_t lds;
    bool persistent;         // launch_stem_l1's
    ConvParams conv; PoolParams pool; Up2Params up2; DecodeParams dec;      // the one `fn` takes is filled
};
// The record of one op (not OP_FORK / OP_JOIN); the text of a VTI_ERR_UNSUPPORTED refusal when the op cannot run, else nullptr
const char* fill_launch(const Plan& P, const Op& op, int B, int swap_rb, const RunOptions& run, const Bindings& b, LaunchRec& L);
// The plain launch_conv record of one row with one configuration (vti_debug_conv2d; the base of the forward's conv ops)
void conv_record(const RunOptions& run, int dtype, const ConvRow& r, const ConvCfg& g, int B, const void* in, int in_ld, int in_coff,
                 void* out, int out_ld, int out_coff, const void* res, int res_ld, int res_coff, const void* wpk, const float* bias,
                 float alpha, bool out_f32, int swap_rb, LaunchRec& L);
void* buf_ptr(const Plan& P, const Bindings& b, int buf);           // where a buffer of the plan lives: input, proto or workspace
std::string op_label(const Plan& P, const Op& op);                  // "model.0 + model.1 + model.2.cv1": VTI_LIST_OPS, stamped launches
const char* launcher_name(Launcher fn);
size_t launch_workgroups(const LaunchRec& L);                       // of a conv launcher's record (diagnostic build: stamp slots)
void conv_geometry(const Plan& P, int i, vti_conv_info* o);         // vti_conv_at: tile, waves, nrep, LDS and flags of conv i's launch

hipError_t launch_debug_nchw(int elem_is_f32, const void* src, int B, int H, int W, int C, int ld, int coff,
                             float* dst, hipStream_t st);
hipError_t launch_debug_set_nchw(int elem_is_f32, const float* src, int B, int H, int W, int C, int ld, int coff,
                                 void* dst, hipStream_t st);      // the inverse, encoding as the storage does

// One frame of a batch whose frames differ in size (vti_pack_frames): what the kernels would otherwise recompute per pixel or per
// box for the ctx's H x W canvas.  A frame table is a FrameTableHeader followed by B rows; vti_letterbox / vti_scale_boxes pass one
// row by value in the launch arguments instead (the same numbers, so both forms give the same bytes).
struct FrameRow {
    long long offset;           // of the frame's first byte in the frame buffer (a multiple of 16)
    int H0, W0, new_h, new_w, top, left;
    double scale_x, scale_y;    // OpenCV resize(): 1 / (new / orig)
    float gain, padx, pady;     // scale_boxes: computed in double, cast once
    int pad;                    // zero: equal inputs pack to equal bytes
};
static_assert(sizeof(FrameRow) == 64, "frame table rows are 64 bytes");
constexpr int kFrameTableMagic = 0x31544656;    // "VFT1"
struct FrameTableHeader {
    int magic, B, H, W, max_H0, max_W0;
    long long total_bytes;      // of the frame buffer the offsets were checked against
    int pad[8];
};
static_assert(sizeof(FrameTableHeader) == 64, "the rows of a frame table stay 64-byte aligned");
// One frame of a windowed predict (vti_pack_windows): `crop` is the row vti_pack_frames would pack for the contiguous copy of the
// window (H0 x W0 = the window's h x w; offset = the byte of the window's first pixel inside the frame buffer, of any alignment),
// then the frame the window lies in and the window's origin in it.  A window table is a FrameTableHeader with kWindowTableMagic
// (max_H0, max_W0: of the full frames) followed by B rows.
struct WindowRow {
    FrameRow crop;
    long long frame_offset;     // of the FRAME's first byte (a multiple of 16)
    int H0, W0;                 // the frame's size
    int x0, y0;                 // the window's origin in the frame
    int pad[10];                // zero
};
static_assert(sizeof(WindowRow) == 128, "window table rows are 128 bytes");
constexpr int kWindowTableMagic = 0x31545756;   // "VWT1"
void letterbox_geom(int H0, int W0, int H, int W, int& new_h, int& new_w, int& top, int& left);
void frame_row_fill(int H, int W, int H0, int W0, long long offset, FrameRow& r);      // geometry of one frame on the H x W canvas (host)

// The NMS table (vti_pack_nms_table): an NmsTableHeader, then one NmsRow per row.  The class set is a bit mask of kNmsMaskWords * 32
// bits (VTI_NMS_TABLE_MAX_CLASSES); filter == 0 means every class and the mask is then all zero, so equal settings pack to equal bytes.
constexpr int kNmsMaskWords = VTI_NMS_TABLE_MAX_CLASSES / 32;
struct NmsRow {
    float conf;
    int max_det;
    double iou;
    int agnostic, filter;
    int pad[2];                 // zero
    unsigned mask[kNmsMaskWords];
};
static_assert(sizeof(NmsRow) == 32 + 4 * kNmsMaskWords && sizeof(NmsRow) % 16 == 0, "NMS table rows stay 16-byte aligned");
constexpr int kNmsTableMagic = 0x31544e56;      // "VNT1"
struct NmsTableHeader {
    int magic, n_rows, nc, mask_words;
    int pad[12];
};
static_assert(sizeof(NmsTableHeader) == 64, "the rows of an NMS table follow a 64-byte header");
struct NmsTable {               // what the NMS launch takes: the device rows, the per-frame row index (nullptr: row 0), the row count
    const NmsRow* rows = nullptr;
    const int* row_of_frame = nullptr;
    int n_rows = 0;
};

// post-processing (post.hip)
// table == nullptr: B frames of H0 x W0 back to back (vti_letterbox); else frame b is row b of the device table (vti_letterbox_frames)
hipError_t launch_letterbox(const uint8_t* frames, int B, int H0, int W0, const FrameRow* table, uint8_t* out, int H, int W,
                            hipStream_t st);
size_t nms_workspace_bytes(int B, int A);
// `best`: optional [B, A, 2] floats (max class score, its first class index as a float) that the producer of `pred` wrote beside it
// (vti_forward_scored): the candidate filter then reads 8 bytes per anchor instead of the nc class scores
// table.rows != nullptr (vti_set_nms_table): conf, iou, agnostic, the class set and min(row.max_det, max_det) of frame b come from row
// table.row_of_frame[b] (nullptr: row 0) of the device table; max_det stays the row stride of dets and the upper bound
hipError_t launch_nms(const float* pred, const float* best, int B, int A, int nc, int nm, float conf, double iou, int max_det,
                      int agnostic, float* dets, int* counts, void* ws, hipStream_t st, NmsTable table = NmsTable{});
hipError_t launch_anchor_best(const float* pred, int B, int A, int nc, int nm, float* best, hipStream_t st);   // the same pairs from pred itself
float* nms_workspace_best(void* ws, int B, int A);       // [B, A, 2] floats at the end of the NMS workspace (vti_predict's own pair buffer)
hipError_t launch_masks(int dtype, const float* dets, const int* counts, const void* proto, int B, int max_det,
                        int nm, int Hp, int Wp, int H, int W, int mode, int packing, uint8_t* masks,
                        int capacity, int* offsets, void* ws, hipStream_t st, int wgs_per_cu = 0);      // wgs_per_cu: RunOptions.mask_wgs_per_cu
size_t masks_workspace_bytes(int capacity, int H, int W);
// retina_masks (process_mask_native): out = {top, bottom, left, right, row_bytes, slot_bytes} of frame-size masks from Hp x Wp
// prototypes (host only; -1 for shapes it cannot describe); the launcher needs the frame-px boxes of vti_scale_boxes
int native_mask_layout(int Hp, int Wp, int H0, int W0, int packing, int out[6]);
hipError_t launch_masks_native(int dtype, const float* dets, const float* xyxy, const int* counts, const void* proto, int B, int max_det,
                               int Hp, int Wp, int H0, int W0, int mode, int packing, uint8_t* masks, int capacity, int* offsets,
                               void* ws, hipStream_t st);
// vti_masks_native_frames: frame b's slots have the layout native_mask_layout(H0[b], W0[b], VTI_PACK_BITS) gives and lie back to back,
// frame-major, from bases[b] on (i64 [B + 1], written with offsets by the launch's prologue); a slot is live iff it ends at or before
// capacity_bytes.  rows: the device frame table's rows.  native_table_bytes<Row> (host; Row: FrameRow or WindowRow): the worst case of
// max_det slots per frame of a packed host table whose rows were validated -- for a window table, slots of the FULL frames -- and
// the tiles of the work list; -1 for a row native_mask_layout cannot describe.
template <class Row>
long long native_table_bytes(const void* host_table, int Hp, int Wp, int max_det, long long* tiles);
size_t masks_native_frames_workspace_bytes(int B);
hipError_t launch_masks_native_frames(int dtype, const float* dets, const float* xyxy, const int* counts, const void* proto,
                                      const FrameRow* rows, int B, int max_det, int Hp, int Wp, int mode, uint8_t* masks,
                                      long long capacity_bytes, int* offsets, long long* bases, void* ws, hipStream_t st);
// The window forms (vti_*_windows; rows: the device window table's rows).  Letterbox: the canvas of the contiguous crops, read in
// place.  Scale boxes: the crop's boxes plus the window's origin (frame px).  Native masks: the ragged buffer of the FULL frames
// (launch_masks_native_frames' layout, offsets, bases and liveness), each instance's crop mask placed at the window's origin; the
// boxes are recomputed in window px from `dets`.
hipError_t launch_letterbox_windows(const uint8_t* frames, int B, const WindowRow* rows, uint8_t* out, int H, int W, hipStream_t st);
hipError_t launch_scale_boxes_windows(const float* dets, const int* counts, int B, int max_det, int nm, const WindowRow* rows,
                                      float* xyxy, hipStream_t st);
hipError_t launch_masks_native_windows(int dtype, const float* dets, const int* counts, const void* proto, const WindowRow* rows, int B,
                                       int max_det, int Hp, int Wp, int mode, uint8_t* masks, long long capacity_bytes, int* offsets,
                                       long long* bases, void* ws, hipStream_t st);
// table != nullptr: gain, pads and clip bounds of frame b from row b of the device table (H0, W0 unused)
hipError_t launch_scale_boxes(const float* dets, const int* counts, int B, int max_det, int nm, int H, int W,
                              int H0, int W0, const FrameRow* table, float* xyxy, hipStream_t st);
hipError_t launch_mask_to_frame(const uint8_t* masks, int n, int H, int W, int H0, int W0, uint8_t* bitmaps,
                                int* nonzero, hipStream_t st);
hipError_t launch_union_envelope(const uint8_t* bitmaps, const int* select, int nsel, int H0, int W0,
                                 uint8_t* uni, int* envelope, hipStream_t st);
hipError_t launch_mask_stats(const uint8_t* bitmaps, int n, int H0, int W0, long long* stats, hipStream_t st);

// consumer.hip: reductions on bit-packed masks, pixel -> world geometry, 1-D 2-means
hipError_t launch_mask_stats_bits(const uint8_t* bits, int n, const int* n_live, int H, int W, int H0, int W0, long long* stats,
                                  hipStream_t st);
hipError_t launch_envelope_bits(const uint8_t* bits, const int* offsets, const float* dets, int B, int max_det, int nm,
                                int capacity, int cls, int H, int W, int H0, int W0, int* envelope, hipStream_t st);
hipError_t launch_pixels_to_world(const double* uv, int n, const double* K, const double* dist, const double* R,
                                  const double* t, double* xyz, int* valid, hipStream_t st);
hipError_t launch_kmeans1d2(const double* values, const int* counts, int B, int max_n, int max_iters, int* labels,
                            double* centers, hipStream_t st);
// vti_measure: per-slot moments, the ROI-kept fabric envelope and the per-frame record; scratch carved as measure_scratch_layout
void measure_scratch_layout(int B, int capacity, int W0, size_t off[3], size_t& total);    // stats i64 [cap,5] | raw i32 [cap] | env i32 [B,W0]
// a camera-table row (vti_measure_pack_cameras): its size and the packing of one validated struct (host)
size_t measure_camera_row_bytes();
void measure_pack_camera(const vti_measure_params& p, void* row);

// ---- what the measure, checker and annotate entry points hand down: each fills these once (host only, never kernel parameters) ----
// The output set of a predict call.  bases != nullptr: the masks are the ragged rows of vti_masks_native_frames (i64 [B + 1], with a
// frame table and native = 1 only), and a slot that ends past capacity_bytes is an empty mask.
struct OutputSet {
    const uint8_t* masks; int native; const float* dets; const float* xyxy; const int* counts; const int* offsets;
    int B, max_det, capacity;
    const long long* bases; long long capacity_bytes;
};
// Which camera serves frame b: row cam_of_frame[b] (nullptr: row 0) of a packed device table of n_cams rows.  All zero: the one
// settings struct of the call serves every frame.
struct CameraChoice { const void* table; int n_cams; const int* cam_of_frame; };
struct Canvas { int nm, H, W; };                // of the ctx: mask coefficients per detection, the letterbox size
// Every frame H0 x W0; or with rows (of a device frame table, already checked against its host copy) frame b has row b's size and
// H0, W0 are the largest ones (the pitches of the scratch)
struct FrameSizes { int H0, W0; const FrameRow* rows; };
// A measurement: the caller's scratch (measure_scratch_layout) and the four output rows
struct MeasureResult { void* scratch; size_t scratch_bytes; double* frame_f64; int* frame_i32; double* stitch_f64; int* stitch_i32; };
// What a drawing call takes beside the output set: the measurement's rows, the selection (host_select checked, dev_select its device
// copy), the pictures and their status, the scratch (annotate_layout)
struct DrawInputs {
    const int* frame_i32; const double* stitch_f64; const int* stitch_i32;
    const int* host_select; const int* dev_select; int n_sel, max_points;
    uint8_t* out; int* status; void* scratch; size_t scratch_bytes;
};

// p != nullptr: one camera for every frame; else cams.  fs.rows != nullptr: fs.W0 is also the pitch of the envelope rows in the scratch
hipError_t launch_measure(const vti_measure_params* p, const CameraChoice& cams, OutputSet o, const Canvas& cv, const FrameSizes& fs,
                          const MeasureResult& r, hipStream_t st);

// vti_measure_checker (Utils/check_stitch_distance.py) and its rig forms: vti_measure's inputs, scratch layout and outputs.
// p != nullptr: one camera and one frame size; else the arguments as launch_measure takes them (the table's rows are checker_pack's)
hipError_t launch_measure_checker(const vti_checker_params* p, const CameraChoice& cams, OutputSet o, const Canvas& cv,
                                  const FrameSizes& fs, const MeasureResult& r, hipStream_t st);
// one validated vti_checker_params -> the CameraRow (measure_dev.h) the checker's kernels take by value (host)
void checker_pack(const vti_checker_params& p, void* row);

// polygons.hip: vti_mask_polygons (Results.masks.xy).  The grid is VTI_POLY_WORKGROUPS persistent workgroups, each with its own
// labelling area of the scratch: parent i32 [R_max] | runs u32 [R_max] | row_start i32 [H+1] | image u64 [H, WW] (only when the
// image does not fit in LDS), R_max = H * ceil(W/2) (the most runs an H x W mask can have).  The scratch starts with a 256-byte
// header whose first int32 is the status word.
#define VTI_POLY_WORKGROUPS 128
struct PolyLayout {
    int WW;                    // 64-bit words per image row
    bool in_lds;               // the H x WW image is kept in LDS
    int forms;                 // bit 0: a geometry of the layout keeps its image in LDS, bit 1: one keeps it in the scratch
    size_t img_bytes, off_runs, off_rows, off_img, area_bytes, total;
};
void mask_polygons_layout(int H, int W, int row_bytes, PolyLayout& L);
// The layout for slots of n geometries (vti_mask_polygons_frames: the frames of a table): every part of the area is the largest any of
// them needs, the image part being that of the geometries whose image does not fit the LDS.  n = 1 is mask_polygons_layout.
void mask_polygons_layout_frames(const int* H, const int* W, int n, PolyLayout& L);
// scale_coords' gain and pads come from (H, W) and (H0, W0): polygons_dev.h, poly_map.
hipError_t launch_mask_polygons(const uint8_t* masks, int n, const int* n_live, int H, int W, int row_bytes, int H0, int W0,
                                int strategy, void* scratch, int* offsets, float* points, long long max_points, hipStream_t st);
// vti_mask_polygons_frames.  bases == nullptr: the slots are letterbox masks of H x W (row_bytes W / 8) and slot s of frame b
// (slot_offsets[b] <= s < slot_offsets[b + 1]) maps to that frame's H0 x W0; else they are vti_masks_native_frames' ragged rows, traced at
// H0[b] x W0[b].  L: mask_polygons_layout_frames of the host table's geometries.  Live: s < min(slot_offsets[B], capacity).
hipError_t launch_mask_polygons_frames(const uint8_t* masks, const long long* bases, long long capacity_bytes, const int* slot_offsets,
                                       const FrameRow* rows, int B, int capacity, int H, int W, const PolyLayout& L, int strategy,
                                       void* scratch, int* offsets, float* points, long long max_points, hipStream_t st);

// annotate.hip: vti_annotate (process_frame's annotated frame).  The scratch holds, per selected frame: the display list (3 + 7 *
// max_det records of 32 bytes), 16 ints of counts, the envelope's points int2 [W0], the outline's vertices int2 [max_points], the
// fabric union u64 [H0, WW] and one labelling area of the contour tracer (parent | runs | row_start, as polygons.hip's).
struct AnnotateLayout {
    int WW;                    // 64-bit words per union row
    bool in_lds;               // the tracer keeps the union in LDS
    size_t off_recs, off_meta, off_env, off_cont, off_union, off_areas, area_bytes, off_runs, off_rows, total;
};
void annotate_layout(int n_sel, int max_det, int H0, int W0, int max_points, AnnotateLayout& L);
// vti_annotate_frames: the rows of the device frame tables of dev_frames and dev_out; H0, W0 passed to launch_annotate are then the
// largest selected ones (the pitches of the scratch), native is 0.  any_lds / any_global: a selected frame's union fits / does not fit
// the tracer's LDS image (which outline instantiations are launched); max_px: the most pixels a selected frame has (the raster grid).
struct AnnotateFrames { const FrameRow* rows_in; const FrameRow* rows_out; bool any_lds, any_global; long long max_px; };
// frames: u8 [B, H0, W0, 3], or with fr the flat buffer of its rows_in; cams: a packed camera table in device memory
hipError_t launch_annotate(const uint8_t* frames, int H0, int W0, const CameraChoice& cams, const OutputSet& o, const Canvas& cv,
                           const DrawInputs& d, hipStream_t st, const AnnotateFrames* fr = nullptr);
// vti_annotate_checker (the stitch-distance checker's picture): the same scratch and the same outline and raster kernels behind a
// prep kernel of its own; the rows are vti_measure_checker's.  p != nullptr: the settings travel by value; else they are cams' row of
// the checker's camera table in device memory, and fr is launch_annotate's
hipError_t launch_annotate_checker(const vti_checker_params* p, const uint8_t* frames, int H0, int W0, const CameraChoice& cams,
                                   const OutputSet& o, const Canvas& cv, const DrawInputs& d, hipStream_t st,
                                   const AnnotateFrames* fr = nullptr);

// stamp.hip: vti_stamp / vti_stamp_frames (the text of the annotated pictures as 1-bit stamps).  The stamp table, host and device
// copy alike: the header | n_pictures picture rows | n_stamps records.  Picture k owns the records [begin, end); the ranges follow each
// other without a gap, so that the records are in picture order and, within a picture, in painting order.
constexpr int kStampTableMagic = 0x31545356;    // "VST1"
constexpr int kStampMaxSide = 8192;             // vti_annotate's limit
constexpr int kStampMaxPitch = 65536;           // words per stamp row
constexpr long long kStampMaxWords = 1ll << 40;
struct StampHeader {
    int magic, n_pictures, n_stamps, pad0;
    long long n_words;          // of the bit buffer the records were checked against
    int pad[10];
};
static_assert(sizeof(StampHeader) == 64, "the rows of a stamp table stay 16-byte aligned");
struct StampPicture { int H0, W0, begin, end; };
struct StampRec {
    long long offset;           // of the stamp's first word in the bit buffer
    int x, y, w, h, pitch;      // the rectangle in its picture; words per row
    unsigned colour;            // B | G << 8 | R << 16
};
static_assert(sizeof(StampPicture) == 16 && sizeof(StampRec) == 32, "a stamp record is two 16-byte vectors");
// pictures: u8 [n,H0,W0,3], or with `rows` (the device frame table's rows) the flat buffer of `total_bytes` bytes whose frame k is
// picture k (H0, W0 are then the largest frame's, max_px the most pixels a frame has).  table: the device copy of the stamp table.
hipError_t launch_stamp(uint8_t* pictures, int n, int H0, int W0, const FrameRow* rows, long long total_bytes, long long max_px,
                        const void* table, int n_stamps, const uint32_t* bits, long long n_words, hipStream_t st);

// overlay.hip: vti_overlay (the model-check viewer's picture).  The scratch holds: 16 ints of counters per selected frame | the contour
// vertices int4 [n_sel, max_points] | the owner planes (8 words per 32-bit mask word, for the larger of a native and a letterbox mask
// slot) per selected frame | min(max_det, 16) labelling areas per selected frame (parent | runs | row_start as polygons.hip's, then
// the instance's bitmap u64 [H0, WW]).
struct OverlayLayout {
    int WW, groups;            // 64-bit words per bitmap row; contour workgroups (areas) per selected frame
    bool in_lds;               // the tracer keeps the bitmap in LDS
    size_t off_meta, off_cont, off_planes, off_areas, plane_words, area_bytes, off_runs, off_rows, off_img, total;
};
void overlay_layout(int n_sel, int max_det, int H0, int W0, int Hm, int Wm, int max_points, OverlayLayout& L);
// vti_overlay_frames: the rows of the device frame tables of dev_frames and dev_out; H0, W0 passed to launch_overlay are then the largest
// selected ones (the pitches of the scratch).  native = 1: the masks are the ragged rows of vti_masks_native_frames -- bases (device,
// i64 [B + 1]), capacity_bytes, and max_slot_words, the most 32-bit words a selected frame's slot has (the owner grid).  any_lds /
// any_global: a selected frame's bitmap fits / does not fit the tracer's LDS image (which contour instantiations are launched);
// max_px: the most pixels a selected frame has (the raster grid).
struct OverlayFrames {
    const FrameRow* rows_in; const FrameRow* rows_out; const long long* bases; long long capacity_bytes, max_slot_words;
    bool any_lds, any_global; long long max_px;
};
// palette: host, 3 * n_colours bytes (BGR); select: the device copy of the (host-checked) selection; H, W: the letterbox mask size
hipError_t launch_overlay(const uint8_t* frames, int B, int H0, int W0, const uint8_t* masks, int native, const float* dets,
                          const float* xyxy, const int* counts, const int* offsets, int max_det, int nm, int capacity, int H, int W,
                          const int* plates, const uint8_t* palette, int n_colours, float alpha, float beta, const int* select,
                          int n_sel, int mode, const uint8_t* annotated, int max_points, uint8_t* out, int* status, void* scratch,
                          hipStream_t st, const OverlayFrames* fr = nullptr);

// jpeg.hip: vti_encode_jpeg (the saved JPEG).  The scratch holds: the header's bytes (1 KiB) | bit total u64 [n] | file size i64 [n] |
// coefficients i16 [n, MCUs, 6, 64] | block bit positions u64 [n, blocks] | the unstuffed stream, NC chunks of 4096 bytes per frame
// (the worst case of 1658 bits per block) | 0xFF count u32 [n, NC].
struct JpegLayout {
    int mr, mc;                // MCU rows and columns of a frame
    long long nblk;            // blocks per frame in the scan, dummy blocks included (6 per MCU)
    long long stream_bytes;    // the most bytes a frame's unstuffed stream can have
    long long NC;              // 4096-byte chunks that hold them
    long long max_file;        // the most bytes one file can have
    size_t off_fbits, off_fsize, off_coef, off_bitpos, off_stream, off_chunk, total;
};
// false on sizes outside 1 <= n, 1 <= H0, W0 <= 8192, n * MCUs <= 2^28
bool encode_jpeg_layout(long long n, int H0, int W0, JpegLayout& L);
void encode_jpeg_header(int H0, int W0, int quality, uint8_t out[624]);      // SOI .. SOS: 623 bytes and one of padding
hipError_t launch_encode_jpeg(const uint8_t* frames, int n, int H0, int W0, int rgb, int quality, void* scratch, long long* offsets,
                              uint8_t* out, long long max_bytes, hipStream_t st);
// vti_encode_jpeg_frames: frame k is row k of a frame table.  MCUs, blocks and chunks are numbered through the whole batch, so the
// scratch is the uniform call's with every frame's part as long as that frame needs, behind the two prefix arrays i64 [n + 1] (MCUs,
// chunks) that the first launch builds from the device table: header bytes (1 KiB) | pm | pc | bit total | file size | coefficients |
// bit positions | streams | 0xFF counts.
struct JpegFramesLayout {
    int n;
    long long n_mcu, n_chunk;  // of the whole batch
    long long max_bytes;       // the sum of the frames' max_file
    size_t off_pm, off_pc, off_fbits, off_fsize, off_coef, off_bitpos, off_stream, off_chunk, total;
};
// host_table: a packed frame table (its rows already validated); false when a frame is outside vti_encode_jpeg's limits
bool encode_jpeg_frames_layout(const void* host_table, JpegFramesLayout& L);
hipError_t launch_encode_jpeg_frames(const uint8_t* frames, const void* host_table, const FrameRow* rows, int rgb, int quality,
                                     void* scratch, long long* offsets, uint8_t* out, long long max_bytes, hipStream_t st);

// jpeg_decode.hip: vti_decode_jpeg (JPEG files -> frames).  The host parses every header; a descriptor table is a JpegDecHeader
// followed by one JpegDecRow per file.  The scratch holds per file, each part rounded up to 256 bytes: the segment states (entry u64 |
// exit u64 | (markers, blocks) u32 x 2 | their scan u32 x 2, 32 bytes per segment), the coefficients i16 [blocks, 64] and the Y, Cb, Cr
// planes u8 (64 bytes per block).
// host: one file's header -> R (offsets relative to the file; layout fields zero); 0, VTI_ERR_ARG or VTI_ERR_UNSUPPORTED with the reason
int decode_jpeg_parse(const uint8_t* d, long long n, JpegDecRow& R, std::string& err);
size_t decode_jpeg_scratch_of(JpegDecRow& R, size_t at);      // sets R's scratch offsets from `at` on (needs nseg, nblk); -> the end
// host: every value of a row a kernel forms an address from, against the header's sizes; scratch_at runs along the rows
bool decode_jpeg_row_ok(const JpegDecRow& R, const JpegDecHeader& H, size_t& scratch_at, std::string& why);
hipError_t launch_decode_jpeg(const uint8_t* files, const void* host_table, const void* dev_table, int n, int rgb, uint8_t* out, int* info,
                              void* scratch, hipStream_t st);

// raw camera frames -> BGR / RGB (rawframes.hip); the arithmetic and the table rows are rawframes_dev.h's
hipError_t launch_convert_raw(const uint8_t* raw, int fmt, int B, int H0, int W0, int rgb, uint8_t* out, hipStream_t st);
// frame b: row b of the device raw table, written at row b's offset of the device frame table; max_items: the largest frame's
hipError_t launch_convert_raw_frames(const uint8_t* raw, const void* dev_raw_table, const FrameRow* dev_frame_rows, int n, int max_items,
                                     int rgb, uint8_t* out, hipStream_t st);

// plan.cpp: launch geometry for one conv (tile, wave split, LDS) -- th/tw/wn/nrep > 0 force a choice
void choose_conv_cfg(const PlanOptions& opt, int dtype, const ConvRow& r, bool conv0, int max_batch, ConvCfg& c,
                     int th = 0, int tw = 0, int wn = 0, int nrep = 0, bool allow_pk = true);
// weights.cpp: one conv's weights -> fragment order; dst_w has cfg.nchunks*ntiles_n*taps KiB, dst_b ntiles_n*16 floats
void pack_conv(int dtype, const ConvRow& r, bool conv0, const ConvCfg& c, const float* w, const float* b,
               uint8_t* dst_w, float* dst_b, int cin_off = 0, float* alpha = nullptr);      // cin_off: the conv's input channels sit at K positions cin_off.. of the chunk; alpha: see ConvParams
size_t packed_conv_bytes(const ConvRow& r, bool conv0, const ConvCfg& c);
// fused second stage: the 1x1 conv `r2` packed against the accumulator layout of a producer with nrep1 cout tiles
void pack_conv_stage2(int dtype, const ConvRow& r2, int nrep1, const float* w, const float* b, uint8_t* dst_w, float* dst_b,
                      bool natural_rows = false, float* alpha = nullptr);
size_t packed_stage2_bytes(int dtype, const ConvRow& r2, int nrep1);
// weights.cpp: parse VTIW1 + pack into MFMA fragment order (host memory)
std::string pack_weights(const Plan& plan, const void* blob, size_t nbytes,
                         std::vector<uint8_t>& wpk, std::vector<float>& bias, std::vector<float>& alpha);

}  // namespace vti
