// The text form of one launch of the forward: the launcher's name, its selector arguments and every field of its parameter block.
// tests/plan_dump_main.cpp prints the records of csrc/launch.cpp with it; the recorder of tests/golden/launch_params_recorder.patch
// printed the arguments of the launch_* calls of the commit before csrc/launch.cpp with it, which is what
// tests/golden/launch_params.json holds.  Pointers print as hex numbers: the bindings are fake addresses k << 40 (never
// dereferenced), so a pointer reads as base plus offset, and null as 0.  Floats print with %a.
#pragma once
#include <cstdio>

#include "../vision-textile-inspection_amd/csrc/vti_internal.h"

namespace launch_dump {

// the fake bindings: the k-th base is k << 40
constexpr unsigned long long kBase = 1ull << 40;
inline char* fake_ws() { return (char*)(1 * kBase); }
inline void* fake_wpk() { return (void*)(2 * kBase); }
inline float* fake_bias() { return (float*)(3 * kBase); }
inline const uint8_t* fake_input() { return (const uint8_t*)(4 * kBase); }
inline float* fake_pred() { return (float*)(5 * kBase); }
inline void* fake_proto() { return (void*)(6 * kBase); }
inline float* fake_best() { return (float*)(7 * kBase); }
inline float fake_alpha(int conv) { return 1.f + (float)(conv + 1) / 1024.f; }      // exact in fp32, distinct per conv, never 1

inline int& op_index() { static int i = -1; return i; }      // the plan's op the next printed launch belongs to

inline unsigned long long ptr(const void* p) { return (unsigned long long)(uintptr_t)p; }

inline void print_conv_block(const vti::ConvParams& p) {
    printf(" in=%llx out=%llx res=%llx wpk=%llx bias=%llx B=%d Hin=%d Win=%d Hout=%d Wout=%d Cin=%d in_ld=%d in_coff=%d Cout=%d out_ld=%d "
           "out_coff=%d res_ld=%d res_coff=%d TH=%d TW=%d tiles_y=%d tiles_x=%d WN=%d act=%d out_f32=%d deconv_c=%d swap_rb=%d nchunks=%d "
           "ntiles_n=%d has_res=%d scalar_store=%d pw_magic=%u rw_magic=%u tw_magic=%u wpk_bytes=%u",
           ptr(p.in), ptr(p.out), ptr(p.res), ptr(p.wpk), ptr(p.bias), p.B, p.Hin, p.Win, p.Hout, p.Wout, p.Cin, p.in_ld, p.in_coff, p.Cout,
           p.out_ld, p.out_coff, p.res_ld, p.res_coff, p.TH, p.TW, p.tiles_y, p.tiles_x, p.WN, p.act, p.out_f32, p.deconv_c, p.swap_rb,
           p.nchunks, p.ntiles_n, p.has_res, p.scalar_store, p.pw_magic, p.rw_magic, p.tw_magic, p.wpk_bytes);
    printf(" w2=%llx bias2=%llx out2=%llx Cout2=%d ntiles2=%d out2_ld=%d out2_coff=%d act2=%d out2_f32=%d scalar_store2=%d nat2=%d "
           "out2_bstride=%d nt=%d wreg=%d best=%llx dfl_stride=%a",
           ptr(p.w2), ptr(p.bias2), ptr(p.out2), p.Cout2, p.ntiles2, p.out2_ld, p.out2_coff, p.act2, p.out2_f32, p.scalar_store2, p.nat2,
           p.out2_bstride, p.nt, p.wreg, ptr(p.best), (double)p.dfl_stride);
    printf(" pk=%d pk_tiles=%d pk_wgs=%d pk_xcd=%d pk_depth=%d pk_wstat=%d pk_lin=%d pk_cps=%d pk_stagger=%d in_bytes=%u out_bytes=%u "
           "res_bytes=%u out2_bytes=%u in2=%llx in2_ld=%d in2_coff=%d up_C=%d in2_bytes=%u fold=%d w0=%llx bias0=%llx alpha=%a alpha2=%a "
           "alpha0=%a stamps=%llx\n",
           p.pk, p.pk_tiles, p.pk_wgs, p.pk_xcd, p.pk_depth, p.pk_wstat, p.pk_lin, p.pk_cps, p.pk_stagger, p.in_bytes, p.out_bytes,
           p.res_bytes, p.out2_bytes, ptr(p.in2), p.in2_ld, p.in2_coff, p.up_C, p.in2_bytes, p.fold, ptr(p.w0), ptr(p.bias0),
           (double)p.alpha, (double)p.alpha2, (double)p.alpha0, ptr(p.stamps));
}

inline void print_stem_l1(int dtype, const vti::ConvParams& p, bool persistent) {
    printf("op %d: launch_stem_l1 dtype=%d persistent=%d |", op_index(), dtype, (int)persistent);
    print_conv_block(p);
}
inline void print_conv(int dtype, int ks, int stride, int nrep, int mode, const vti::ConvParams& p, size_t lds) {
    printf("op %d: launch_conv dtype=%d ks=%d stride=%d nrep=%d mode=%d lds=%zu |", op_index(), dtype, ks, stride, nrep, mode, lds);
    print_conv_block(p);
}
inline void print_fold(const char* launcher, int dtype, const vti::ConvParams& p, size_t lds) {      // launch_convfold / launch_conv_pk_fold
    printf("op %d: %s dtype=%d lds=%zu |", op_index(), launcher, dtype, lds);
    print_conv_block(p);
}
inline void print_pool(int dtype, const vti::PoolParams& p) {
    printf("op %d: launch_sppf_pool dtype=%d | in=%llx out=%llx B=%d H=%d W=%d C=%d ld=%d in_coff=%d out_coff=%d\n", op_index(), dtype,
           ptr(p.in), ptr(p.out), p.B, p.H, p.W, p.C, p.ld, p.in_coff, p.out_coff);
}
inline void print_up2(int dtype, const vti::Up2Params& p) {
    printf("op %d: launch_upsample2x dtype=%d | in=%llx out=%llx B=%d H=%d W=%d C=%d in_ld=%d in_coff=%d out_ld=%d out_coff=%d\n",
           op_index(), dtype, ptr(p.in), ptr(p.out), p.B, p.H, p.W, p.C, p.in_ld, p.in_coff, p.out_ld, p.out_coff);
}
inline void print_decode(const char* launcher, const vti::DecodeParams& p) {                         // launch_decode / launch_box_decode
    printf("op %d: %s |", op_index(), launcher);
    for (int l = 0; l < 3; ++l)
        printf(" box%d=%llx cls%d=%llx mc%d=%llx H%d=%d W%d=%d stride%d=%d a0_%d=%d", l, ptr(p.box[l]), l, ptr(p.cls[l]), l, ptr(p.mc[l]), l,
               p.H[l], l, p.W[l], l, p.stride[l], l, p.a0[l]);
    printf(" B=%d A=%d nc=%d nm=%d reg_max=%d pred=%llx\n", p.B, p.A, p.nc, p.nm, p.reg_max, ptr(p.pred));
}
inline void print_anchor_best(const float* pred, int B, int A, int nc, int nm, const float* best) {
    printf("after the ops: launch_anchor_best | pred=%llx B=%d A=%d nc=%d nm=%d best=%llx\n", ptr(pred), B, A, nc, nm, ptr(best));
}
inline void print_conv_info(int i, const vti_conv_info& o) {      // vti_conv_at's launch geometry of conv i
    printf("conv %d: %s tile=%dx%d waves_n=%d nrep=%d lds_bytes=%d fused=%d persistent=%d\n", i, o.name, o.tile_h, o.tile_w, o.waves_n,
           o.nrep, o.lds_bytes, o.fused, o.persistent);
}
inline void print_refusal(int status, const char* text) { printf("op %d: refused (status %d): %s\n", op_index(), status, text); }

}  // namespace launch_dump
