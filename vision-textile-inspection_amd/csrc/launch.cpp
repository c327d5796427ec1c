// The launch parameters of the forward, host only (no kernel, no HIP call): what goes into the parameter block of each op of the
// plan and which launcher takes it, as a function of (Plan, Op, B, swap_rb, RunOptions, Bindings).  vti_api.cpp issues the records
// on the streams; tests/test_plan_golden.py pins them field by field (tests/golden/launch_params.json).  Each op form sits beside
// the launch geometry vti_conv_at reports of the convs it runs.
#include <cstring>

#include "vti_internal.h"

namespace vti {

void* buf_ptr(const Plan& P, const Bindings& b, int buf) {
    if (buf == 0) return (void*)b.input;
    if (buf == P.proto_buf_c) return b.proto;
    return b.ws + P.bufs[buf].off;
}

// Delay units (x 1024 cycles) of the staggered persistent 3x3 launches.  h2 only by default: -2.6 ... -4.2 % per forward on five of
// seven boxes (A/B on one box at a time), +0.8 % on the two fastest; fp16: +0.2 ... +1 % on a fast box, fp32: nothing.  VTI_PK_STAGGER=n overrides.
static int stagger_units(const RunOptions& run, int dtype) { return run.pk_stagger >= 0 ? run.pk_stagger : (dtype == VTI_H2 ? 10 : 0); }

// ---- the arithmetic every form shares --------------------------------------------------------------------------------------------
// Stores of n channels at channel offset coff into rows of ld channels: 16-byte vector stores need all three to be multiples of 4.
static int scalar_store(int n, int ld, int coff) { return (n % 4 || ld % 4 || coff % 4) ? 1 : 0; }
static unsigned magic(unsigned n) { return (unsigned)((0x100000000ull + n - 1) / n); }      // ceil(2^32 / n): division-free indexing
static void set_tiles(ConvParams& p, int TH, int TW) {
    p.TH = TH; p.TW = TW;
    p.tiles_y = (p.Hout + TH - 1) / TH; p.tiles_x = (p.Wout + TW - 1) / TW;
}
// the grid of a persistent launch over `tiles` tiles (pk_grid); from 8 workgroups on each XCD walks a contiguous range of them
static void set_pk_grid(ConvParams& p, const RunOptions& run, size_t tiles, int wgpc, int gy) {
    p.pk_tiles = (int)tiles;
    p.pk_wgs = pk_grid(p.pk_tiles, wgpc, gy, run.pk_max_wgs);      // tests: force many tiles per workgroup
    p.pk_xcd = p.pk_wgs >= 8 ? 1 : 0;
}
// Bytes of a [px, ld] tensor of es-byte elements.  The persistent kernels range-check with 32-bit byte counts and mark out-of-range
// lanes with 2^31, so a tensor they address must stay below that.
static size_t tensor_bytes(size_t px, int ld, size_t es) { return px * ld * es; }
static bool below_2g(size_t bytes) { return bytes < 0x80000000ull; }

static LaunchRec& conv_form(LaunchRec& L, Launcher fn, const ConvRow& r, int dtype) {
    L.fn = fn; L.name = r.name.c_str(); L.dtype = dtype;
    L.ks = L.stride = L.nrep = L.mode = 0; L.lds = 0; L.persistent = false;
    memset(&L.conv, 0, sizeof L.conv);
    return L;
}
static void own_geometry(const ConvCfg& g, vti_conv_info* o) {      // the conv an op is named after: the chosen configuration
    o->tile_h = g.TH; o->tile_w = g.TW; o->waves_n = g.WN; o->nrep = g.NREP;
    o->lds_bytes = (int32_t)g.lds; o->persistent = g.pk;      // 1: conv3_pk, 2: conv1_pk, 3: bneck_pk
}

// ---- the fused 1x1 second stage of an op (op.fused): its weights, where it writes and how it stores -----------------------------------
// wpk_off / bias_off: the stage's pack; grid: the conv whose output grid the stage's rows follow
static void fill_stage2(const Plan& P, const Bindings& b, ConvParams& p, const Op& op, size_t wpk_off, size_t bias_off, const ConvRow& grid) {
    const ConvCfg& g = op.cfg;
    const Buf& o2 = P.bufs[op.out2.buf];
    p.w2 = (const char*)b.wpk + wpk_off; p.bias2 = b.bias + bias_off; p.alpha2 = b.alpha[op.fused];
    p.out2 = buf_ptr(P, b, op.out2.buf);
    p.Cout2 = g.gemm_n2; p.ntiles2 = g.ntiles2; p.out2_ld = o2.C; p.out2_coff = op.out2.coff;
    p.act2 = P.convs[op.fused].kind == 0; p.out2_f32 = op.out2_f32 ? 1 : 0;
    p.scalar_store2 = scalar_store(g.gemm_n2, o2.C, op.out2.coff);
    p.nat2 = op.nat2;           // fp32 NHWC output (e.g. the h2 engine's proto): stage-2 weights are packed with natural rows
    p.out2_bstride = grid.h_out * grid.w_out;
}
static void stage2_geometry(const Op& op, vti_conv_info* o) {       // runs inside its producer's kernel, on that kernel's geometry
    o->tile_h = op.cfg.TH; o->tile_w = op.cfg.TW; o->waves_n = 1; o->nrep = op.cfg.ntiles2; o->lds_bytes = 0; o->fused = 1;
}

// ---- stem + layer 1 in one kernel (stem_l1_kernel: 16 x 20 layer-1 output tiles, 2 n-tiles), + the 1x1 conv after layer 1 ---------------
static void fill_stem_l1(const Plan& P, const Op& op, int B, int swap_rb, const RunOptions& run, const Bindings& b, LaunchRec& L) {
    const ConvRow& r = P.convs[op.conv];
    const ConvRow& r1 = P.convs[op.fused_l1];
    const ConvCfg& g = op.cfg;
    ConvParams& q = conv_form(L, LAUNCH_STEM_L1, r, P.desc.dtype).conv;
    L.persistent = !run.stem_not_persistent;
    q.in = b.input; q.B = B; q.Hin = r.h_in; q.Win = r.w_in; q.Hout = r1.h_out; q.Wout = r1.w_out;
    q.Cin = 16; q.Cout = r1.c2; q.ntiles_n = 2; q.act = 1; q.swap_rb = swap_rb ? 1 : 0;
    q.out = buf_ptr(P, b, op.out2.buf); q.out_ld = P.bufs[op.out2.buf].C; q.out_coff = op.out2.coff;
    q.wpk = (const char*)b.wpk + g.wpk_off2; q.bias = b.bias + g.bias_off2;     // layer 1
    q.w0 = (const char*)b.wpk + g.wpk_off; q.bias0 = b.bias + g.bias_off;       // stem
    q.alpha = b.alpha[op.fused_l1]; q.alpha0 = b.alpha[op.conv]; q.alpha2 = 1.f;
    if (op.fused >= 0) {    // layer 1 itself is not stored (out2 = that conv's view); its rows follow layer 1's grid
        q.out = nullptr;
        fill_stage2(P, b, q, op, g.wpk_off3, g.bias_off3, r1);
    }
    int th, tw;
    stem_l1_tile(&th, &tw);
    set_tiles(q, th, tw);
    q.WN = 1;
    q.scalar_store = scalar_store(q.Cout, q.out_ld, q.out_coff);
}
static void stem_l1_geometry(const Op& op, int i, vti_conv_info* o) {
    if (op.conv == i) return own_geometry(op.cfg, o);
    if (op.fused == i) stage2_geometry(op, o);
    else { o->waves_n = 1; o->nrep = 2; o->lds_bytes = 0; o->fused = 1; }      // layer 1
    stem_l1_tile(&o->tile_h, &o->tile_w);
}

// ---- ConvTranspose2d(2,2) + 3x3 + fused 1x1 as four 2x2 convs on the low-resolution map (per tile, or on the persistent schedule) ------
static void fill_fold(const Plan& P, const Op& op, int B, const RunOptions& run, const Bindings& b, LaunchRec& L) {
    const ConvRow& ru = P.convs[op.fold];
    const ConvCfg& g = op.cfg;
    ConvParams& q = conv_form(L, g.pk ? LAUNCH_CONV_PK_FOLD : LAUNCH_CONVFOLD, P.convs[op.conv], P.desc.dtype).conv;
    L.lds = g.lds;
    q.in = buf_ptr(P, b, op.in.buf); q.B = B; q.Hin = ru.h_in; q.Win = ru.w_in; q.Hout = ru.h_in; q.Wout = ru.w_in;
    q.Cin = ru.c1; q.in_ld = P.bufs[op.in.buf].C; q.in_coff = op.in.coff; q.Cout = g.gemm_n; q.act = 1; q.fold = 1; q.pk_lin = run.pk_linear_map;
    set_tiles(q, g.TH, g.TW);
    q.WN = 4; q.nt = g.threads;
    q.nchunks = g.nchunks; q.ntiles_n = g.ntiles_n;
    q.pw_magic = magic((unsigned)(g.TW + 2));
    q.tw_magic = magic((unsigned)g.TW);
    q.wpk = (const char*)b.wpk + g.wpk_off; q.bias = b.bias + g.bias_off; q.wpk_bytes = (unsigned)packed_fold_bytes(g);
    q.alpha = b.alpha[op.conv]; q.alpha0 = 1.f;
    fill_stage2(P, b, q, op, g.wpk_off2, g.bias_off2, P.convs[op.conv]);      // the op's output grid: the 2x map
    if (g.pk) {             // persistent schedule: composed weights resident in LDS, tiles walked per XCD
        q.pk = 1; q.pk_depth = g.pk_depth; q.in_bytes = (unsigned)tensor_bytes((size_t)B * q.Hin * q.Win, q.in_ld, P.esize);
        set_pk_grid(q, run, (size_t)B * q.tiles_y * q.tiles_x, 1, 1);
    }
}
static void fold_geometry(const Op& op, int i, vti_conv_info* o) {
    if (op.conv == i) return own_geometry(op.cfg, o);
    if (op.fused == i) return stage2_geometry(op, o);
    // the ConvTranspose folded into the following 3x3: never materialised (`fused` stays 0: that flag means "runs inside the PREVIOUS row's kernel")
    o->tile_h = op.cfg.TH; o->tile_w = op.cfg.TW; o->persistent = op.cfg.pk; o->waves_n = 4; o->nrep = op.cfg.NREP; o->lds_bytes = 0;
}

// ---- one conv of the table, per tile or persistent (launch_conv) ---------------------------------------------------------------------
// The plain launch of a row with a configuration: the conv form's base, and all of vti_debug_conv2d's.
void conv_record(const RunOptions& run, int dtype, const ConvRow& r, const ConvCfg& g, int B, const void* in, int in_ld, int in_coff,
                 void* out, int out_ld, int out_coff, const void* res, int res_ld, int res_coff, const void* wpk, const float* bias,
                 float alpha, bool out_f32, int swap_rb, LaunchRec& L) {
    const bool deconv = r.kind == 2, conv0 = r.c1 == 3;
    const int ks = deconv ? 1 : r.k, st = deconv ? 1 : r.s;
    ConvParams& p = conv_form(L, LAUNCH_CONV, r, dtype).conv;
    L.ks = ks; L.stride = st; L.nrep = g.NREP; L.mode = conv0 ? 1 : 0; L.lds = g.lds;
    p.in = in; p.out = out; p.wpk = wpk; p.bias = bias;
    p.B = B; p.Hin = r.h_in; p.Win = r.w_in;
    p.Hout = deconv ? r.h_in : r.h_out; p.Wout = deconv ? r.w_in : r.w_out;
    p.Cin = r.c1; p.in_ld = in_ld; p.in_coff = in_coff;
    p.Cout = g.gemm_n; p.out_ld = out_ld; p.out_coff = out_coff;
    if (res) { p.res = res; p.res_ld = res_ld; p.res_coff = res_coff; p.has_res = 1; }
    set_tiles(p, g.TH, g.TW);
    p.WN = g.WN;
    p.nt = g.threads;
    p.wreg = g.pk ? 0 : g.wreg;      // the per-tile kernel's flag; conv1_pk's register-resident weights are pk_wstat == 2
    p.pk_lin = run.pk_linear_map;       // A/B aid: the linear pixel -> column-tile map of the persistent 3x3 kernels
    p.act = r.kind == 0; p.out_f32 = out_f32 ? 1 : 0;
    p.deconv_c = deconv ? r.c2 : 0;
    p.swap_rb = swap_rb ? 1 : 0;
    p.nchunks = g.nchunks; p.ntiles_n = g.ntiles_n;
    p.scalar_store = scalar_store(g.gemm_n, out_ld, out_coff);
    p.pw_magic = magic(conv0 ? (unsigned)g.TW : (unsigned)((g.TW - 1) * st + ks));
    p.rw_magic = magic(((unsigned)(2 * g.TW + 1) * 3 + 6) >> 2);      // stem: dwords per u8 patch row
    p.tw_magic = magic((unsigned)g.TW);
    p.wpk_bytes = (unsigned)packed_conv_bytes(r, conv0, g);
    p.alpha = alpha; p.alpha2 = p.alpha0 = 1.f;
    if (!g.pk) return;
    // persistent kernels: workgroups along x walk the tiles; conv1_pk's are runs of TH * 80 pixels of the flattened [B*H*W] index space
    const size_t es = dtype == VTI_F16 ? 2 : 4, npx = (size_t)B * p.Hout * p.Wout;
    const size_t ib = tensor_bytes(g.pk == 2 ? npx : (size_t)B * r.h_in * r.w_in, in_ld, es);
    const size_t ob = tensor_bytes(deconv && g.pk == 2 ? 4 * npx : npx, out_ld, out_f32 ? 4 : es);
    const size_t rb = res && g.pk != 2 ? tensor_bytes(npx, res_ld, es) : 0;
    p.pk = (below_2g(ib) && below_2g(ob) && below_2g(rb) && !(res && g.pk == 2)) ? g.pk : 0;      // else the per-tile kernel
    p.in_bytes = (unsigned)ib; p.out_bytes = (unsigned)ob; p.res_bytes = (unsigned)rb;
    p.pk_depth = g.pk_depth; p.pk_wstat = g.pk_wstat;
    const int gy = g.ntiles_n / (g.WN * g.NREP);
    if (g.pk == 2) {
        p.pk_cps = g.pk_cps;
        set_pk_grid(p, run, (npx + (size_t)g.TH * 80 - 1) / ((size_t)g.TH * 80), g.pk_wgpc, gy);
    } else {
        set_pk_grid(p, run, (size_t)B * p.tiles_y * p.tiles_x, g.pk_wgpc, gy);
        // launches that fill the chip start the upper half of their workgroups late (conv_pk.hip: pk_stagger_wait)
        if ((g.pk == 1 || g.pk == 4) && p.pk_tiles >= std::max(1, 256 * g.pk_wgpc / gy) && p.pk_wgs >= 16) p.pk_stagger = stagger_units(run, dtype);
    }
}

// + its extras: the fused 1x1 (into a buffer or into pred), the Bottleneck's second 3x3 and the C2f's closing 1x1, the folded upsample
static const char* fill_conv(const Plan& P, const Op& op, int B, int swap_rb, const RunOptions& run, const Bindings& b, LaunchRec& L) {
    const ConvRow& r = P.convs[op.conv];
    const ConvCfg& g = op.cfg;
    const int dt = P.desc.dtype;
    conv_record(run, dt, r, g, B, buf_ptr(P, b, op.in.buf), P.bufs[op.in.buf].C, op.in.coff,
                buf_ptr(P, b, op.out.buf), P.bufs[op.out.buf].C, op.out.coff,
                op.has_res ? buf_ptr(P, b, op.res.buf) : nullptr, op.has_res ? P.bufs[op.res.buf].C : 0, op.res.coff,
                (const char*)b.wpk + g.wpk_off, b.bias + g.bias_off, b.alpha[op.conv], op.out_f32, swap_rb, L);
    ConvParams& p = L.conv;
    if (op.pair >= 0) p.alpha2 = b.alpha[op.pair];
    if (op.fused >= 0) {
        fill_stage2(P, b, p, op, g.wpk_off2, g.bias_off2, r);
        if (op.pred_mode) {     // class / coefficient towers write their rows of the anchor-major pred [B, A, no] directly
            const int no = 4 + P.desc.nc + P.desc.nm;
            p.out2 = b.pred + (size_t)op.pred_a0 * no;
            p.out2_ld = no; p.out2_coff = op.pred_cbase; p.out2_f32 = 1; p.out2_bstride = P.num_anchors;
            p.act2 = op.pred_mode == 2 ? 2 : op.pred_mode == 3 ? 3 : 0;
            p.dfl_stride = (float)op.dfl_stride;
            p.scalar_store2 = scalar_store(g.gemm_n2, no, op.pred_cbase);
            p.best = (op.pred_mode == 2 && b.best) ? b.best + (size_t)op.pred_a0 * 2 : nullptr;     // class towers: (max, class) per anchor
        }
    }
    if (op.pair >= 0) {         // fused Bottleneck: second conv's weights; p.out / p.res already are the second conv's views
        p.w2 = (const char*)b.wpk + g.wpk_off2;
        p.bias2 = b.bias + g.bias_off2;
        if (p.pk != 3) return "fused bottleneck needs the persistent kernel (tensor too large?)";
        if (op.tail >= 0) {     // + the C2f's closing 1x1: the patch carries [y0 | y1] (in_coff = y0's offset), y2 is not stored
            const Buf& o2 = P.bufs[op.out2.buf];
            if (dt == VTI_F16) p.in_coff -= r.c1;          // fp16: one 64-byte slot = [y0 | y1]; h2: the patch stays y1, y0 is read directly
            p.alpha0 = b.alpha[op.tail];
            p.w0 = (const char*)b.wpk + g.wpk_off3; p.bias0 = b.bias + g.bias_off3;
            p.out2 = buf_ptr(P, b, op.out2.buf); p.out2_ld = o2.C; p.out2_coff = op.out2.coff; p.Cout2 = P.convs[op.tail].c2;
            const size_t o2b = tensor_bytes((size_t)B * p.Hout * p.Wout, o2.C, P.esize);
            if (!below_2g(o2b)) return "fused bottleneck tail: output tensor too large";
            p.out2_bytes = (unsigned)o2b;
        }
    }
    if (op.up_C > 0) {
        const Buf& ub = P.bufs[op.up_src.buf];
        p.in2 = buf_ptr(P, b, op.up_src.buf); p.in2_ld = ub.C; p.in2_coff = op.up_src.coff; p.up_C = op.up_C;
        p.in2_bytes = (unsigned)tensor_bytes((size_t)B * ub.H * ub.W, ub.C, P.esize);
        if (p.pk != 2) return "folded upsample needs the persistent 1x1 kernel (tensor too large?)";
    }
    return nullptr;
}
static void conv_geometry_of(const Op& op, int i, vti_conv_info* o) {
    if (op.conv == i) return own_geometry(op.cfg, o);
    if (op.fused == i) return stage2_geometry(op, o);
    // inside the first 3x3's kernel (bneck_pk): the C2f's closing 1x1 (tail), or the second 3x3 of the Bottleneck (pair)
    o->tile_h = op.cfg.TH; o->tile_w = op.cfg.TW; o->waves_n = 1; o->nrep = op.tail == i ? 2 : op.cfg.NREP; o->lds_bytes = 0;
    o->fused = 1; o->persistent = 1;
}

// ---- the ops that are no conv ---------------------------------------------------------------------------------------------------------
static void fill_pool(const Plan& P, const Op& op, int B, const Bindings& b, LaunchRec& L) {
    const Buf& ib = P.bufs[op.in.buf];
    L.fn = LAUNCH_POOL;
    PoolParams& p = L.pool;
    p.in = buf_ptr(P, b, op.in.buf); p.out = (void*)p.in;
    p.B = B; p.H = ib.H; p.W = ib.W; p.C = op.in.C; p.ld = ib.C; p.in_coff = op.in.coff; p.out_coff = op.out.coff;
}
static void fill_up2(const Plan& P, const Op& op, int B, const Bindings& b, LaunchRec& L) {
    const Buf& ib = P.bufs[op.in.buf];
    L.fn = LAUNCH_UP2;
    Up2Params& p = L.up2;
    p.in = buf_ptr(P, b, op.in.buf); p.out = buf_ptr(P, b, op.out.buf);
    p.B = B; p.H = ib.H; p.W = ib.W; p.C = op.in.C; p.in_ld = ib.C; p.in_coff = op.in.coff;
    p.out_ld = P.bufs[op.out.buf].C; p.out_coff = op.out.coff;
}
static void fill_decode(const Plan& P, int B, const Bindings& b, LaunchRec& L) {
    L.fn = P.pred_scatter ? LAUNCH_BOX_DECODE : LAUNCH_DECODE;      // pred_scatter: the towers wrote classes and coefficients themselves
    DecodeParams& p = L.dec;
    memset(&p, 0, sizeof p);
    int a0 = 0;
    for (int l = 0; l < 3; ++l) {
        const Level& lv = P.levels[l];
        p.box[l] = (const float*)(b.ws + P.bufs[lv.box_buf].off);
        p.cls[l] = (const float*)(b.ws + P.bufs[lv.cls_buf].off);
        p.mc[l] = (const float*)(b.ws + P.bufs[lv.mc_buf].off);
        p.H[l] = lv.H; p.W[l] = lv.W; p.stride[l] = lv.stride; p.a0[l] = a0;
        a0 += lv.H * lv.W;
    }
    p.B = B; p.A = P.num_anchors; p.nc = P.desc.nc; p.nm = P.desc.nm; p.reg_max = P.desc.reg_max;
    p.pred = b.pred;
}

// ---- one op of the plan -------------------------------------------------------------------------------------------------------------
const char* fill_launch(const Plan& P, const Op& op, int B, int swap_rb, const RunOptions& run, const Bindings& b, LaunchRec& L) {
    L.name = nullptr; L.dtype = P.desc.dtype;
    switch (op.kind) {
    case OP_CONV0:
    case OP_CONV:
        if (op.fused_l1 >= 0) fill_stem_l1(P, op, B, swap_rb, run, b, L);
        else if (op.fold >= 0) fill_fold(P, op, B, run, b, L);
        else return fill_conv(P, op, B, swap_rb, run, b, L);
        break;
    case OP_POOL: fill_pool(P, op, B, b, L); break;
    case OP_UP2: fill_up2(P, op, B, b, L); break;
    case OP_DECODE: fill_decode(P, B, b, L); break;
    case OP_FORK:
    case OP_JOIN: break;       // no launch: the caller's streams
    }
    return nullptr;
}

void conv_geometry(const Plan& P, int i, vti_conv_info* o) {
    for (const Op& op : P.ops) {
        if ((op.kind != OP_CONV && op.kind != OP_CONV0) || (op.conv != i && op.tail != i && op.pair != i && op.fold != i && op.fused_l1 != i && op.fused != i))
            continue;
        if (op.fused_l1 >= 0) stem_l1_geometry(op, i, o);
        else if (op.fold >= 0) fold_geometry(op, i, o);
        else conv_geometry_of(op, i, o);
    }
}

std::string op_label(const Plan& P, const Op& op) {
    if (op.kind != OP_CONV && op.kind != OP_CONV0) return op.kind == OP_POOL ? "sppf_pool" : op.kind == OP_UP2 ? "upsample2x" : "decode";
    auto name = [&](int conv) { return P.convs[conv].name; };
    std::string s = name(op.conv);
    if (op.fused_l1 >= 0) s += " + " + name(op.fused_l1);
    else if (op.fold >= 0) s += " (folded: " + name(op.fold) + ")";
    else if (op.pair >= 0) s += " + " + name(op.pair) + (op.tail >= 0 ? " + " + name(op.tail) : "");
    if (op.fused >= 0) s += " + " + name(op.fused);
    return s;
}

const char* launcher_name(Launcher fn) {
    static const char* const names[] = {"launch_stem_l1", "launch_conv", "launch_convfold", "launch_conv_pk_fold", "launch_sppf_pool",
                                        "launch_upsample2x", "launch_decode", "launch_box_decode"};
    return names[fn];
}

// workgroups of a conv-form launch (the stamp slots of the diagnostic build): the persistent grid or one per tile, times the n-groups
size_t launch_workgroups(const LaunchRec& L) {
    const ConvParams& p = L.conv;
    const size_t tiles = (size_t)p.B * p.tiles_y * p.tiles_x;
    if (L.fn == LAUNCH_STEM_L1) return (size_t)stem_l1_grid(L.dtype, (int)tiles, L.persistent);
    const int NTB = p.WN * L.nrep;
    return (p.pk ? (size_t)p.pk_wgs : tiles) * ((p.ntiles_n + NTB - 1) / NTB);
}

}  // namespace vti
