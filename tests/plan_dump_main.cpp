// Stand-alone program (its own main, linked against libvti.so): prints a canonical text dump of everything the host planner
// decides, so that tests/test_plan_golden.py can compare plans byte for byte with the ones recorded in tests/golden/plan_dumps.json.
// Nothing here touches a GPU.
//
//   plan_dump_main plan  SCALE NC NM H W MAX_BATCH DTYPE [--set MEMBER=VALUE ...]
//       the plan of one vti_desc under the switches of the environment; with --set the environment is not read: the planner gets a
//       default PlanOptions with the named members filled in directly (the planner is a function of its arguments)
//   plan_dump_main cfg   DTYPE B H W C1 C2 K S KIND TH TW WN NREP
//       the ConvCfg vti_debug_conv2d would run one conv with (forced tile / waves / nrep; 0 = free)
//   plan_dump_main twice NAME VALUE_A VALUE_B SCALE NC NM H W MAX_BATCH DTYPE
//       two plans built in ONE process, the environment switch NAME set to VALUE_A and then to VALUE_B ("-" = unset), separated by
//       a line "==== second plan"
//   plan_dump_main runopts
//       the launch path's switches (RunOptions) as parsed from the environment
//   plan_dump_main launches SCALE NC NM H W MAX_BATCH DTYPE B SWAP_RB BEST
//       every launch of one forward of B frames (BEST 1: with the anchor pairs) under the switches of the environment, one line per
//       launch: the op's index, the launcher, its selector arguments, every field of its block (tests/launch_dump.h), the tensors at
//       fake addresses; a refusal's text in place of its line; then what vti_conv_at reports of every conv
//   plan_dump_main cfglaunch DTYPE B H W C1 C2 K S KIND TH TW WN NREP
//       the launch vti_debug_conv2d would issue for that conv (dense tensors, without and with a residual)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../vision-textile-inspection_amd/csrc/vti_internal.h"
#include "launch_dump.h"

using namespace vti;

static void dump_view(const char* tag, const View& v) { printf(" %s=%d:%d+%d", tag, v.buf, v.coff, v.C); }

static void dump_cfg(const ConvCfg& c) {
    printf(" cfg: TH=%d TW=%d WN=%d NREP=%d nchunks=%d ntiles_n=%d gemm_n=%d lds=%zu wpk_off=%zu bias_off=%zu ntiles2=%d gemm_n2=%d "
           "wpk_off2=%zu bias_off2=%zu wpk_off3=%zu bias_off3=%zu pk=%d pk_wgpc=%d pk_depth=%d pk_wstat=%d pk_cps=%d threads=%d wreg=%d\n",
           c.TH, c.TW, c.WN, c.NREP, c.nchunks, c.ntiles_n, c.gemm_n, c.lds, c.wpk_off, c.bias_off, c.ntiles2, c.gemm_n2, c.wpk_off2,
           c.bias_off2, c.wpk_off3, c.bias_off3, c.pk, c.pk_wgpc, c.pk_depth, c.pk_wstat, c.pk_cps, c.threads, c.wreg);
}

static void dump_plan(const Plan& P, const std::string& err) {
    if (!err.empty()) { printf("refused: %s\n", err.c_str()); return; }
    printf("esize=%d proto_buf_c=%d proto_src=%d:%d+%d num_anchors=%d pred_scatter=%d dfl_fused=%d ws_bytes=%zu wpk_bytes=%zu bias_floats=%zu "
           "macs=%lld fused_params=%lld\n", P.esize, P.proto_buf_c, P.proto_src.buf, P.proto_src.coff, P.proto_src.C, P.num_anchors,
           (int)P.pred_scatter, (int)P.dfl_fused, P.ws_bytes, P.wpk_bytes, P.bias_floats, (long long)P.macs, (long long)P.fused_params);
    for (size_t i = 0; i < P.bufs.size(); ++i) {
        const Buf& b = P.bufs[i];
        printf("buf %zu: C=%d H=%d W=%d elem=%d off=%zu bytes=%zu\n", i, b.C, b.H, b.W, b.elem, b.off, b.bytes);
    }
    for (size_t i = 0; i < P.convs.size(); ++i) {
        const ConvRow& r = P.convs[i];
        printf("conv %zu: %s c1=%d c2=%d k=%d s=%d kind=%d in=%dx%d out=%dx%d", i, r.name.c_str(), r.c1, r.c2, r.k, r.s, r.kind, r.h_in,
               r.w_in, r.h_out, r.w_out);
        dump_view("conv_out", P.conv_out[i]);
        printf("\n");
    }
    for (size_t i = 0; i < P.ops.size(); ++i) {
        const Op& o = P.ops[i];
        printf("op %zu: kind=%d conv=%d lane=%d", i, (int)o.kind, o.conv, o.lane);
        dump_view("in", o.in); dump_view("out", o.out); dump_view("res", o.res); dump_view("out2", o.out2); dump_view("up_src", o.up_src);
        printf(" has_res=%d out_f32=%d out2_f32=%d fused=%d tail=%d pair=%d fold=%d fused_l1=%d pred_mode=%d pred_cbase=%d pred_a0=%d "
               "dfl_stride=%d nat2=%d up_C=%d\n", (int)o.has_res, (int)o.out_f32, (int)o.out2_f32, o.fused, o.tail, o.pair, o.fold,
               o.fused_l1, o.pred_mode, o.pred_cbase, o.pred_a0, o.dfl_stride, o.nat2, o.up_C);
        if (o.kind == OP_CONV || o.kind == OP_CONV0) dump_cfg(o.cfg);
    }
    for (size_t i = 0; i < P.levels.size(); ++i) {
        const Level& l = P.levels[i];
        printf("level %zu: C=%d H=%d W=%d stride=%d box_buf=%d cls_buf=%d mc_buf=%d\n", i, l.C, l.H, l.W, l.stride, l.box_buf, l.cls_buf,
               l.mc_buf);
    }
    int launches = 0;
    for (const Op& o : P.ops) launches += (o.kind != OP_FORK && o.kind != OP_JOIN);
    printf("num_launches=%d\n", launches);
}

static vti_desc desc_of(char** a) {
    vti_desc d;
    memset(&d, 0, sizeof d);
    d.scale = a[0][0]; d.nc = atoi(a[1]); d.nm = atoi(a[2]); d.reg_max = 16; d.H = atoi(a[3]); d.W = atoi(a[4]);
    d.max_batch = atoi(a[5]); d.dtype = atoi(a[6]);
    return d;
}

// the row vti_debug_conv2d makes of (.., H, W, C1, C2, K, S, KIND, ..)
static ConvRow debug_row(const int* v) {
    const int H = v[2], W = v[3], k = v[6], s = v[7], kind = v[8];
    ConvRow r;
    r.name = "debug"; r.c1 = v[4]; r.c2 = v[5]; r.k = k; r.s = s; r.kind = kind; r.h_in = H; r.w_in = W;
    if (kind == 2) { r.h_out = 2 * H; r.w_out = 2 * W; }
    else { r.h_out = (H + 2 * (k / 2) - k) / s + 1; r.w_out = (W + 2 * (k / 2) - k) / s + 1; }
    return r;
}

static void dump_record(const LaunchRec& L) {
    switch (L.fn) {
    case LAUNCH_STEM_L1: launch_dump::print_stem_l1(L.dtype, L.conv, L.persistent); break;
    case LAUNCH_CONV: launch_dump::print_conv(L.dtype, L.ks, L.stride, L.nrep, L.mode, L.conv, L.lds); break;
    case LAUNCH_CONVFOLD:
    case LAUNCH_CONV_PK_FOLD: launch_dump::print_fold(launcher_name(L.fn), L.dtype, L.conv, L.lds); break;
    case LAUNCH_POOL: launch_dump::print_pool(L.dtype, L.pool); break;
    case LAUNCH_UP2: launch_dump::print_up2(L.dtype, L.up2); break;
    case LAUNCH_DECODE:
    case LAUNCH_BOX_DECODE: launch_dump::print_decode(launcher_name(L.fn), L.dec); break;
    }
}

// What vti_forward / vti_forward_scored would launch: the loop of forward_impl without its streams.
static void dump_launches(const vti_desc& d, const Options& opt, int B, int swap_rb, bool with_best) {
    Plan P;
    const std::string err = P.build(d, opt.plan);
    if (!err.empty()) { printf("vti_create refused: vti_create: %s\n", err.c_str()); return; }
    std::vector<float> alpha;
    for (size_t i = 0; i < P.convs.size(); ++i) alpha.push_back(launch_dump::fake_alpha((int)i));
    const Bindings bind{launch_dump::fake_ws(), launch_dump::fake_wpk(), launch_dump::fake_bias(), alpha.data(), launch_dump::fake_input(),
                        launch_dump::fake_pred(), launch_dump::fake_proto(), with_best ? launch_dump::fake_best() : nullptr};
    LaunchRec L;
    bool refused = false;
    for (size_t i = 0; i < P.ops.size() && !refused; ++i) {
        const Op& op = P.ops[i];
        if (op.kind == OP_FORK || op.kind == OP_JOIN) continue;
        launch_dump::op_index() = (int)i;
        if (const char* e = fill_launch(P, op, B, swap_rb, opt.run, bind, L)) { launch_dump::print_refusal(VTI_ERR_UNSUPPORTED, e); refused = true; }
        else dump_record(L);
    }
    if (!refused && with_best && !P.pred_scatter)
        launch_dump::print_anchor_best(bind.pred, B, P.num_anchors, P.desc.nc, P.desc.nm, bind.best);
    for (size_t i = 0; i < P.convs.size(); ++i) {
        const ConvRow& r = P.convs[i];
        vti_conv_info o;
        memset(&o, 0, sizeof o);
        snprintf(o.name, sizeof o.name, "%s", r.name.c_str());
        conv_geometry(P, (int)i, &o);
        launch_dump::print_conv_info((int)i, o);
    }
}

static void build_and_dump(const vti_desc& d, const PlanOptions& opt) {
    Plan P;
    const std::string err = P.build(d, opt);
    dump_plan(P, err);
}

// --set MEMBER=VALUE: the members of PlanOptions that tests/test_plan_golden.py fills in directly
static bool set_member(PlanOptions& o, const std::string& kv) {
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) return false;
    const std::string k = kv.substr(0, eq);
    const long long v = atoll(kv.c_str() + eq + 1);
    if (k == "no_pk") o.no_pk = v != 0;
    else if (k == "no_fuse") o.no_fuse = v != 0;
    else if (k == "no_bneck") o.no_bneck = v != 0;
    else if (k == "p3_lanes") o.p3_lanes = v != 0;
    else if (k == "pk1_no_wgpc2") o.pk1_no_wgpc2 = v != 0;
    else if (k == "pk1_all") o.pk1_all = v != 0;
    else if (k == "conv1_wreg") o.conv1_wreg = v != 0;
    else if (k == "fold512") o.fold512 = (int)v;
    else if (k == "pk_fused") o.pk_fused = (int)v;
    else if (k == "pk_depth") o.pk_depth = (int)v;
    else if (k == "pk_limit_bytes") o.pk_limit_bytes = (size_t)v;
    else if (k == "pk1_wstat_bytes") o.pk1_wstat_bytes = (size_t)v;
    else return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc >= 9 && !strcmp(argv[1], "plan")) {
        PlanOptions opt;
        if (argc == 9) opt = options_from_env().plan;
        for (int i = 9; i < argc; i += 2)
            if (i + 1 >= argc || strcmp(argv[i], "--set") || !set_member(opt, argv[i + 1])) { fprintf(stderr, "bad --set\n"); return 2; }
        build_and_dump(desc_of(argv + 2), opt);
        return 0;
    }
    if (argc == 15 && !strcmp(argv[1], "cfg")) {
        int v[13];
        for (int i = 0; i < 13; ++i) v[i] = atoi(argv[2 + i]);
        const int dtype = v[0], B = v[1];
        const ConvRow r = debug_row(v);
        ConvCfg g;
        choose_conv_cfg(options_from_env().plan, dtype, r, r.c1 == 3, B, g, v[9], v[10], v[11], v[12]);
        dump_cfg(g);
        return 0;
    }
    if (argc == 12 && !strcmp(argv[1], "launches")) {
        dump_launches(desc_of(argv + 2), options_from_env(), atoi(argv[9]), atoi(argv[10]), atoi(argv[11]) != 0);
        return 0;
    }
    if (argc == 15 && !strcmp(argv[1], "cfglaunch")) {
        int v[13];
        for (int i = 0; i < 13; ++i) v[i] = atoi(argv[2 + i]);
        const int dtype = v[0], B = v[1];
        const ConvRow r = debug_row(v);
        const Options opt = options_from_env();
        ConvCfg g;
        choose_conv_cfg(opt.plan, dtype, r, r.c1 == 3, B, g, v[9], v[10], v[11], v[12]);
        if (g.TH == 0) { printf("no launch configuration fits\n"); return 0; }
        launch_dump::op_index() = 0;
        for (int res = 0; res < 2; ++res) {      // the tensors dense: ld = channels, offsets 0
            LaunchRec L;
            conv_record(opt.run, dtype, r, g, B, launch_dump::fake_input(), r.c1, 0, launch_dump::fake_pred(), r.c2, 0,
                        res ? launch_dump::fake_proto() : nullptr, res ? r.c2 : 0, 0, launch_dump::fake_wpk(), launch_dump::fake_bias(),
                        launch_dump::fake_alpha(0), false, 0, L);
            dump_record(L);
        }
        return 0;
    }
    if (argc == 12 && !strcmp(argv[1], "twice")) {
        for (int round = 0; round < 2; ++round) {
            const char* val = argv[3 + round];
            if (!strcmp(val, "-")) unsetenv(argv[2]); else setenv(argv[2], val, 1);
            if (round) printf("==== second plan\n");
            build_and_dump(desc_of(argv + 5), options_from_env().plan);
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "runopts")) {
        const RunOptions r = options_from_env().run;
        printf("pk_max_wgs=%d pk_stagger=%d pk_linear_map=%d single_stream=%d list_ops=%d stem_not_persistent=%d mask_wgs_per_cu=%d stamp_op=%s\n",
               r.pk_max_wgs, r.pk_stagger, (int)r.pk_linear_map, (int)r.single_stream, (int)r.list_ops, (int)r.stem_not_persistent,
               r.mask_wgs_per_cu, r.stamp_op.c_str());
        return 0;
    }
    fprintf(stderr, "usage: plan_dump_main plan|cfg|twice|runopts|launches|cfglaunch ... (see the head of tests/plan_dump_main.cpp)\n");
    return 2;
}
