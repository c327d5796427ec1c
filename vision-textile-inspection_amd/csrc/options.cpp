// The VTI_* environment switches: the one table that names them and the only code under csrc/ that reads the environment.
// They are developer aids (A/B arms, sweeps, tests of a fall-back); the defaults are the product.  Every switch is read when a
// context is created (vti_create) -- per call for vti_debug_conv2d, which has no context -- and never on the forward path.
// DESIGN.md ("Environment switches") carries the same table for readers.
#include <algorithm>
#include <cstdlib>

#include "vti_internal.h"

namespace vti {

namespace {

// the parse rules (v: the switch's text, nullptr when unset)
bool on1(const char* v) { return v && v[0] == '1'; }                   // on iff the first character is '1' ("10" is on, "true" is off)
int clamped(const char* v, int lo, int hi, int unset) { return v ? std::max(lo, std::min(hi, atoi(v))) : unset; }
int floor1(const char* v) { return v ? std::max(1, atoi(v)) : 0; }     // atoi, at least 1; 0: unset

struct Switch {
    const char* name;
    const char* values;      // what it accepts
    const char* dflt;        // what holds when it is unset
    const char* when;        // "plan": read by the planner; "launch": by the launch path
    const char* meaning;
    void (*parse)(const char* v, Options& o);
};
#define PLAN_FLAG(member) [](const char* v, Options& o) { o.plan.member = on1(v); }
#define RUN_FLAG(member) [](const char* v, Options& o) { o.run.member = on1(v); }

const Switch kSwitches[] = {
    // which kernel a conv gets
    {"VTI_NO_PK", "1", "off", "plan", "3x3 stride-1 convs stay off the persistent kernel (conv3_pk)", PLAN_FLAG(no_pk)},
    {"VTI_NO_PK1", "1", "off", "plan", "1x1 convs stay off the persistent kernel (conv1_pk)", PLAN_FLAG(no_pk1)},
    {"VTI_NO_PK2", "1", "off", "plan", "3x3 stride-2 convs stay off the persistent kernel", PLAN_FLAG(no_pk2)},
    {"VTI_PK1_ALL", "1", "off", "plan", "conv1_pk also on maps below 1600 px and on the ConvTranspose", PLAN_FLAG(pk1_all)},
    {"VTI_PK_FUSED", "1 / 2 / other", "h2: the 64-channel box towers", "plan",
     "fused 3x3 + 1x1 ops on the persistent schedule: 1 all, 2 those with NREP <= 4, anything else none",
     [](const char* v, Options& o) { o.plan.pk_fused = !v ? -1 : v[0] == '1' ? 1 : v[0] == '2' ? 2 : 0; }},
    {"VTI_PK_LIMIT_BYTES", "bytes (atoll)", "2147483648", "plan", "tensors from this size on keep their convs on the per-tile kernels",
     [](const char* v, Options& o) { if (v) o.plan.pk_limit_bytes = (size_t)atoll(v); }},
    {"VTI_CONV1_WREG", "0", "on", "plan", "0: the 1x1 kernels stage their weights through LDS instead of registers",
     [](const char* v, Options& o) { o.plan.conv1_wreg = !(v && v[0] == '0'); }},
    // the cost searches of the persistent kernels
    {"VTI_PK_WIDE16", "1", "off", "plan", "fp16 uses the ingest-priced 3x3 search of the 4-byte types", PLAN_FLAG(pk_wide16)},
    {"VTI_NO_PK_WSTAT", "1", "off", "plan", "the 3x3 search does not try resident weights", PLAN_FLAG(no_pk_wstat)},
    {"VTI_H2_NO_N5", "1", "off", "plan", "h2: the 3x3 search skips NREP = 5", PLAN_FLAG(h2_no_n5)},
    {"VTI_PK_DEPTH", "integer, clamped to 2..4", "2", "plan", "deepest patch ring of conv3_pk (both strides) and bneck_pk",
     [](const char* v, Options& o) { o.plan.pk_depth = clamped(v, 2, 4, 2); }},
    {"VTI_PK_FOLD_DEPTH", "integer, clamped to 2..4", "3", "plan", "deepest patch ring of the persistent fold kernel",
     [](const char* v, Options& o) { o.plan.pk_fold_depth = clamped(v, 2, 4, 3); }},
    {"VTI_PK1_WSTAT_KB", "KiB (atoi)", "96", "plan", "conv1_pk keeps an n-group's weights stationary in LDS up to this size",
     [](const char* v, Options& o) { if (v) o.plan.pk1_wstat_bytes = (size_t)atoi(v) * 1024; }},
    {"VTI_PK1_INFLIGHT_KB", "kB (atof)", "50", "plan", "conv1_pk cost model: bytes in flight per CU that saturate the ingest",
     [](const char* v, Options& o) { if (v) o.plan.pk1_inflight_bytes = atof(v) * 1e3; }},
    {"VTI_PK1_NO_WGPC2", "1", "off", "plan", "conv1_pk (4-byte types): never two workgroups per CU", PLAN_FLAG(pk1_no_wgpc2)},
    {"VTI_PK1_FORCE_WGPC2", "1", "off", "plan", "conv1_pk (4-byte types): always two workgroups per CU", PLAN_FLAG(pk1_force_wgpc2)},
    // the fusion passes, in the planner's order
    {"VTI_P3_LANES", "1", "off", "plan", "the three P3 head towers on three streams instead of one", PLAN_FLAG(p3_lanes)},
    {"VTI_NO_FUSE", "1", "off", "plan", "no 3x3 -> 1x1 fusion (head towers, proto)", PLAN_FLAG(no_fuse)},
    {"VTI_NO_FOLD", "1", "off", "plan", "the proto ConvTranspose is not folded into the following 3x3", PLAN_FLAG(no_fold)},
    {"VTI_NO_BNECK", "1", "off", "plan", "no fused C2f bottleneck pairs (bneck_pk)", PLAN_FLAG(no_bneck)},
    {"VTI_NO_BNECK_TAIL", "1", "off", "plan", "bneck_pk without the C2f's closing 1x1", PLAN_FLAG(no_bneck_tail)},
    {"VTI_NO_STEM_FUSE", "1", "off", "plan", "stem and layer 1 as two kernels", PLAN_FLAG(no_stem_fuse)},
    {"VTI_NO_STEM_FUSE3", "1", "off", "plan", "the stem kernel without model.2.cv1 as its third stage", PLAN_FLAG(no_stem_fuse3)},
    {"VTI_NO_PRED_SCATTER", "1", "off", "plan", "class / coefficient towers write head buffers, the decode kernel gathers them",
     PLAN_FLAG(no_pred_scatter)},
    {"VTI_NO_DFL_FUSE", "1", "off", "plan", "box towers write logits, a decode kernel does DFL + dist2bbox", PLAN_FLAG(no_dfl_fuse)},
    {"VTI_FOLD512", "1 / other", "on for h2", "plan", "the fold kernel's 8-wave form (8 x 20 tiles): 1 also for fp32, anything else off",
     [](const char* v, Options& o) { o.plan.fold512 = v ? v[0] == '1' : -1; }},
    {"VTI_NO_FOLD512", "1", "off", "plan", "h2: the fold kernel's 4-wave form (ignored when VTI_FOLD512 is set)", PLAN_FLAG(no_fold512)},
    {"VTI_NO_PK_FOLD", "1", "off", "plan", "the fold kernel stays off the persistent schedule", PLAN_FLAG(no_pk_fold)},
    {"VTI_NO_T512", "1", "off", "plan", "fused towers never use 8-wave workgroups on 16 x 40 tiles", PLAN_FLAG(no_t512)},
    {"VTI_NO_UPFUSE", "1", "off", "plan", "the neck's Upsample + Concat stay their own op", PLAN_FLAG(no_upfuse)},
    // the launch path
    {"VTI_PK_MAX_WGS", "integer (atoi), at least 1", "none", "launch", "cap of a persistent launch's workgroups (tests: many tiles each)",
     [](const char* v, Options& o) { o.run.pk_max_wgs = floor1(v); }},
    {"VTI_PK_STAGGER", "integer, clamped to 0..255", "h2: 10, else 0", "launch", "delay units (x 1024 cycles) of the staggered 3x3 launches",
     [](const char* v, Options& o) { o.run.pk_stagger = clamped(v, 0, 255, -1); }},
    {"VTI_PK_LINEAR_MAP", "1", "off", "launch", "the persistent 3x3 kernels' linear pixel -> column-tile map", RUN_FLAG(pk_linear_map)},
    {"VTI_SINGLE_STREAM", "1", "off", "launch", "every op on the caller's stream: no side streams are created", RUN_FLAG(single_stream)},
    {"VTI_STEM_NOT_PERSISTENT", "1", "off", "launch", "the stem kernel with one workgroup per tile", RUN_FLAG(stem_not_persistent)},
    {"VTI_MASK_WGS_PER_CU", "integer (atoi), at least 1", "none", "launch", "cap of the mask kernels' resident workgroups per CU",
     [](const char* v, Options& o) { o.run.mask_wgs_per_cu = floor1(v); }},
    {"VTI_LIST_OPS", "set at all", "off", "launch", "every forward lists its launches on stderr",
     [](const char* v, Options& o) { o.run.list_ops = v != nullptr; }},
    {"VTI_STAMP_OP", "a conv's name", "none", "launch", "diagnostic build only: the op whose launch is stamped",
     [](const char* v, Options& o) { o.run.stamp_op = v ? v : ""; }},
};

}  // namespace

Options parse_options(const char* (*get)(const char* name, void* user), void* user) {
    Options o;
    for (const Switch& s : kSwitches) s.parse(get(s.name, user), o);
    return o;
}

Options options_from_env() {
    return parse_options([](const char* name, void*) { return (const char*)getenv(name); }, nullptr);
}

}  // namespace vti
