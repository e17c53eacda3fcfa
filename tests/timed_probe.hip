// Host program behind tests/test_times_host.py: asks the pure half of the two timed entry points (include/chirpgp_hip_timed.h;
// chirpgp_amd/csrc/cgp_args.hpp: prepare_filter / prepare_smoother with FilterCall::timed / SmootherCall::timed) what it makes of a call,
// and which kernel the call would run (cgp_route.hpp).  Built with `hipcc --cuda-host-only`; opens no device, links no library and launches
// nothing: every pointer of a case is a non-null fake that nobody reads.
// stdin: one call a line --
//   <filter|smoother|select> method model_id d n_harm n_params sigma_s n_groups grouped sigma_flags B T flags dts dts_stride dts_repeat null_rows num_cus
// (dts: 0 = NULL); stdout a line: "refused <rc>: <message>", "empty", or the plan -- for a filter "<route> wave=<0|1> timed=<0|1> sub=<0|1>
// gaps=<0|1> stride=<dts_stride>", for a smoother "<route> wave=<0|1> timed=<0|1> sub=<0|1> sel=<none|kernel|gather> stride=<> repeat=<>".
#include <cstdio>
#include <cstring>
#include "../chirpgp_amd/csrc/cgp_kernels.hpp"
#include "../include/chirpgp_hip_timed.h"

using namespace cgp;

static const char* name(FilterRoute r) {
    switch (r) {
    case FilterRoute::kGenericWave: return "generic_wave";
    case FilterRoute::kGenericLane: return "generic_lane";
    case FilterRoute::kCdEkf4Mfma: return "cdekf4_mfma";
    case FilterRoute::kCdSgp4Mfma: return "cdsgp4_mfma";
    case FilterRoute::kCdEkf4Coop: return "cdekf4_coop";
    case FilterRoute::kCdSgp4Coop: return "cdsgp4_coop";
    default: return "untimed";                       // a kernel that knows no intervals: a timed call must never end here
    }
}
static const char* name(SmootherRoute r) {
    switch (r) {
    case SmootherRoute::kSdeLinear: return "sde_linear";
    case SmootherRoute::kSdeHarm: return "sde_harm";
    case SmootherRoute::kCdSgp4Mfma: return "cdsgps4_mfma";
    case SmootherRoute::kCdEks4Mfma: return "cdeks4_mfma";
    case SmootherRoute::kCdSgp4Coop: return "cdsgps4_coop";
    case SmootherRoute::kCdEks4Coop: return "cdeks4_coop";
    case SmootherRoute::kLane4: return "lane4";
    default: return "untimed";
    }
}
static const char* name(SmootherSelect s) { return s == SmootherSelect::kKernel ? "kernel" : s == SmootherSelect::kGather ? "gather" : "none"; }

int main() {
    static_assert(CGP_TIMED_VERSION == 1, "include/chirpgp_hip_timed.h");
    alignas(16) static double memory[64];
    static const int group_start[1] = {0};
    char entry[32];
    int method, model_id, d, n_harm, n_params, s, n_groups, grouped, has_dts, null_rows, num_cus;
    unsigned sflags, flags;
    long long B, T, dts_stride, dts_repeat;
    while (scanf("%31s %d %d %d %d %d %d %d %d %u %lld %lld %u %d %lld %lld %d %d", entry, &method, &model_id, &d, &n_harm, &n_params, &s, &n_groups,
                 &grouped, &sflags, &B, &T, &flags, &has_dts, &dts_stride, &dts_repeat, &null_rows, &num_cus) == 18) {
        cgp_model model;
        memset(&model, 0, sizeof(model));
        model.model_id = model_id; model.d = d; model.n_harm = n_harm; model.n_params = n_params; model.params = memory; model.gamma = memory;
        cgp_sigma sigma;
        memset(&sigma, 0, sizeof(sigma));
        sigma.s = s; sigma.d = d; sigma.xi = memory; sigma.w = memory; sigma.group_start = grouped ? group_start : nullptr;
        sigma.n_groups = n_groups; sigma.flags = sflags;
        const cgp_sigma* sg = s > 0 ? &sigma : nullptr;
        cgp_init init;
        memset(&init, 0, sizeof(init));
        init.H = memory; init.Xi = memory; init.m0 = memory; init.P0 = memory;
        HostCtx host;
        host.num_cus = num_cus;
        const double* dts = has_dts ? memory : nullptr;
        Verdict v;
        if (!strcmp(entry, "filter")) {
            FilterCall call{method, &model, sg, &init, 0.0, memory, T, 1, nullptr, B, T, memory, memory, memory, flags};
            call.dts = dts; call.dts_stride = dts_stride; call.timed = true;
            FilterPlan plan;
            v = prepare_filter(call, host, plan);
            if (v.rc == CGP_OK && !v.empty)
                printf("%s wave=%d timed=%d sub=%d gaps=%d stride=%lld\n", name(plan.route.route), (int)plan.route.wave, (int)plan.route.timed,
                       (int)plan.route.substeps, (int)plan.route.gaps, (long long)plan.io.dts_stride);
        } else {
            cgp_smooth_out out;
            memset(&out, 0, sizeof(out));
            out.comp = -1;
            if (!null_rows) { out.mss = memory; out.Pss = memory; }
            if (!strcmp(entry, "select")) { out.comp = 2; out.comp_mean = memory; }
            SmootherCall call{method, &model, sg, 0.0, memory, memory, B, T, &out, flags};
            call.dts = dts; call.dts_stride = dts_stride; call.dts_repeat = dts_repeat; call.timed = true;
            SmootherPlan plan;
            v = prepare_smoother(call, host, plan);
            if (v.rc == CGP_OK && !v.empty)
                printf("%s wave=%d timed=%d sub=%d sel=%s stride=%lld repeat=%lld\n", name(plan.route.route), (int)plan.route.wave, (int)plan.route.timed,
                       (int)plan.route.substeps, name(plan.route.select), (long long)plan.io.dts_stride, (long long)plan.io.dts_repeat);
        }
        if (v.rc != CGP_OK) printf("refused %d: %s\n", v.rc, v.message ? v.message : "");
        else if (v.empty) printf("empty\n");
    }
    return 0;
}
