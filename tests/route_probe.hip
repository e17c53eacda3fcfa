// Host program behind tests/test_routes.py: asks the library's own route functions (chirpgp_amd/csrc/cgp_route.hpp) which kernel each
// launch of tests/route_cases.py would take.  Built with `hipcc --cuda-host-only`; opens no device and launches nothing.
// stdin: one case a line (route_cases.probe_line); stdout a line: "refused: <the library's message>", for a filter "<route> wave=<0|1>
// segs=<n>", for a smoother the whole plan -- "<route> wave=<0|1> segs=<n> tiles=<per segment> bsegs=<n> chunks=<per segment>
// burn=<chunks> sel=<none|kernel|gather>": the exact split of the walks, the split with burn-in, how selected outputs get written.
#include <cstdio>
#include <cstring>
#include "../chirpgp_amd/csrc/cgp_kernels.hpp"

using namespace cgp;

static const char* name(FilterRoute r) {
    switch (r) {
    case FilterRoute::kGenericWave: return "generic_wave";
    case FilterRoute::kGenericLane: return "generic_lane";
    case FilterRoute::kKf4Mfma: return "kf4_mfma";
    case FilterRoute::kEkf4Mfma: return "ekf4_mfma";
    case FilterRoute::kEkf4MfmaSeg: return "ekf4_mfma_seg";
    case FilterRoute::kEkf4MfmaX4: return "ekf4_mfma_x4";
    case FilterRoute::kEkf4Coop: return "ekf4_coop";
    case FilterRoute::kSgp4Mfma: return "sgp4_mfma";
    case FilterRoute::kSgp4Coop: return "sgp4_coop";
    case FilterRoute::kLane4Ekf: return "lane4_ekf";
    case FilterRoute::kLane4Sgp: return "lane4_sgp";
    case FilterRoute::kEkf8Coop: return "ekf8_coop";
    case FilterRoute::kSgp8Coop: return "sgp8_coop";
    case FilterRoute::kCdEkf4Mfma: return "cdekf4_mfma";
    case FilterRoute::kCdEkf4Coop: return "cdekf4_coop";
    case FilterRoute::kCdSgp4Mfma: return "cdsgp4_mfma";
    case FilterRoute::kCdSgp4Coop: return "cdsgp4_coop";
    case FilterRoute::kKpt8Coop: return "kpt8_coop";
    case FilterRoute::kGenericKpt: return "generic_kpt";
    }
    return "?";
}
static const char* name(SmootherRoute r) {
    switch (r) {
    case SmootherRoute::kCoop8Linear: return "coop8_linear";
    case SmootherRoute::kWalk4Linear: return "walk4_linear";
    case SmootherRoute::kDiscLinear: return "disc_linear";
    case SmootherRoute::kCoop8Harm: return "coop8_harm";
    case SmootherRoute::kWalk4Harm: return "walk4_harm";
    case SmootherRoute::kLane4: return "lane4";
    case SmootherRoute::kDiscHarm: return "disc_harm";
    case SmootherRoute::kSdeLinear: return "sde_linear";
    case SmootherRoute::kCdSgp4Mfma: return "cdsgps4_mfma";
    case SmootherRoute::kCdSgp4Coop: return "cdsgps4_coop";
    case SmootherRoute::kCdEks4Mfma: return "cdeks4_mfma";
    case SmootherRoute::kCdEks4Coop: return "cdeks4_coop";
    case SmootherRoute::kSdeHarm: return "sde_harm";
    case SmootherRoute::kNone: return "none";
    }
    return "?";
}

static const char* name(SmootherSelect s) {
    switch (s) {
    case SmootherSelect::kNone: return "none";
    case SmootherSelect::kKernel: return "kernel";
    case SmootherSelect::kGather: return "gather";
    }
    return "?";
}

int main() {
    alignas(16) static double memory[64];      // what the pointers of a case point at: never read, only their alignment counts
    char entry[32];
    int method, model_id, d, n_harm, s, n_groups, grouped, align, num_cus, null_rows, blocks_per_cu, walk_cap;
    unsigned sflags, flags;
    long long B, T, segments, burn_in;
    while (scanf("%31s %d %d %d %d %d %d %d %u %lld %lld %u %lld %d %d %d %d %d %lld", entry, &method, &model_id, &d, &n_harm, &s, &n_groups, &grouped, &sflags,
                 &B, &T, &flags, &segments, &align, &num_cus, &null_rows, &blocks_per_cu, &walk_cap, &burn_in) == 19) {
        const double* rows = (const double*)((const char*)memory + align);
        static const int group_start[1] = {0};
        cgp_model model;
        memset(&model, 0, sizeof(model));
        model.model_id = model_id; model.d = d; model.n_harm = n_harm; model.params = memory; model.gamma = memory;
        cgp_sigma sigma;
        memset(&sigma, 0, sizeof(sigma));
        sigma.s = s; sigma.d = d; sigma.xi = memory; sigma.w = memory; sigma.group_start = grouped ? group_start : nullptr;
        sigma.n_groups = n_groups; sigma.flags = sflags;
        const cgp_sigma* sg = s > 0 ? &sigma : nullptr;
        const ModelArgs ma = model_args(&model, sg, 1e-3, flags);
        if (!strncmp(entry, "filter", 6)) {
            FilterIO io{};
            io.ys = rows; io.ys_stride = T; io.ys_repeat = 1; io.B = B; io.T = T; io.flags = flags;
            const FilterDecision r = route_filter({method, &model, sg, &io, &ma, flags, segments, num_cus});
            if (r.rc != CGP_OK) printf("refused: %s\n", r.message);
            else printf("%s wave=%d segs=%d\n", name(r.route), (int)r.wave, r.segs);
        } else {
            SmootherIO io{};
            io.mfs = rows; io.Pfs = rows; io.B = B; io.T = T; io.flags = flags;
            SmootherQuery q{method, &model, sg, &io, &ma, flags, num_cus};
            q.walk_cap = walk_cap;
            q.segments = segments; q.burn_in = burn_in;
            q.want_sel = !strcmp(entry, "select"); q.null_rows = null_rows != 0;
            const SmootherDecision r = route_smoother(q);
            if (r.rc != CGP_OK) { printf("refused: %s\n", r.message); continue; }
            // the exact split as the walks' launcher works it out, with the case's answer in place of the occupancy query
            const WalkSegments w = walk_segments(r.split, B, T, num_cus, blocks_per_cu);
            printf("%s wave=%d segs=%d tiles=%d bsegs=%d chunks=%d burn=%d sel=%s\n", name(r.route), (int)r.wave, w.segs, w.tiles_per_seg,
                   r.bsegs, r.chunks_per_bseg, r.burn_chunks, name(r.select));
        }
    }
    return 0;
}
