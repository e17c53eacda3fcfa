// Host program behind tests/test_abi_refusals.py: asks the pure half of every C-ABI entry point (chirpgp_amd/csrc/cgp_args.hpp: the
// prepare_ functions) what it makes of each call of tests/abi_cases.py.  Built with `hipcc --cuda-host-only`; opens no device, links no
// library and launches nothing: every pointer of a case is a non-null fake that nobody reads (comps, the one host array, is real).
// stdin: one call a line (abi_cases.probe_line: "<entry> key=value ..."); stdout a line: "refused <rc>: <message>", "empty" or "ok".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../chirpgp_amd/csrc/cgp_kernels.hpp"

using namespace cgp;

alignas(16) static double memory[64];                // what the pointers of a case point at: never read, only their alignment counts

struct Case {
    std::map<std::string, long long> kv;
    long long operator()(const std::string& key) const {
        const auto it = kv.find(key);
        return it == kv.end() ? 0 : it->second;
    }
    template <class P = double> P* ptr(const std::string& key) const { return (*this)(key) ? (P*)memory : nullptr; }
    const cgp_model* model(cgp_model& m) const {
        const Case& c = *this;
        memset(&m, 0, sizeof m);
        m.model_id = (int)c("model.model_id"); m.d = (int)c("model.d"); m.n_harm = (int)c("model.n_harm"); m.n_params = (int)c("model.n_params");
        m.params = ptr("model.params"); m.param_stride = c("model.param_stride"); m.gamma = ptr("model.gamma"); m.gamma_stride = c("model.gamma_stride");
        return c("model") ? &m : nullptr;
    }
    const cgp_sigma* sigma(cgp_sigma& s) const {
        const Case& c = *this;
        memset(&s, 0, sizeof s);
        s.s = (int)c("sigma.s"); s.d = (int)c("sigma.d"); s.xi = ptr("sigma.xi"); s.w = ptr("sigma.w"); s.group_start = ptr<int>("sigma.group_start");
        s.n_groups = (int)c("sigma.n_groups"); s.flags = (uint32_t)c("sigma.flags");
        return c("sigma") ? &s : nullptr;
    }
    const cgp_init* init(cgp_init& i) const {
        const Case& c = *this;
        memset(&i, 0, sizeof i);
        i.H = ptr("init.H"); i.H_stride = c("init.H_stride"); i.Xi = ptr("init.Xi"); i.Xi_stride = c("init.Xi_stride");
        i.m0 = ptr("init.m0"); i.m0_stride = c("init.m0_stride"); i.P0 = ptr("init.P0"); i.P0_stride = c("init.P0_stride");
        return c("init") ? &i : nullptr;
    }
    CustomModel custom() const {
        const Case& c = *this;
        if (!c("m")) return {};
        return {true, (int)c("m.kind"), (int)c("m.d"), (int)c("m.device"), c("m.ekf") != 0, c("m.sgp") != 0};
    }
};

static Verdict prepare(const std::string& entry, const Case& c) {
    const HostCtx host;                              // device 0 of a 256-CU GPU, nothing set by cgp_debug_set
    cgp_model model_s; cgp_sigma sigma_s; cgp_init init_s;
    const cgp_model* model = c.model(model_s);
    const cgp_sigma* sigma = c.sigma(sigma_s);
    const cgp_init* init = c.init(init_s);
    ModelArgs ma;
    const double dt = 1e-3;
    const int64_t B = c("B"), T = c("T");
    const uint32_t flags = (uint32_t)c("flags");
    if (entry == "cgp_filter" || entry == "cgp_filter_time_split") {
        FilterCall call{(int)c("method"), model, sigma, init, dt, c.ptr("ys"), c("ys_stride"), c("ys_repeat"), c.ptr<int32_t>("ys_index"), B, T,
                        c.ptr("mfs"), c.ptr("Pfs"), c.ptr("nll"), flags};
        if (entry == "cgp_filter_time_split") { call.time_split = true; call.segments = c("segments"); call.burn_in = c("burn_in"); call.junction_err = c.ptr("junction_err"); }
        FilterPlan plan;
        return prepare_filter(call, host, plan);
    }
    if (entry == "cgp_smoother" || entry == "cgp_smoother_time_split" || entry == "cgp_smoother_select") {
        cgp_smooth_out out;
        memset(&out, 0, sizeof out);
        const bool select = entry == "cgp_smoother_select";
        if (select) {
            out.mss = c.ptr("out.mss"); out.Pss = c.ptr("out.Pss"); out.comp = (int)c("out.comp"); out.func = (int)c("out.func");
            out.comp_mean = c.ptr("out.comp_mean"); out.comp_var = c.ptr("out.comp_var"); out.expect = c.ptr("out.expect");
            out.xi = c.ptr("out.xi"); out.w = c.ptr("out.w"); out.order = (int)c("out.order");
        } else { out.mss = c.ptr("mss"); out.Pss = c.ptr("Pss"); out.comp = -1; }
        SmootherCall call{(int)c("method"), model, sigma, dt, c.ptr("mfs"), c.ptr("Pfs"), B, T, (!select || c("out")) ? &out : nullptr, flags};
        if (entry == "cgp_smoother_time_split") { call.time_split = true; call.segments = c("segments"); call.burn_in = c("burn_in"); call.junction_err = c.ptr("junction_err"); }
        SmootherPlan plan;
        return prepare_smoother(call, host, plan);
    }
    if (entry == "cgp_smoother_sample") {
        cgp_sample_out out;
        memset(&out, 0, sizeof out);
        out.paths = c.ptr("out.paths"); out.comp_paths = c.ptr("out.comp_paths"); out.comp = (int)c("out.comp"); out.func = (int)c("out.func");
        SampleIO io{};
        return prepare_smoother_sample((int)c("method"), model, sigma, dt, c.ptr("mfs"), c.ptr("Pfs"), B, T, c("S"), (uint64_t)c("seed"), c("trial0"), c("sample0"),
                                       c.ptr("normals"), c("out") ? &out : nullptr, flags, io, ma);
    }
    if (entry.size() > 9 && (entry.find("_nll_grad") != std::string::npos || entry.find("_nll_fisher") != std::string::npos)) {
        static const std::string names[] = {"cgp_ekf_nll_grad", "cgp_ekf_nll_fisher", "cgp_sgp_nll_grad", "cgp_sgp_nll_fisher", "cgp_cd_ekf_nll_grad"};
        const char* name = nullptr;
        for (const std::string& n : names) if (n == entry) name = n.c_str();
        if (!name) return {1, "no such entry point"};
        const TangentCall call{name, entry.find("_sgp_") != std::string::npos, entry.find("_fisher") != std::string::npos, entry.find("_cd_") != std::string::npos};
        TangentIO io{};
        return prepare_tangent(call, model, call.sgp ? sigma : nullptr, init, dt, c.ptr("ys"), c("ys_stride"), c("ys_repeat"), c.ptr<int32_t>("ys_index"), B, T,
                               c.ptr("dirs"), (int32_t)c("n_dir"), c.ptr("nll"), c.ptr("grad"), c.ptr("fisher"), flags, io, ma);
    }
    if (entry == "cgp_filter_custom") {
        FilterIO io{};
        return prepare_filter_custom(c.custom(), sigma, c.ptr("params"), c("param_stride"), c.ptr("gamma"), c("gamma_stride"), init, dt, c.ptr("ys"), c("ys_stride"),
                                     c("ys_repeat"), c.ptr<int32_t>("ys_index"), B, T, c.ptr("mfs"), c.ptr("Pfs"), c.ptr("nll"), flags, host, io, ma);
    }
    if (entry == "cgp_smoother_custom") {
        SmootherIO io{};
        return prepare_smoother_custom(c.custom(), sigma, c.ptr("params"), c("param_stride"), c.ptr("gamma"), c("gamma_stride"), dt, c.ptr("mfs"), c.ptr("Pfs"), B, T,
                                       c.ptr("mss"), c.ptr("Pss"), flags, host, io, ma);
    }
    if (entry == "cgp_simulate") {
        SimIO io{};
        SimShape shape;
        return prepare_simulate(model, init, dt, (uint64_t)c("seed"), c("trial0"), B, T, c.ptr("xs"), c.ptr("ys"), flags, host, io, ma, shape);
    }
    if (entry == "cgp_simulate_x0") return prepare_simulate_x0(model, init, c("trial0"), B, c.ptr("x0"));
    if (entry == "cgp_add_noise") return prepare_add_noise(c.ptr("clean"), c("clean_stride"), c.ptr("Xi"), c("trial0"), B, T, c.ptr("ys"));
    if (entry == "cgp_gaussian_expectation" || entry == "cgp_gaussian_expectation_fn")
        return prepare_gaussian_expectation(entry == "cgp_gaussian_expectation" ? CGP_FN_SOFTPLUS : (int)c("func"), c.ptr("ms"), c.ptr("sd"), c("n"), c.ptr("xi"),
                                            c.ptr("w"), (int32_t)c("order"), c.ptr("out"));
    if (entry == "cgp_squared_error_sums") {
        int32_t comps[16] = {0};
        for (int i = 0; i < 16 && i < c("comps.n"); i++) comps[i] = (int32_t)c("comps." + std::to_string(i));
        ErrComps ec{};
        return prepare_squared_error_sums(c.ptr("a"), c.ptr("r"), B, T, (int32_t)c("d"), c("comps") ? comps : nullptr, (int32_t)c("n"), c.ptr("sums"), ec);
    }
    if (entry == "cgp_pcrlb_sums") {
        PcrlbIO io{};
        int key = 0;
        return prepare_pcrlb_sums(model, dt, c.ptr("x0"), c.ptr("xs"), B, T, c.ptr("sums"), flags, io, ma, key);
    }
    if (entry == "cgp_debug_math") return prepare_debug_math((int)c("op"), c.ptr("x"), c("n"), c.ptr("out0"));
    if (entry == "cgp_debug_philox") return prepare_debug_philox(c.ptr<uint32_t>("ctr"), c.ptr<uint32_t>("key"), c("n"), c.ptr<uint32_t>("out"));
    return {1, "no such entry point"};
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream words(line);
        std::string entry, word;
        words >> entry;
        Case c;
        while (words >> word) {
            const size_t eq = word.find('=');
            c.kv[word.substr(0, eq)] = std::stoll(word.substr(eq + 1));
        }
        const Verdict v = prepare(entry, c);
        if (v.rc != CGP_OK) printf("refused %d: %s\n", v.rc, v.message ? v.message : "");
        else puts(v.empty ? "empty" : "ok");
    }
    return 0;
}
