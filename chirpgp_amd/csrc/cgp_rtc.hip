// cgp_rtc.hip -- models compiled at run time (hiprtc) into the generic lane-per-trial kernels (and, for an SDE model's smoothers with
// CGP_RK4_SUBSTEPS, the one-wavefront-per-trial ones): cgp_model_from_source, cgp_filter_custom, cgp_smoother_custom.  See cgp_custom.hpp for the model interface.  libhiprtc is opened on first use (dlopen), so a process that never
// builds a custom model never loads it.
#include <dlfcn.h>
#include <cstring>
#include <string>
#include <vector>
#include "cgp_kernels.hpp"
#include "cgp_ctx.hpp"

struct cgp_custom_model {
    int kind = 0, d = 0;
    int device = 0;
    hipModule_t module = nullptr;
    hipFunction_t filter = nullptr, smoother = nullptr, sgp_filter = nullptr, sgp_smoother = nullptr;
    // CGP_RK4_SUBSTEPS (CGP_CUSTOM_SDE only): SubstepPredict in the filters' one-lane-per-trial shape, SubstepSmooth with one wavefront per trial
    hipFunction_t filter_sub = nullptr, smoother_sub = nullptr, sgp_filter_sub = nullptr, sgp_smoother_sub = nullptr;
};

namespace {
using namespace cgp;

struct Rtc {
    void* lib = nullptr;
    int (*CreateProgram)(void**, const char*, const char*, int, const char**, const char**) = nullptr;
    int (*AddNameExpression)(void*, const char*) = nullptr;
    int (*CompileProgram)(void*, int, const char**) = nullptr;
    int (*GetProgramLogSize)(void*, size_t*) = nullptr;
    int (*GetProgramLog)(void*, char*) = nullptr;
    int (*GetLoweredName)(void*, const char*, const char**) = nullptr;
    int (*GetCodeSize)(void*, size_t*) = nullptr;
    int (*GetCode)(void*, char*) = nullptr;
    int (*DestroyProgram)(void**) = nullptr;
    bool ok = false;
};
Rtc& rtc() {
    static Rtc r = [] {
        Rtc x;
        for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"}) {
            x.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (x.lib) break;
        }
        if (!x.lib) return x;
        auto sym = [&](const char* n) { return dlsym(x.lib, n); };
        x.CreateProgram = (decltype(x.CreateProgram))sym("hiprtcCreateProgram");
        x.AddNameExpression = (decltype(x.AddNameExpression))sym("hiprtcAddNameExpression");
        x.CompileProgram = (decltype(x.CompileProgram))sym("hiprtcCompileProgram");
        x.GetProgramLogSize = (decltype(x.GetProgramLogSize))sym("hiprtcGetProgramLogSize");
        x.GetProgramLog = (decltype(x.GetProgramLog))sym("hiprtcGetProgramLog");
        x.GetLoweredName = (decltype(x.GetLoweredName))sym("hiprtcGetLoweredName");
        x.GetCodeSize = (decltype(x.GetCodeSize))sym("hiprtcGetCodeSize");
        x.GetCode = (decltype(x.GetCode))sym("hiprtcGetCode");
        x.DestroyProgram = (decltype(x.DestroyProgram))sym("hiprtcDestroyProgram");
        x.ok = x.CreateProgram && x.AddNameExpression && x.CompileProgram && x.GetProgramLogSize && x.GetProgramLog && x.GetLoweredName &&
               x.GetCodeSize && x.GetCode && x.DestroyProgram;
        return x;
    }();
    return r;
}

// what the pure half needs to know of a model, with the kernel of this entry: the EKF-type one and the sigma-point one
CustomModel custom_model(const cgp_custom_model* m, bool smoother) {
    if (!m) return {};
    return {true, m->kind, m->d, m->device, (smoother ? m->smoother : m->filter) != nullptr, (smoother ? m->sgp_smoother : m->sgp_filter) != nullptr};
}
template <class IO>
Verdict enqueue_custom(hipFunction_t kernel, IO& io, ModelArgs& ma, void* stream) {
    void* args[] = {&io, &ma};
    return hip_rc(hipModuleLaunchKernel(kernel, (unsigned)((io.B + 63) / 64), 1, 1, 64, 1, 1, 0, (hipStream_t)stream, args, nullptr));
}
// the second launch geometry, of a smoother with CGP_RK4_SUBSTEPS: one wavefront per trial, the sigma-point set staged in dynamic LDS
Verdict enqueue_custom_wave(hipFunction_t kernel, SmootherIO& io, ModelArgs& ma, int d, bool sigma, void* stream) {
    if (io.B > 0x7fffffffLL) return {CGP_E_UNSUPPORTED, "CGP_RK4_SUBSTEPS: a smoother runs one workgroup per trial: B must be < 2^31"};
    void* args[] = {&io, &ma};
    const unsigned dyn = sigma ? (unsigned)sigma_lds_bytes(ma, d) : 0u;
    return hip_rc(hipModuleLaunchKernel(kernel, (unsigned)io.B, 1, 1, 64, 1, 1, dyn, (hipStream_t)stream, args, nullptr));
}
}  // namespace

extern "C" {

int cgp_model_from_source(cgp_ctx* ctx, int kind, int32_t d, const char* body, const char* include_dir, cgp_custom_model** out) {
    if (!ctx) return CGP_E_ARG;
    if (!out) return fail(ctx, CGP_E_ARG, "out is NULL");
    *out = nullptr;
    if (kind != CGP_CUSTOM_DISCRETE && kind != CGP_CUSTOM_SDE && kind != CGP_CUSTOM_MEASUREMENT)
        return fail(ctx, CGP_E_ARG, "kind must be CGP_CUSTOM_DISCRETE, CGP_CUSTOM_SDE or CGP_CUSTOM_MEASUREMENT");
    if (d < 1 || d > 8) return fail(ctx, CGP_E_UNSUPPORTED, "custom models: state dimension 1..8");
    if (!body || !include_dir) return fail(ctx, CGP_E_ARG, "body / include_dir is NULL");
    Rtc& R = rtc();
    if (!R.ok) return fail(ctx, CGP_E_UNSUPPORTED, "libhiprtc.so could not be loaded: custom models need the runtime compiler of ROCm");
    DeviceScope on_device(ctx->device);
    if (!on_device.ok) return fail(ctx, CGP_E_HIP, "hipSetDevice failed");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess) return fail(ctx, CGP_E_HIP, "hipGetDeviceProperties failed");

    const std::string D = std::to_string(d);
    std::string src = "#include \"cgp_custom.hpp\"\nnamespace cgp_user {\nusing namespace cgp::ad;\n#line 1 \"model\"\n";
    src += body;
    // (the kernels take FilterIO / SmootherIO / ModelArgs BY VALUE: the headers under include_dir must be the ones this library was built from --
    // their sizes travel with the code object and are compared after loading)
    src += "\n}\nextern \"C\" __device__ const unsigned cgp_rtc_abi[3] = {(unsigned)sizeof(cgp::FilterIO), (unsigned)sizeof(cgp::SmootherIO), (unsigned)sizeof(cgp::ModelArgs)};\n"
           "struct CgpUserModel {\n";
    std::string f_name, s_name, sf_name, ss_name, fsub_name, ssub_name, sfsub_name, sssub_name;      // (sub: CGP_RK4_SUBSTEPS, SDE models)
    if (kind == CGP_CUSTOM_DISCRETE) {
        src += "    template <class T> __device__ static void mean(const T* u, const double* p, double dt, T* m) { cgp_user::cond_mean(u, p, dt, m); }\n"
               "    __device__ static void cov(const double* u, const double* p, double dt, double* c) { cgp_user::cond_cov(u, p, dt, c); }\n};\n"
               "using CgpUserM = cgp::CustomDisc<" + D + ", CgpUserModel>;\n";
        f_name = "cgp::filter_kernel<cgp::EkfPredict<CgpUserM, false>, cgp::LinearMeasurement<" + D + ">>";
        s_name = "cgp::smoother_kernel<cgp::EksStep<CgpUserM, false>>";
        sf_name = "cgp::filter_kernel<cgp::SgpPredictCustom<CgpUserM>, cgp::LinearMeasurement<" + D + ">>";
        ss_name = "cgp::smoother_kernel<cgp::SgpsStepCustom<CgpUserM>>";
    } else if (kind == CGP_CUSTOM_MEASUREMENT) {
        // ekf_for_kpt: linear dynamics (F, Sigma as the parameter vector), the caller's h -- a filter, nothing else
        src += "    template <class T> __device__ static T measure(const T* u, const double* q) { return cgp_user::measure(u, q); }\n};\n";
        f_name = "cgp::filter_kernel<cgp::EkfPredict<cgp::LinearDisc<" + D + ">, false>, cgp::CustomMeasurement<" + D + ", CgpUserModel>>";
    } else {
        src += "    template <class T> __device__ static void drift(const T* u, const double* p, T* a) { cgp_user::drift(u, p, a); }\n};\n"
               "using CgpUserM = cgp::CustomSDE<" + D + ", CgpUserModel>;\n";
        f_name = "cgp::filter_kernel<cgp::CdEkfPredict<CgpUserM, false>, cgp::LinearMeasurement<" + D + ">>";
        s_name = "cgp::smoother_kernel<cgp::CdEksStep<CgpUserM, false>>";
        sf_name = "cgp::filter_kernel<cgp::CdSgpPredict<CgpUserM, false>, cgp::LinearMeasurement<" + D + ">>";
        ss_name = "cgp::smoother_kernel<cgp::CdSgpsStep<CgpUserM, false>>";
        fsub_name = "cgp::filter_kernel<cgp::SubstepPredict<cgp::CdEkfPredict<CgpUserM, false>>, cgp::LinearMeasurement<" + D + ">>";
        ssub_name = "cgp::smoother_kernel<cgp::SubstepSmooth<cgp::CdEksStep<CgpUserM, true>>>";
        sfsub_name = "cgp::filter_kernel<cgp::SubstepPredict<cgp::CdSgpPredict<CgpUserM, false>>, cgp::LinearMeasurement<" + D + ">>";
        sssub_name = "cgp::smoother_kernel<cgp::SubstepSmooth<cgp::CdSgpsStep<CgpUserM, true>>>";
    }
    void* prog = nullptr;
    if (R.CreateProgram(&prog, src.c_str(), "cgp_custom_model.hip", 0, nullptr, nullptr) != 0) return fail(ctx, CGP_E_HIP, "hiprtcCreateProgram failed");
    auto done = [&](int code, const std::string& msg) { R.DestroyProgram(&prog); return fail(ctx, code, msg); };
    constexpr int kNames = 8;
    const std::string* names[kNames] = {&f_name, &s_name, &sf_name, &ss_name, &fsub_name, &ssub_name, &sfsub_name, &sssub_name};
    for (const std::string* n : names)
        if (!n->empty() && R.AddNameExpression(prog, n->c_str()) != 0) return done(CGP_E_HIP, "hiprtcAddNameExpression failed");
    const std::string arch = std::string("--offload-arch=") + prop.gcnArchName;
    const std::string inc1 = std::string("-I") + include_dir, inc2 = std::string("-I") + include_dir + "/../../include";
    const char* opts[] = {arch.c_str(), "-std=c++17", "-O3", "-fno-fast-math", inc1.c_str(), inc2.c_str()};
    const int rc = R.CompileProgram(prog, 6, opts);
    if (rc != 0) {
        size_t n = 0;
        std::string log;
        if (R.GetProgramLogSize(prog, &n) == 0 && n > 1) { log.resize(n); R.GetProgramLog(prog, &log[0]); }
        if (log.size() > 6000) log.resize(6000);
        return done(CGP_E_ARG, "the model source does not compile:\n" + log);
    }
    const char* low[kNames] = {};
    size_t size = 0;
    for (int i = 0; i < kNames; i++)
        if (!names[i]->empty() && R.GetLoweredName(prog, names[i]->c_str(), &low[i]) != 0) return done(CGP_E_HIP, "hiprtc: no lowered name");
    if (R.GetCodeSize(prog, &size) != 0) return done(CGP_E_HIP, "hiprtc: no code");
    std::vector<char> code(size);
    if (R.GetCode(prog, code.data()) != 0) return done(CGP_E_HIP, "hiprtcGetCode failed");
    cgp_custom_model* m = new cgp_custom_model;
    m->kind = kind; m->d = d; m->device = ctx->device;
    hipFunction_t* fns[kNames] = {&m->filter, &m->smoother, &m->sgp_filter, &m->sgp_smoother, &m->filter_sub, &m->smoother_sub, &m->sgp_filter_sub, &m->sgp_smoother_sub};
    bool loaded = hipModuleLoadData(&m->module, code.data()) == hipSuccess;
    for (int i = 0; loaded && i < kNames; i++)
        if (low[i]) loaded = hipModuleGetFunction(fns[i], m->module, low[i]) == hipSuccess;
    if (!loaded) {
        const std::string why = hipGetErrorString(hipGetLastError());
        if (m->module) (void)hipModuleUnload(m->module);
        delete m;
        return done(CGP_E_HIP, "loading the compiled model failed: " + why);
    }
    {
        hipDeviceptr_t abi_ptr = nullptr;
        size_t abi_bytes = 0;
        unsigned abi[3] = {0, 0, 0};
        const bool read = hipModuleGetGlobal(&abi_ptr, &abi_bytes, m->module, "cgp_rtc_abi") == hipSuccess && abi_bytes == sizeof(abi) &&
                          hipMemcpy(abi, abi_ptr, sizeof(abi), hipMemcpyDeviceToHost) == hipSuccess;
        if (!read || abi[0] != sizeof(FilterIO) || abi[1] != sizeof(SmootherIO) || abi[2] != sizeof(ModelArgs)) {
            (void)hipModuleUnload(m->module);
            delete m;
            return done(CGP_E_ARG, "the headers under include_dir are not the ones this library was built from (argument structs differ in size): "
                                   "point include_dir at the csrc/ of this build");
        }
    }
    R.DestroyProgram(&prog);
    *out = m;
    return CGP_OK;
}

void cgp_custom_model_destroy(cgp_custom_model* m) {
    if (!m) return;
    {
        DeviceScope on_device(m->device);
        if (m->module) (void)hipModuleUnload(m->module);
    }
    delete m;
}


int cgp_filter_custom(cgp_ctx* ctx, const cgp_custom_model* m, const cgp_sigma* sigma, const double* params, int64_t param_stride, const double* gamma, int64_t gamma_stride,
                      const cgp_init* init, double dt, const double* ys, int64_t ys_stride, int64_t ys_repeat, const int32_t* ys_index,
                      int64_t B, int64_t T, double* mfs, double* Pfs, double* nll, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    FilterIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_filter_custom(custom_model(m, false), sigma, params, param_stride, gamma, gamma_stride, init, dt, ys, ys_stride, ys_repeat,
                                                   ys_index, B, T, mfs, Pfs, nll, flags, host_of(ctx), io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        if (ma.substeps > 1) return enqueue_custom(sigma ? m->sgp_filter_sub : m->filter_sub, io, ma, stream);
        return enqueue_custom(sigma ? m->sgp_filter : m->filter, io, ma, stream);
    });
}

int cgp_smoother_custom(cgp_ctx* ctx, const cgp_custom_model* m, const cgp_sigma* sigma, const double* params, int64_t param_stride, const double* gamma, int64_t gamma_stride,
                        double dt, const double* mfs, const double* Pfs, int64_t B, int64_t T, double* mss, double* Pss, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    SmootherIO io{};
    ModelArgs ma;
    const Verdict prepared = prepare_smoother_custom(custom_model(m, true), sigma, params, param_stride, gamma, gamma_stride, dt, mfs, Pfs, B, T, mss, Pss, flags,
                                                     host_of(ctx), io, ma);
    return launch_on(ctx, prepared, kLaunchLocked, [&]() -> Verdict {
        if (ma.substeps > 1) return enqueue_custom_wave(sigma ? m->sgp_smoother_sub : m->smoother_sub, io, ma, m->d, sigma != nullptr, stream);
        return enqueue_custom(sigma ? m->sgp_smoother : m->smoother, io, ma, stream);
    });
}

}  // extern "C"
