// Input side of the path: cgp_simulate, cgp_simulate_x0, cgp_add_noise and the Philox test hook.
#include "cgp_simulate.hpp"
#include "cgp_ctx.hpp"

namespace cgp {
int dispatch_simulate(int model_id, int key, bool wave, const SimIO& io, const ModelArgs& ma, hipStream_t st) {
    if (model_id == CGP_M_LINEAR) {
        switch (key) {
        case 1: return launch_simulate<LinearDisc<1>>(wave, io, ma, st);
        case 2: return launch_simulate<LinearDisc<2>>(wave, io, ma, st);
        case 3: return launch_simulate<LinearDisc<3>>(wave, io, ma, st);
        case 4: return launch_simulate<LinearDisc<4>>(wave, io, ma, st);
        case 5: return launch_simulate<LinearDisc<5>>(wave, io, ma, st);
        case 6: return launch_simulate<LinearDisc<6>>(wave, io, ma, st);
        case 8: return launch_simulate<LinearDisc<8>>(wave, io, ma, st);
        default: return CGP_E_UNSUPPORTED;
        }
    }
    switch (key) {
    case 1: return launch_simulate<HarmonicLCD<1>>(wave, io, ma, st);
    case 2: return launch_simulate<HarmonicLCD<2>>(wave, io, ma, st);
    case 3: return launch_simulate<HarmonicLCD<3>>(wave, io, ma, st);
    default: return CGP_E_UNSUPPORTED;
    }
}

template <int D>
static int launch_x0(const double* m0, int64_t m0_stride, const double* P0, int64_t P0_stride, uint64_t seed, int64_t trial0, int64_t B,
                     double* x0, hipStream_t st) {
    hipLaunchKernelGGL((simulate_x0_kernel<D>), dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, m0, m0_stride, P0, P0_stride, seed, trial0, B, x0);
    return hip_rc(hipGetLastError());
}

int dispatch_simulate_x0(int d, const double* m0, int64_t m0_stride, const double* P0, int64_t P0_stride, uint64_t seed, int64_t trial0,
                         int64_t B, double* x0, hipStream_t st) {
    switch (d) {
    case 1: return launch_x0<1>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 2: return launch_x0<2>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 3: return launch_x0<3>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 4: return launch_x0<4>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 5: return launch_x0<5>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 6: return launch_x0<6>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 7: return launch_x0<7>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    case 8: return launch_x0<8>(m0, m0_stride, P0, P0_stride, seed, trial0, B, x0, st);
    default: return CGP_E_UNSUPPORTED;
    }
}
}  // namespace cgp

using namespace cgp;

extern "C" {

int cgp_simulate(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, double dt, uint64_t seed, int64_t trial0,
                 int64_t B, int64_t T, double* xs, double* ys, uint32_t flags, void* stream) {
    if (!ctx) return CGP_E_ARG;
    SimIO io{};
    ModelArgs ma;
    SimShape shape;
    return launch_on(ctx, prepare_simulate(model, init, dt, seed, trial0, B, T, xs, ys, flags, host_of(ctx), io, ma, shape), kLaunchUnlocked, [&]() -> Verdict {
        const int rc = dispatch_simulate(model->model_id, shape.key, shape.wave, io, ma, (hipStream_t)stream);
        if (rc == CGP_E_UNSUPPORTED) return {rc, "this (model, dimension) combination is not compiled in"};
        return rc;
    });
}

int cgp_simulate_x0(cgp_ctx* ctx, const cgp_model* model, const cgp_init* init, uint64_t seed, int64_t trial0, int64_t B, double* x0, void* stream) {
    if (!ctx) return CGP_E_ARG;
    return launch_on(ctx, prepare_simulate_x0(model, init, trial0, B, x0), kLaunchUnlocked, [&]() -> Verdict {
        return dispatch_simulate_x0(model->d, init->m0, init->m0_stride, init->P0, init->P0_stride, seed, trial0, B, x0, (hipStream_t)stream);
    });
}

int cgp_add_noise(cgp_ctx* ctx, const double* clean, int64_t clean_stride, const double* Xi, int64_t Xi_stride,
                  uint64_t seed, int64_t trial0, int64_t B, int64_t T, double* ys, void* stream) {
    if (!ctx) return CGP_E_ARG;
    return launch_on(ctx, prepare_add_noise(clean, clean_stride, Xi, trial0, B, T, ys), kLaunchUnlocked, [&]() -> Verdict {
        const int64_t total = B * ((T + 1) / 2), blocks = (total + 255) / 256;
        const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
        hipLaunchKernelGGL(add_noise_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, clean, clean_stride, Xi, Xi_stride, seed, trial0, B, T, ys);
        return hip_rc(hipGetLastError());
    });
}

int cgp_debug_philox(cgp_ctx* ctx, const uint32_t* ctr, const uint32_t* key, int64_t n, uint32_t* out, void* stream) {
    if (!ctx) return CGP_E_ARG;
    return launch_on(ctx, prepare_debug_philox(ctr, key, n, out), kLaunchUnlocked, [&]() -> Verdict {
        const int64_t blocks = (n + 255) / 256;
        hipLaunchKernelGGL(debug_philox_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, ctr, key, n, out);
        return hip_rc(hipGetLastError());
    });
}

}  // extern "C"
