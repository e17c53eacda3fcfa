// What does the EKF kernel's parking write cost as the kernel issues it?  (cgp_mfma4.hpp: every step all 64 lanes write the same
// 16 bytes -- S and the innovation -- to the step's LDS slot with one ds_write_b128, picked up per lane at the 64-step NLL flush.)
// One wavefront on one SIMD; a "step" is a chain of 16 dependent v_fma_f64 with the write of the chain's value behind it, eight
// steps per loop iteration with the slot in the instruction's offset, as in the kernel.  Ticks per step, minus the chain alone:
//   all      ds_write_b128, 64 lanes active, one address                        (what the kernel does)
//   exec16 / exec4 / exec1   the same with 16 / 4 / 1 lanes active: the mask sits in a scalar pair set once per 8-step group,
//            EXEC is switched to it and back around each write
//   buffer   two raw buffer stores (b64) into a workspace row, lane 0's offset inside the window, the others' beyond it
//            (the OobWindow form of the kernel's output stores)
//   hipcc --offload-arch=gfx950 -O3 -o park_write park_write.hip && ./park_write
#include <hip/hip_runtime.h>
#include <cstdio>
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
enum { NONE, ALL, EXEC16, EXEC4, EXEC1, BUFFER };
constexpr int kChain = 16;

template <int KIND> __global__ void k(double* out, double* ws, long long* cyc, int n) {
    __shared__ double park[64 * 4];                                          // 64 slots of 32 bytes, as in the kernel
    const int lane = threadIdx.x;
    double x = 0.25 + lane * 1e-9, a = 0.999, b = 1e-3;
    asm volatile("" : "+v"(x), "+v"(a), "+v"(b));
    const unsigned long long mask = KIND == EXEC16 ? 0xFFFFull : KIND == EXEC4 ? 0xFull : 0x1ull;
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)ws, 0, 64 * 16, 0x27000);
    const unsigned boff = lane == 0 ? 0u : 0x80000000u;
    park[lane] = 0.0; park[64 + lane] = 0.0; park[128 + lane] = 0.0; park[192 + lane] = 0.0;
    __syncthreads();
    const long long t0 = __builtin_readcyclecounter();
    for (int i = 0; i < n; i++) {
        const unsigned addr = (unsigned)(i & 7) * 256u;                     // the 8-step group's first slot
        unsigned long long m = mask;
        asm volatile("" : "+s"(m));                                          // (the mask in a scalar pair, set per group)
#pragma unroll
        for (int j = 0; j < 8; j++) {
#pragma unroll
            for (int c = 0; c < kChain; c++) x = fma(x, a, b);
            const double innov = x - b;                                      // (off the chain, as the innovation is)
            u32x4 v; v.x = (unsigned)__double2loint(x); v.y = (unsigned)__double2hiint(x); v.z = (unsigned)__double2loint(innov); v.w = (unsigned)__double2hiint(innov);
            if (KIND == ALL)
                asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(addr), "v"(v), "i"(32 * j) : "memory");
            if (KIND == EXEC16 || KIND == EXEC4 || KIND == EXEC1)
                asm volatile("s_mov_b64 exec, %3\n\tds_write_b128 %0, %1 offset:%2\n\ts_mov_b64 exec, -1" :: "v"(addr), "v"(v), "i"(32 * j), "s"(m) : "memory");
            if (KIND == BUFFER) {
                u32x2 lo, hi; lo.x = v.x; lo.y = v.y; hi.x = v.z; hi.y = v.w;
                __builtin_amdgcn_raw_buffer_store_b64(lo, rsrc, (int)boff, (int)(addr / 2 + 16 * j), 0);
                __builtin_amdgcn_raw_buffer_store_b64(hi, rsrc, (int)(boff + 8u), (int)(addr / 2 + 16 * j), 0);
            }
        }
    }
    const long long t1 = __builtin_readcyclecounter();
    __syncthreads();
    out[lane] = x + park[lane] + park[64 + lane] + park[128 + lane] + park[192 + lane];
    if (lane == 0) cyc[0] = t1 - t0;
}
template <int KIND> double run(double* out, double* ws, long long* cyc) {
    const int n = 1 << 13; long long h = 0;
    for (int rep = 0; rep < 2; rep++) {
        hipLaunchKernelGGL((k<KIND>), dim3(1), dim3(64), 0, 0, out, ws, cyc, n);
        if (hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost) != hipSuccess) { printf("launch failed\n"); exit(1); }
    }
    return (double)h / n / 8;
}
int main() {
    double *out, *ws; long long* cyc;
    if (hipMalloc(&out, 64 * sizeof(double)) != hipSuccess || hipMalloc(&ws, 64 * 16) != hipSuccess || hipMalloc(&cyc, 8) != hipSuccess) return 1;
    const double none = run<NONE>(out, ws, cyc);
    printf("ticks per step (chain of %d dependent v_fma_f64): chain alone %.2f\n", kChain, none);
    const double all = run<ALL>(out, ws, cyc), e16 = run<EXEC16>(out, ws, cyc), e4 = run<EXEC4>(out, ws, cyc), e1 = run<EXEC1>(out, ws, cyc);
    const double buf = run<BUFFER>(out, ws, cyc);
    printf("added by the parking write:  all %.2f   exec16 %.2f   exec4 %.2f   exec1 %.2f   buffer (two stores) %.2f\n",
           all - none, e16 - none, e4 - none, e1 - none, buf - none);
    // the slots hold what the last group wrote whatever the form (lane 0's value in the restricted forms)
    double h[64];
    if (hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("check %.6f\n", h[0]);
    return 0;
}
