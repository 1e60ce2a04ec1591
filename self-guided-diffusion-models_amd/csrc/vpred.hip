// v-prediction (Salimans & Ho 2022, "Progressive Distillation", section 4; the reference has no such parameterization):
//   v = sa[t] * noise - s1[t] * x_start,   sa = sqrt(alphas_cumprod), s1 = sqrt(1 - alphas_cumprod)
// Two element-wise, HBM-bound passes (gfx950): the training-side q_sample that also forms the target, and the sampling-side
// change of variables from a (guided) v to the eps every update kernel reads.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like pndm.hip and dpm.hip: every product below is
// rounded before it is added, so a torch-fp32 restatement reproduces the outputs bit for bit (tests/test_hip_vpred.py).
// x_noisy carries the bits of sgd_q_sample (csrc/backward.hip): that unit allows contraction, but its kernel is compiled to
// one packed multiply of both products and an add, i.e. the same two rounded products; the test compares the two launches.
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// one thread per element: consecutive lanes read and write consecutive addresses of all four tensors
__global__ __launch_bounds__(256) void q_sample_v_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                                         const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                         const float* __restrict__ s1, int b, long chw,
                                                         float* __restrict__ x_noisy, float* __restrict__ v) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)b * chw) return;
    const int n = i / chw;
    const int64_t tt = t[n];
    const float a = sa[tt], s = s1[tt], xi = x0[i], ni = noise[i];
    x_noisy[i] = a * xi + s * ni;                           // == sgd_q_sample (ddpm_sampler.py:116-119)
    v[i] = a * ni - s * xi;
}

// one thread per PIXEL, looping over its channels.  x is hw-major (NCHW): per channel the 64 lanes of a wave read 256
// consecutive bytes.  v and eps_out are c-minor: a lane touches c consecutive floats, a wave 64 * c * 4 consecutive bytes,
// every byte of which it uses over the c iterations.  (One thread per element would be coalesced on one side only and
// split each wave's accesses to the other into c short runs.)
__global__ __launch_bounds__(256) void v_to_eps_kernel(const float* __restrict__ x, const float* __restrict__ v,
                                                       const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                       const float* __restrict__ s1, int cfg_mode, float w, int b, int c, int hw,
                                                       float* __restrict__ eps_out) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;          // (n, p)
    if (i >= (long)b * hw) return;
    const int p = i % hw, n = i / hw;
    const int64_t tt = t[n];
    const float a = sa[tt], s = s1[tt];
    for (int cc = 0; cc < c; ++cc) {
        const float vg = guided(v, cfg_mode, w, b, n, c, hw, cc, p);
        const float xi = x[((long)n * c + cc) * hw + p];
        eps_out[i * c + cc] = a * vg + s * xi;
    }
}

}  // namespace

extern "C" int sgd_q_sample_v(const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                              int32_t b, int64_t chw, float* x_noisy_out, float* v_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!x0 || !noise || !t || !sqrt_ac || !sqrt_1mac || !x_noisy_out || !v_out || b <= 0 || chw <= 0) return SGD_ERR_ARG;
    if (chw > INT64_MAX / b || ((long)b * chw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(q_sample_v_kernel, dim3(nblk((long)b * chw)), dim3(256), 0, (hipStream_t)stream, x0, noise, t, sqrt_ac,
                       sqrt_1mac, b, (long)chw, x_noisy_out, v_out);
    return sgd_check_launch();
}

extern "C" int sgd_v_to_eps(const float* x, const float* v_out, const int64_t* t, const float* sqrt_ac, const float* sqrt_1mac,
                            int32_t cfg_mode, float w, int32_t b, int32_t c, int32_t hw, float* eps_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !v_out || !t || !sqrt_ac || !sqrt_1mac || !eps_out || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 || cfg_mode > 2)
        return SGD_ERR_ARG;
    if (2L * b > INT32_MAX || ((long)b * hw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(v_to_eps_kernel, dim3(nblk((long)b * hw)), dim3(256), 0, (hipStream_t)stream, x, v_out, t, sqrt_ac,
                       sqrt_1mac, cfg_mode, w, b, c, hw, eps_out);
    return sgd_check_launch();
}
