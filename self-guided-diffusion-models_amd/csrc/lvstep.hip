// Ancestral ('native') sampler update of a learned-variance model (Nichol & Dhariwal 2021; gfx950; include/sgdm_hip.h:
// sgd_ddpm_lv_step; the reference has no learned variance): ONE element-wise, HBM-bound launch per UNet evaluation that reads
// the raw network output [2b | b, hw, 2C] -- mean channels [0, C) through guided(), variance channels [C, 2C) from the
// conditional half alone (GLIDE's rule: guidance acts on the mean only) -- and performs
//   x0    = k0 x - k1 m                      (eps: sqrt_recip, sqrt_recipm1 | x0: 0, -1 | v: sa, s1; time is uniform over the batch)
//   clip != 0: x0 = min(max(x0, -1), 1)
//   frac  = (v + 1) / 2,   lv = frac max_log + (1 - frac) min_log
//   x_out = k2 x0 + k3 x + exp(0.5 lv) * kz * z          (z is not read when kz == 0)
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like vstep.hip: every product is rounded before it is
// added, so a torch-fp32 restatement reproduces the update (tests/test_hip_learned_variance.py); exp is the one transcendental.
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// one thread per NCHW element, like the other step kernels.  x / x_out carry no __restrict__: the update may run in place
__global__ __launch_bounds__(256) void ddpm_lv_step_kernel(const float* x, const float* __restrict__ out, const float* __restrict__ z,
                                                           int cfg_mode, float w, const sgd_lvstep_row* __restrict__ row, int clip,
                                                           int b, int c, int hw, float* x_out, float* __restrict__ x0_out) {
    const long count = (long)b * c * hw;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float k0 = row->k0, k1 = row->k1, k2 = row->k2, k3 = row->k3, mx = row->max_log, mn = row->min_log, kz = row->kz;
    const auto [n, cc, p] = nchw_split(i, c, hw);
    const float m = guided(out, cfg_mode, w, b, n, 2 * c, hw, cc, p);
    const float v = out[((long)n * hw + p) * (2 * c) + c + cc];
    const float xi = x[i];
    float x0 = k0 * xi - k1 * m;
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    float acc = k2 * x0 + k3 * xi;
    if (kz != 0.f) {
        const float frac = (v + 1.f) * 0.5f;
        const float lv = frac * mx + (1.f - frac) * mn;
        acc = acc + (expf(0.5f * lv) * kz) * z[i];
    }
    if (x0_out) x0_out[i] = x0;
    x_out[i] = acc;
}

}  // namespace

extern "C" int sgd_ddpm_lv_step(const float* x, const float* out, const float* z, int32_t cfg_mode, float w,
                                const sgd_lvstep_row* row_dev, int32_t clip, int32_t b, int32_t c, int32_t hw, float* x_out,
                                float* x0_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !out || !row_dev || !x_out || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 || cfg_mode > 2) return SGD_ERR_ARG;
    if (2L * b > INT32_MAX || 2L * b * c > INT32_MAX || ((long)b * c * hw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(ddpm_lv_step_kernel, dim3(nblk((long)b * c * hw)), dim3(256), 0, (hipStream_t)stream, x, out, z, cfg_mode, w,
                       row_dev, clip, b, c, hw, x_out, x0_out);
    return sgd_check_launch();
}
