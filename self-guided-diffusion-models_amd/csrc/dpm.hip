// DPM-Solver++(2M) sampler update (gfx950): one element-wise launch per UNet evaluation, first- and second-order rows alike.
// Lu et al. 2022, "DPM-Solver++", Algorithm 2 (multistep, data prediction); the reference has no such sampler.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like pndm.hip: every product below is rounded before
// it is added, so the update is a fixed sequence of correctly rounded IEEE fp32 adds and multiplies that a torch-fp32
// restatement reproduces bit for bit (tests/test_hip_dpmsolver.py).  All scalars come from the host (float64, rounded once):
// no division and no sqrt on the device.
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// x / x_out carry no __restrict__: the update may run in place
__global__ __launch_bounds__(256) void dpmpp_step_kernel(const float* x, const float* __restrict__ eps, int cfg_mode, float w,
                                                         const sgd_dpmpp_row* __restrict__ row, float* __restrict__ x0_hist,
                                                         int clip, int b, int c, int hw, float* x_out) {
    const long count = (long)b * c * hw;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float s1ma = row->s1ma, rsa = row->rsa, A = row->A, B = row->B, kc = row->cc, kp = row->cp;
    const auto [n, cc, p] = nchw_split(i, c, hw);
    const float e = guided(eps, cfg_mode, w, b, n, c, hw, cc, p);
    const float xi = x[i];
    float x0 = (xi - s1ma * e) * rsa;                       // data prediction
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    float D = kc * x0;
    if (kp != 0.f) D = D + kp * x0_hist[i];                 // first-order rows never read the (maybe uninitialised) history
    x0_hist[i] = x0;
    x_out[i] = A * xi + B * D;
}

}  // namespace

extern "C" int sgd_dpmpp_step(const float* x, const float* eps_nhwc, int32_t cfg_mode, float w, const sgd_dpmpp_row* row_dev,
                              float* x0_hist, int32_t clip, int32_t b, int32_t c, int32_t hw, float* x_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !eps_nhwc || !row_dev || !x0_hist || !x_out || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 || cfg_mode > 2)
        return SGD_ERR_ARG;
    if ((long)b * c > INT32_MAX || ((long)b * c * hw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(dpmpp_step_kernel, dim3(nblk((long)b * c * hw)), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, cfg_mode,
                       w, row_dev, x0_hist, clip, b, c, hw, x_out);
    return sgd_check_launch();
}
