// Data-form sampler update for parameterization 'v' (gfx950): ONE element-wise, HBM-bound launch per UNet evaluation that
// reads the network output as v and performs the 'native' (ancestral), 'ddim' or 'dpmsolver' update in the variables
//   x0 = sa x - s1 v,   eps = sa v + s1 x        (sa = sqrt(alphas_cumprod[t]), s1 = sqrt(1 - alphas_cumprod[t]))
// which are finite at every SNR, sa = 0 included: the form a zero-terminal-SNR schedule (Lin et al. 2023, "Common Diffusion
// Noise Schedules and Sample Steps Are Flawed") needs, where the eps form x0 = (x - s1 eps) / sa is 0 / 0.  It replaces the pair
// sgd_v_to_eps + update kernel of the eps form.  The reference has no such parameterization.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like dpm.hip and vpred.hip: every product below is
// rounded before it is added, so the update is a fixed sequence of correctly rounded IEEE fp32 adds and multiplies that a
// torch-fp32 restatement reproduces bit for bit (tests/test_hip_ztsnr.py).  All row scalars come from the host (float64,
// rounded once): no division and no sqrt on the device.
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// one thread per NCHW element, like the other step kernels: x, z, x0_hist and x_out are read and written at consecutive
// addresses by consecutive lanes; v_out goes through guided().  x / x_out carry no __restrict__: the update may run in place
__global__ __launch_bounds__(256) void v_step_kernel(const float* x, const float* __restrict__ v_out, const float* __restrict__ z,
                                                     int cfg_mode, float w, const int64_t* __restrict__ t,
                                                     const float* __restrict__ sa, const float* __restrict__ s1,
                                                     const sgd_vstep_row* __restrict__ row, float* __restrict__ x0_hist, int clip,
                                                     int b, int c, int hw, float* x_out) {
    const long count = (long)b * c * hw;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float kx = row->kx, k0 = row->k0, ke = row->ke, kz = row->kz, kh = row->kh;
    const auto [n, cc, p] = nchw_split(i, c, hw);
    const float vg = guided(v_out, cfg_mode, w, b, n, c, hw, cc, p);
    const int64_t tt = t[n];
    const float a = sa[tt], s = s1[tt];
    const float xi = x[i];
    float x0 = a * xi - s * vg;                             // data prediction: finite at a == 0
    const float eps = a * vg + s * xi;                      // the bits of sgd_v_to_eps
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    float acc = kx * xi + k0 * x0;
    if (ke != 0.f) acc = acc + ke * eps;
    if (kh != 0.f) acc = acc + kh * x0_hist[i];             // rows without history never read the (maybe uninitialised) buffer
    if (kz != 0.f) acc = acc + kz * z[i];                   // z may be NULL when no row has noise
    x0_hist[i] = x0;
    x_out[i] = acc;
}

}  // namespace

extern "C" int sgd_v_step(const float* x, const float* v_out, const float* z, int32_t cfg_mode, float w, const int64_t* t,
                          const float* sqrt_ac, const float* sqrt_1mac, const sgd_vstep_row* row_dev, float* x0_hist,
                          int32_t clip, int32_t b, int32_t c, int32_t hw, float* x_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !v_out || !t || !sqrt_ac || !sqrt_1mac || !row_dev || !x0_hist || !x_out || b <= 0 || c <= 0 || hw <= 0 ||
        cfg_mode < 0 || cfg_mode > 2)
        return SGD_ERR_ARG;
    if (2L * b > INT32_MAX || (long)b * c > INT32_MAX || ((long)b * c * hw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(v_step_kernel, dim3(nblk((long)b * c * hw)), dim3(256), 0, (hipStream_t)stream, x, v_out, z, cfg_mode, w,
                       t, sqrt_ac, sqrt_1mac, row_dev, x0_hist, clip, b, c, hw, x_out);
    return sgd_check_launch();
}
