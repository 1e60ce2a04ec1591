// PNDM sampler update (gfx950): one element-wise launch per UNet evaluation, Runge-Kutta warm-up and linear multistep alike.
// Reference: diffusion/sampler/pndm_sampler.py:96-141 (step_prk, step_plms, transfer).
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS): every product below is rounded before it is added,
// which is the operation sequence of the reference's torch ops.  (The clang pragma `fp contract(off)` does not override
// -ffp-contract=fast, so the flag has to come from the command line.)  With the per-evaluation scalars formed on the host
// from the reference's fp32 expressions in IEEE arithmetic, a step fed the reference's residual reproduces the reference's
// image bit for bit.
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// the reference's Python constants 1/6, 1/3, 1/24 as torch casts them for an fp32 tensor (double -> nearest fp32)
constexpr float K16 = 0x1.555556p-3f, K13 = 0x1.555556p-2f, K124 = 0x1.555556p-5f;

// x / x_out carry no __restrict__: the update may run in place
__global__ __launch_bounds__(256) void pndm_step_kernel(const float* x, const float* __restrict__ eps, int cfg_mode, float w,
                                                        const sgd_pndm_row* __restrict__ row, float* __restrict__ acc,
                                                        float* __restrict__ base, float* __restrict__ ring, int b, int c,
                                                        int hw, float* x_out) {
    const long count = (long)b * c * hw;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int phase = row->phase;
    const float d = row->d, c1 = row->c1, c2 = row->c2;
    // ring slots reduced mod 3: a malformed row can mix up the history but never address outside the ring
    const long s1 = (unsigned)row->slot1 % 3u, s2 = (unsigned)row->slot2 % 3u, s3 = (unsigned)row->slot3 % 3u;
    const auto [n, cc, p] = nchw_split(i, c, hw);
    const float e = guided(eps, cfg_mode, w, b, n, c, hw, cc, p);
    float src, r;                                           // transfer(src, t, t_next, r)
    if (phase == SGD_PNDM_RK0) {                            // step_prk, t % 4 == 0 (cur_residual starts from int 0)
        src = x[i];
        acc[i] = K16 * e;
        base[i] = src;
        ring[s1 * count + i] = e;                           // ets.append(residual)
        r = e;
    } else if (phase == SGD_PNDM_RK12) {                    // t % 4 == 1, 2
        acc[i] = acc[i] + K13 * e;
        src = base[i];
        r = e;
    } else if (phase == SGD_PNDM_RK3) {                     // t % 4 == 3
        src = base[i];
        r = acc[i] + K16 * e;
    } else {                                                // step_plms: ets[-1] = e, ets[-2..-4] = slot1..slot3
        src = x[i];
        const float e2 = ring[s1 * count + i], e3 = ring[s2 * count + i];
        float* const r4 = ring + s3 * count + i;
        const float e4 = *r4;
        r = K124 * (55.f * e - 59.f * e2 + 37.f * e3 - 9.f * e4);
        *r4 = e;                                            // the oldest entry leaves the window
    }
    x_out[i] = src + d * (c1 * src - c2 * r);               // Eq. 9 (pndm_sampler.py:137-141)
}

}  // namespace

extern "C" int sgd_pndm_step(const float* x, const float* eps_nhwc, int32_t cfg_mode, float w, const sgd_pndm_row* row_dev,
                             float* acc, float* base, float* ring, int32_t b, int32_t c, int32_t hw, float* x_out,
                             void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !eps_nhwc || !row_dev || !acc || !base || !ring || !x_out || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 ||
        cfg_mode > 2)
        return SGD_ERR_ARG;
    if ((long)b * c > INT32_MAX || ((long)b * c * hw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(pndm_step_kernel, dim3(nblk((long)b * c * hw)), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc,
                       cfg_mode, w, row_dev, acc, base, ring, b, c, hw, x_out);
    return sgd_check_launch();
}
