// Guidance pass between the UNet and a sampler update (gfx950): the guided network output written to a [b, hw, c] buffer
// that every update kernel (and sgd_v_to_eps) then reads with cfg_mode = 0.  Two things the fused combine inside the update
// kernels cannot do live here (include/sgdm_hip.h: sgd_cfg_guide; neither has a counterpart in the reference):
//   * the guidance weight is read from DEVICE memory, so a captured step serves any per-step weight schedule;
//   * CFG rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4): the guided
//     output of each sample is scaled towards the standard deviation of the conditional output.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like pndm.hip, dpm.hip and vpred.hip: guided() rounds
// each product before it is added, so rescale = 0 reproduces a torch-fp32 restatement bit for bit (tests/test_hip_cfg_schedule.py).
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

constexpr int GUIDE_THREADS = 1024;                 // one workgroup per sample: 16 waves
constexpr int GUIDE_WAVES = GUIDE_THREADS / 64;

// rescale == 0: element-wise, one thread per element ([hw, c] of a sample is one flat run: c = 1, hw = c * hw)
__global__ __launch_bounds__(256) void cfg_guide_kernel(const float* __restrict__ out, int cfg_mode,
                                                        const float* __restrict__ w_dev, int b, long chw,
                                                        float* __restrict__ g_out) {
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= (long)b * chw) return;
    const float w = *w_dev;
    const float oc = out[i];
    const float ou = out[(long)b * chw + i];
    g_out[i] = cfg_mode == 1 ? (1.f - w) * ou + w * oc : (1.f + w) * oc - w * ou;
}

// sum of two per-thread values over the workgroup, in a fixed order: xor-shuffles inside each wave (every lane ends with the
// wave's sum), one LDS slot per wave, then every thread adds the GUIDE_WAVES slots in ascending order.  No atomics: the
// result depends on the input alone.
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*red)[GUIDE_WAVES]) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    __syncthreads();                                // the previous reduction's slots have been read by everyone
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = a;
        red[1][wave] = b;
    }
    __syncthreads();
    a = 0.f;
    b = 0.f;
    for (int i = 0; i < GUIDE_WAVES; ++i) {
        a += red[0][i];
        b += red[1][i];
    }
}

// rescale > 0: one workgroup per sample, three passes over the sample's two halves (2 x chw floats: 96 KiB at the flagship
// size, L2-resident after the first pass): means, centred squares, scaled write.  g is re-formed in each pass by the same
// rounded operations, so the three passes see the same bits.
__global__ __launch_bounds__(GUIDE_THREADS) void cfg_guide_rescale_kernel(const float* __restrict__ out, int cfg_mode,
                                                                          const float* __restrict__ w_dev, float rescale,
                                                                          int b, int chw, float* __restrict__ g_out) {
    __shared__ float red[2][GUIDE_WAVES];
    const int n = blockIdx.x;
    const float w = *w_dev;
    float sc = 0.f, sg = 0.f;
    for (int e = threadIdx.x; e < chw; e += GUIDE_THREADS) {
        sc += out[(long)n * chw + e];
        sg += guided(out, cfg_mode, w, b, n, 1, chw, 0, e);
    }
    block_sum2(sc, sg, red);
    const float mc = sc / (float)chw, mg = sg / (float)chw;
    float qc = 0.f, qg = 0.f;
    for (int e = threadIdx.x; e < chw; e += GUIDE_THREADS) {
        const float dc = out[(long)n * chw + e] - mc;
        const float dg = guided(out, cfg_mode, w, b, n, 1, chw, 0, e) - mg;
        qc += dc * dc;
        qg += dg * dg;
    }
    block_sum2(qc, qg, red);
    float f = 1.f;
    if (chw > 1) {                                  // unbiased, as torch.std
        const float s_pos = sqrtf(qc / (float)(chw - 1)), s_g = sqrtf(qg / (float)(chw - 1));
        if (s_g > 0.f) f = s_pos / s_g;
    }
    const float k = rescale * f + (1.f - rescale);
    for (int e = threadIdx.x; e < chw; e += GUIDE_THREADS)
        g_out[(long)n * chw + e] = k * guided(out, cfg_mode, w, b, n, 1, chw, 0, e);
}

}  // namespace

extern "C" int sgd_cfg_guide(const float* out, int32_t cfg_mode, const float* w_dev, float rescale, int32_t b, int32_t c,
                             int32_t hw, float* guided_out, void* stream) {
    SGD_CLEAR_ERR();
    if (!out || !w_dev || !guided_out || b <= 0 || c <= 0 || hw <= 0 || (cfg_mode != 1 && cfg_mode != 2)) return SGD_ERR_ARG;
    if (!(rescale >= 0.f && rescale <= 1.f)) return SGD_ERR_ARG;                        // (NaN fails both comparisons)
    const long chw = (long)c * hw;
    if (chw > INT32_MAX || 2L * b > INT32_MAX || ((long)b * chw + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    if (rescale == 0.f)
        hipLaunchKernelGGL(cfg_guide_kernel, dim3(nblk((long)b * chw)), dim3(256), 0, (hipStream_t)stream, out, cfg_mode, w_dev,
                           b, chw, guided_out);
    else
        hipLaunchKernelGGL(cfg_guide_rescale_kernel, dim3(b), dim3(GUIDE_THREADS), 0, (hipStream_t)stream, out, cfg_mode, w_dev,
                           rescale, b, (int)chw, guided_out);
    return sgd_check_launch();
}
