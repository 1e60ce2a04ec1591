// Helpers shared by the sampler kernels: misc.hip (DDPM / DDIM steps, cfg combine, x0 quantile), pndm.hip, dpm.hip, vpred.hip.
//
// Everything here is __device__ __forceinline__ (or host inline) and is therefore compiled under the flags of the file that
// includes it: pndm.hip, dpm.hip and vpred.hip (build.py: FILE_FLAGS, -ffp-contract=off) get guided() with each product
// rounded before it is added, as torch does; misc.hip (global -ffp-contract=fast) gets it contracted, which is what the
// DDPM / DDIM trajectories were validated with.  That difference is why each of those files used to carry its own copy.
#pragma once
#include "sgdm_common.h"

// guided network output (include/sgdm_hip.h, "Sampler step kernels"): `out` is [2b, hw, c] ([cond ; uncond]) when
// cfg_mode != 0, else [b, hw, c]
__device__ __forceinline__ float guided(const float* __restrict__ out, int cfg_mode, float w, int b, int n, int c, int hw,
                                        int cc, int p) {
    const float oc = out[((long)n * hw + p) * c + cc];
    if (cfg_mode == 0) return oc;
    const float ou = out[((long)(n + b) * hw + p) * c + cc];
    if (cfg_mode == 1) return (1.f - w) * ou + w * oc;        // imagen  (openaimodel.py:855)
    return (1.f + w) * oc - w * ou;                           // cfg     (openaimodel.py:857)
}

// flat index i of an NCHW [b, c, hw] tensor -> sample n, channel cc, pixel p
struct sgd_ncp { int n, cc, p; };
__device__ __forceinline__ sgd_ncp nchw_split(long i, int c, int hw) {
    const int p = i % hw;
    const long t = i / hw;
    return {(int)(t / c), (int)(t % c), p};
}

// blocks of 256 threads, one thread per element
inline unsigned nblk(long total) { return (unsigned)((total + 255) / 256); }
