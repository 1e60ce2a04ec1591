// The device core shared by the fused loss pairs: loss.hip (sgd_loss_fwd / sgd_loss_bwd), lvloss.hip (sgd_lv_loss_fwd /
// sgd_lv_loss_bwd), distill.hip (sgd_distill_loss_fwd / sgd_distill_loss_bwd) and progressive.hip (sgd_pd_loss_fwd /
// sgd_pd_loss_bwd).  They differ in the target they form and in what else they compute per element; what an element of the
// simple term costs, its gradient, the order in which a sample's elements are summed and the launch arithmetic are the same, and
// live here once: the simple terms of the pairs agree bit for bit because they ARE the same code, which the tests assert
// (tests/test_hip_learned_variance.py, tests/test_hip_distill.py, tests/test_hip_progressive.py).
//
// (gradclip.hip, the gradient norm of the optimizer's clip, takes loss_block_sum from here and nothing else.)
//
// Everything here is __device__ __forceinline__ (or host inline) and is therefore compiled under the flags of the file that
// includes it.  All includers are -ffp-contract=off (build.py: FILE_FLAGS): every product is rounded before it is added,
// so the gradient reproduces a torch-fp32 restatement bit for bit.  A file compiled with contraction on must not include this.
#pragma once
#include "sgdm_common.h"

constexpr int LOSS_FWD_THREADS = 1024;              // forward: one workgroup per sample, 16 waves
constexpr int LOSS_BWD_THREADS = 256;               // backward: `bps` blocks per sample

// target = noise (par 0) | x0 (par 1) | sa[t] * noise - s1[t] * x0 (par 2: the bits of sgd_q_sample_v's v_out)
__device__ __forceinline__ float loss_target(int par, float xi, float ni, float sa, float s1) {
    if (par == 0) return ni;
    if (par == 1) return xi;
    return sa * ni - s1 * xi;                       // two rounded products, as q_sample_v_kernel (csrc/vpred.hip)
}

// l = d * d (kind 0) | |d| (kind 1) | |d| < 1 ? 0.5 * d * d : |d| - 0.5 (kind 2, smooth_l1 with beta 1)
__device__ __forceinline__ float loss_elem(int kind, float d) {
    if (kind == 0) return d * d;
    const float ad = fabsf(d);
    if (kind == 1) return ad;
    return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

// d l / d d times k (k: the sample's upstream factor; 2 * k is exact)
__device__ __forceinline__ float loss_grad(int kind, float d, float k) {
    if (kind == 0) return (2.f * k) * d;
    if (kind == 1) return k * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
    return k * fminf(fmaxf(d, -1.f), 1.f);
}

// The sum of a workgroup's per-thread partials, valid in thread 0: xor-shuffles inside each wave, one LDS slot per wave
// (`red`: THREADS / 64 doubles), folded in ascending order by thread 0.  No atomics: the result depends on the inputs alone.
// The partials are double: the fp32 value of an element is exact in it.
template <int THREADS>
__device__ __forceinline__ double loss_block_sum(double acc, double* red) {
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < THREADS / 64; ++i) s += red[i];
    return s;
}

// W consecutive floats in one access: W == 4 is one 16-byte load / store (p + i on a 16-byte boundary), W == 1 one float.
// Every kernel is templated on W and walks its elements in the same per-thread order at either width.
template <int W>
using loss_vec = float __attribute__((ext_vector_type(W)));

// (`need` false: a tensor the target does not read; the pointer may be NULL and nothing is read)
template <int W>
__device__ __forceinline__ loss_vec<W> loss_load(const float* __restrict__ p, long i, bool need = true) {
    return need ? *reinterpret_cast<const loss_vec<W>*>(p + i) : loss_vec<W>(0.f);
}

template <int W>
__device__ __forceinline__ void loss_store(float* __restrict__ p, long i, loss_vec<W> v) {
    *reinterpret_cast<loss_vec<W>*>(p + i) = v;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The argument rules of the pairs whose target is a GUIDED teacher output (distill.hip, progressive.hip): `out` NCHW [b, c, hw],
// `teach` NHWC [2b | b, hw, c] read through guided() (csrc/sampler_common.h), the weight from device memory.
inline bool guided_loss_args_ok(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t,
                                int32_t kind, int32_t b, int32_t c, int32_t hw) {
    if (!out || !teach || !t || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 || cfg_mode > 2 || kind < 0 || kind > 2) return false;
    if (cfg_mode != 0 && !w_dev) return false;
    return (long)c * hw <= INT32_MAX && 2L * b <= INT32_MAX;
}

// their 16-byte path: a whole number of pixel quads per plane, every NCHW tensor on a 16-byte boundary (NULL: not part of the
// call; the teacher is read float by float and may sit anywhere)
inline bool guided_loss_vec_ok(int32_t hw, const float* p0, const float* p1 = nullptr, const float* p2 = nullptr) {
    return hw % 4 == 0 && aligned16(p0) && aligned16(p1) && aligned16(p2);
}

// the element-wise passes: blocks of LOSS_BWD_THREADS per sample for `per_sample` floats, a thread per quad (vec) or per float;
// 0 when b samples of that many blocks do not fit a grid
inline unsigned loss_bps(bool vec, int64_t per_sample, int32_t b) {
    const int64_t units = vec ? per_sample / 4 : per_sample;
    const int64_t bps = (units + LOSS_BWD_THREADS - 1) / LOSS_BWD_THREADS;
    return bps > INT32_MAX / b ? 0u : (unsigned)bps;
}

// launch the <4> (vec) or the <1> instance of a kernel on the same arguments
template <typename... KA, typename... A>
inline int loss_launch(bool vec, void (*k4)(KA...), void (*k1)(KA...), unsigned grid, int threads, void* stream, A... args) {
    hipLaunchKernelGGL(vec ? k4 : k1, dim3(grid), dim3(threads), 0, (hipStream_t)stream, args...);
    return sgd_check_launch();
}
