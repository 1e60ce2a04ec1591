// Guidance distillation (Meng et al. 2023, "On Distillation of Guided Diffusion Models", stage 1; the reference has no
// counterpart): the loss of a student's single conditional evaluation against the teacher's GUIDED output, and its gradient
// (gfx950; include/sgdm_hip.h: sgd_distill_loss_fwd, sgd_distill_loss_bwd).  Per element
//   target = guided(teach, cfg_mode, *w_dev)     (csrc/sampler_common.h: the form the step kernels and sgd_cfg_guide use)
//   d = out - target;   l = d * d (kind 0) | |d| (kind 1) | |d| < 1 ? 0.5 * d * d : |d| - 0.5 (kind 2, smooth_l1 with beta 1)
// i.e. sgd_loss_fwd / sgd_loss_bwd (csrc/loss.hip) with another target.  The target is formed on the fly in both passes from the
// teacher's RAW output where its engine left it: no target tensor is written, nothing is re-laid.
//
// Layouts: `out` / `gout` are the student's, hw-major (NCHW [b, c, hw]); `teach` is the teacher engine's, c-minor ([2b, hw, c],
// [cond ; uncond], or [b, hw, c] with cfg_mode 0).  As in sgd_v_to_eps (csrc/vpred.hip) a thread owns PIXELS and loops over the
// channels: per channel a wave reads 256 consecutive bytes of `out` (1 KiB on the 16-byte path) and, over the c iterations,
// every byte of 64 * c (256 * c) consecutive floats of each teacher half.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like guide.hip and loss.hip: guided() rounds each
// product before it is added, so the target carries the bits of sgd_cfg_guide (rescale 0) and of a torch-fp32 restatement, and
// the gradient reproduces that restatement bit for bit (tests/test_hip_distill.py).
//
// Both passes are HBM-bound and small (3 * b * c * hw floats).  The forward is one workgroup per sample with one barrier,
// like sgd_loss_fwd, and like it is deliberately not split over several workgroups (a second launch or atomics).
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

constexpr int DISTILL_THREADS = 1024;               // forward: one workgroup per sample, 16 waves
constexpr int DISTILL_WAVES = DISTILL_THREADS / 64;

__device__ __forceinline__ float distill_elem(int kind, float d) {
    if (kind == 0) return d * d;
    const float ad = fabsf(d);
    if (kind == 1) return ad;
    return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

// d l / d d times k (k: the sample's upstream factor; 2 * k is exact) -- csrc/loss.hip: loss_grad
__device__ __forceinline__ float distill_grad(int kind, float d, float k) {
    if (kind == 0) return (2.f * k) * d;
    if (kind == 1) return k * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
    return k * fminf(fmaxf(d, -1.f), 1.f);
}

// VEC: hw % 4 == 0 and `out` 16-byte aligned (then every channel plane starts on a 16-byte boundary): a thread owns four
// consecutive pixels and reads them from a plane in one 16-byte access.  Otherwise one pixel per thread.  The teacher is read
// float by float either way (a thread's 4 * c floats are consecutive; the c iterations use every byte of the lines they touch).
// Per-thread partial sums in double (the fp32 value l of an element is exact in it), xor-shuffles inside each wave, one LDS slot
// per wave, folded in ascending order by thread 0: no atomics, the result depends on the inputs alone.
template <bool VEC>
__global__ __launch_bounds__(DISTILL_THREADS) void distill_fwd_kernel(const float* __restrict__ out, const float* __restrict__ teach,
                                                                      int cfg_mode, const float* __restrict__ w_dev,
                                                                      const int64_t* __restrict__ t, const float* __restrict__ wt,
                                                                      int kind, int b, int c, int hw,
                                                                      float* __restrict__ per_raw, float* __restrict__ per_w) {
    __shared__ double red[DISTILL_WAVES];
    const int n = blockIdx.x;
    const float w = cfg_mode ? *w_dev : 0.f;
    const float* __restrict__ o_n = out + (long)n * c * hw;
    double acc = 0.0;
    if (VEC) {
        for (int q = threadIdx.x; q < hw / 4; q += DISTILL_THREADS) {
            const int p = 4 * q;
            for (int cc = 0; cc < c; ++cc) {
                const f32x4 o = *reinterpret_cast<const f32x4*>(o_n + (long)cc * hw + p);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc += (double)distill_elem(kind, o[j] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j));
            }
        }
    } else {
        for (int p = threadIdx.x; p < hw; p += DISTILL_THREADS)
            for (int cc = 0; cc < c; ++cc)
                acc += (double)distill_elem(kind, o_n[(long)cc * hw + p] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p));
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < DISTILL_WAVES; ++i) s += red[i];
        const float raw = (float)(s / ((double)c * (double)hw));
        per_raw[n] = raw;
        per_w[n] = wt ? wt[t[n]] * raw : raw;
    }
}

// element-wise over [b, c, hw]: `bps` blocks of 256 threads per sample, a thread per pixel quad (VEC) or per pixel, all of its
// channels; the sample index is one scalar division per block and t / wt / gper / w are scalar loads.  Nothing passed by
// value changes from step to step: the upstream gradient and the guidance weight are read from device memory.
template <bool VEC>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const float* __restrict__ out, const float* __restrict__ teach,
                                                          int cfg_mode, const float* __restrict__ w_dev,
                                                          const int64_t* __restrict__ t, const float* __restrict__ wt,
                                                          const float* __restrict__ gper, float gscale, int kind, int b, int c,
                                                          int hw, unsigned bps, float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * 256 + threadIdx.x;            // pixel quad (VEC) or pixel of the sample
    if (u >= (VEC ? hw / 4 : hw)) return;
    const float w = cfg_mode ? *w_dev : 0.f;
    float k = (gper[n] * (wt ? wt[t[n]] : 1.f)) / (float)((long)c * hw);
    k = k * gscale;
    const long base = (long)n * c * hw;
    if (VEC) {
        const int p = 4 * (int)u;
        for (int cc = 0; cc < c; ++cc) {
            const long i = base + (long)cc * hw + p;
            const f32x4 o = *reinterpret_cast<const f32x4*>(out + i);
            f32x4 g;
#pragma unroll
            for (int j = 0; j < 4; ++j) g[j] = distill_grad(kind, o[j] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j), k);
            *reinterpret_cast<f32x4*>(gout + i) = g;
        }
    } else {
        const int p = (int)u;
        for (int cc = 0; cc < c; ++cc) {
            const long i = base + (long)cc * hw + p;
            gout[i] = distill_grad(kind, out[i] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p), k);
        }
    }
}

bool distill_args_ok(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t, int32_t kind,
                     int32_t b, int32_t c, int32_t hw) {
    if (!out || !teach || !t || b <= 0 || c <= 0 || hw <= 0 || cfg_mode < 0 || cfg_mode > 2 || kind < 0 || kind > 2) return false;
    if (cfg_mode != 0 && !w_dev) return false;
    return (long)c * hw <= INT32_MAX && 2L * b <= INT32_MAX;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int sgd_distill_loss_fwd(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t,
                                    const float* wt, int32_t kind, int32_t b, int32_t c, int32_t hw, float* per_raw, float* per_w,
                                    void* stream) {
    SGD_CLEAR_ERR();
    if (!distill_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !per_raw || !per_w) return SGD_ERR_ARG;
    if (hw % 4 == 0 && aligned16(out))
        hipLaunchKernelGGL(distill_fwd_kernel<true>, dim3(b), dim3(DISTILL_THREADS), 0, (hipStream_t)stream, out, teach, cfg_mode,
                           w_dev, t, wt, kind, b, c, hw, per_raw, per_w);
    else
        hipLaunchKernelGGL(distill_fwd_kernel<false>, dim3(b), dim3(DISTILL_THREADS), 0, (hipStream_t)stream, out, teach, cfg_mode,
                           w_dev, t, wt, kind, b, c, hw, per_raw, per_w);
    return sgd_check_launch();
}

extern "C" int sgd_distill_loss_bwd(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t,
                                    const float* wt, int32_t kind, int32_t b, int32_t c, int32_t hw, const float* gper,
                                    float gscale, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!distill_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !gper || !gout) return SGD_ERR_ARG;
    const bool vec = hw % 4 == 0 && aligned16(out) && aligned16(gout);
    const int64_t units = vec ? hw / 4 : hw;
    const int64_t bps = (units + 255) / 256;
    if (bps > INT32_MAX / b) return SGD_ERR_ARG;
    const dim3 grid((unsigned)(bps * b));
    if (vec)
        hipLaunchKernelGGL(distill_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, teach, cfg_mode, w_dev, t, wt,
                           gper, gscale, kind, b, c, hw, (unsigned)bps, gout);
    else
        hipLaunchKernelGGL(distill_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, teach, cfg_mode, w_dev, t, wt,
                           gper, gscale, kind, b, c, hw, (unsigned)bps, gout);
    return sgd_check_launch();
}
