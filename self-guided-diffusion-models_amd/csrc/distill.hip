// Guidance distillation (Meng et al. 2023, "On Distillation of Guided Diffusion Models", stage 1; the reference has no
// counterpart): the loss of a student's single conditional evaluation against the teacher's GUIDED output, and its gradient
// (gfx950; include/sgdm_hip.h: sgd_distill_loss_fwd, sgd_distill_loss_bwd).  Per element
//   target = guided(teach, cfg_mode, *w_dev)     (csrc/sampler_common.h: the form the step kernels and sgd_cfg_guide use)
//   d = out - target;   l = d * d (kind 0) | |d| (kind 1) | |d| < 1 ? 0.5 * d * d : |d| - 0.5 (kind 2, smooth_l1 with beta 1)
// i.e. sgd_loss_fwd / sgd_loss_bwd (csrc/loss.hip) with another target: loss_elem / loss_grad are csrc/loss_common.h's.  The
// target is formed on the fly in both passes from the teacher's RAW output where its engine left it: no target tensor is
// written, nothing is re-laid.
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
#include "loss_common.h"
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// W == 4: hw % 4 == 0 and `out` 16-byte aligned (then every channel plane starts on a 16-byte boundary): a thread owns four
// consecutive pixels and reads them from a plane in one 16-byte access.  W == 1: one pixel per thread.  The teacher is read
// float by float either way (a thread's W * c floats are consecutive; the c iterations use every byte of the lines they touch).
// Summed as loss_block_sum (csrc/loss_common.h).
template <int W>
__global__ __launch_bounds__(LOSS_FWD_THREADS) void distill_fwd_kernel(const float* __restrict__ out, const float* __restrict__ teach,
                                                                       int cfg_mode, const float* __restrict__ w_dev,
                                                                       const int64_t* __restrict__ t, const float* __restrict__ wt,
                                                                       int kind, int b, int c, int hw,
                                                                       float* __restrict__ per_raw, float* __restrict__ per_w) {
    __shared__ double red[LOSS_FWD_THREADS / 64];
    const int n = blockIdx.x;
    const float w = cfg_mode ? *w_dev : 0.f;
    const float* __restrict__ o_n = out + (long)n * c * hw;
    double acc = 0.0;
    for (int u = threadIdx.x; u < hw / W; u += LOSS_FWD_THREADS) {
        const int p = W * u;
        for (int cc = 0; cc < c; ++cc) {
            const loss_vec<W> o = loss_load<W>(o_n, (long)cc * hw + p);
#pragma unroll
            for (int j = 0; j < W; ++j) acc += (double)loss_elem(kind, o[j] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j));
        }
    }
    const double s = loss_block_sum<LOSS_FWD_THREADS>(acc, red);
    if (threadIdx.x == 0) {
        const float raw = (float)(s / ((double)c * (double)hw));
        per_raw[n] = raw;
        per_w[n] = wt ? wt[t[n]] * raw : raw;
    }
}

// element-wise over [b, c, hw]: `bps` blocks per sample, a thread per pixel quad (W == 4) or per pixel, all of its channels; the
// sample index is one scalar division per block and t / wt / gper / w are scalar loads.  Nothing passed by value changes from
// step to step: the upstream gradient and the guidance weight are read from device memory.
template <int W>
__global__ __launch_bounds__(LOSS_BWD_THREADS) void distill_bwd_kernel(const float* __restrict__ out, const float* __restrict__ teach,
                                                                       int cfg_mode, const float* __restrict__ w_dev,
                                                                       const int64_t* __restrict__ t, const float* __restrict__ wt,
                                                                       const float* __restrict__ gper, float gscale, int kind,
                                                                       int b, int c, int hw, unsigned bps,
                                                                       float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * LOSS_BWD_THREADS + threadIdx.x;
    if (u >= hw / W) return;
    const float w = cfg_mode ? *w_dev : 0.f;
    float k = (gper[n] * (wt ? wt[t[n]] : 1.f)) / (float)((long)c * hw);
    k = k * gscale;
    const int p = W * (int)u;
    for (int cc = 0; cc < c; ++cc) {
        const long i = ((long)n * c + cc) * hw + p;
        const loss_vec<W> o = loss_load<W>(out, i);
        loss_vec<W> g;
#pragma unroll
        for (int j = 0; j < W; ++j) g[j] = loss_grad(kind, o[j] - guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j), k);
        loss_store<W>(gout, i, g);
    }
}

// (the argument rules and the 16-byte path's are csrc/loss_common.h's, shared with progressive.hip: guided_loss_args_ok,
// guided_loss_vec_ok)

}  // namespace

extern "C" int sgd_distill_loss_fwd(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t,
                                    const float* wt, int32_t kind, int32_t b, int32_t c, int32_t hw, float* per_raw, float* per_w,
                                    void* stream) {
    SGD_CLEAR_ERR();
    if (!guided_loss_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !per_raw || !per_w) return SGD_ERR_ARG;
    return loss_launch(guided_loss_vec_ok(hw, out), distill_fwd_kernel<4>, distill_fwd_kernel<1>, (unsigned)b,
                       LOSS_FWD_THREADS, stream, out, teach, cfg_mode, w_dev, t, wt, kind, b, c, hw, per_raw, per_w);
}

extern "C" int sgd_distill_loss_bwd(const float* out, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* t,
                                    const float* wt, int32_t kind, int32_t b, int32_t c, int32_t hw, const float* gper,
                                    float gscale, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!guided_loss_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !gper || !gout) return SGD_ERR_ARG;
    const bool vec = guided_loss_vec_ok(hw, out, gout);
    const unsigned bps = loss_bps(vec, hw, b);
    if (!bps) return SGD_ERR_ARG;
    return loss_launch(vec, distill_bwd_kernel<4>, distill_bwd_kernel<1>, bps * b, LOSS_BWD_THREADS, stream, out, teach, cfg_mode,
                       w_dev, t, wt, gper, gscale, kind, b, c, hw, bps, gout);
}
