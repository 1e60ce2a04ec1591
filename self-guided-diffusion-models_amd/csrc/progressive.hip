// Progressive distillation (Salimans & Ho 2022, Algorithm 2; stage 2 of Meng et al. 2023; the reference has no counterpart): a
// student whose ONE deterministic DDIM step t -> e lands where TWO steps t -> m -> e of a frozen teacher land (gfx950;
// include/sgdm_hip.h: sgd_pd_half_step, sgd_pd_loss_fwd, sgd_pd_loss_bwd).  A DDIM step is linear in the network output for every
// parameterization, so with y1 = guided(teacher(z_t, t)) and y2 = guided(teacher(z_m, m)) the student's target is
//   y* = d0 z_t + d1 y1 + d2 y2,      z_m = a1 z_t + b1 y1
// with five per-grid-point scalars (sgd_pd_row; sgdm_amd/diffusion.py: progressive_rows, float64 on the host, rounded once; every
// |d| <= 1, so nothing cancels).  Three passes:
//   sgd_pd_half_step   z_mid = a1 x + b1 y1 and head = d0 x + d1 y1, from one read of x and of the teacher's first output
//   sgd_pd_loss_fwd    sgd_distill_loss_fwd with target = head + d2 y2, y2 read where the second evaluation's engine left it
//   sgd_pd_loss_bwd    sgd_distill_loss_bwd with that target
// The target is never written.  loss_elem / loss_grad / loss_block_sum / loss_load / loss_launch and the argument rules are
// csrc/loss_common.h's, guided() is csrc/sampler_common.h's: the loss of an element, its gradient and the order of the sums are
// those of distill.hip because they are the same code.
//
// Layouts as in distill.hip: x / z_mid / head / out / gout are hw-major (NCHW [b, c, hw]), `teach` is the teacher engine's,
// c-minor ([2b, hw, c], [cond ; uncond], or [b, hw, c] with cfg_mode 0).  A thread owns a pixel quad (hw % 4 == 0 and every NCHW
// tensor 16-byte aligned) or a pixel and loops over the channels: per channel a wave touches whole lines of each plane and, over
// the c iterations, every byte of the teacher lines it reads.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), as csrc/loss_common.h demands: every product is rounded
// before it is added, so z_mid, head and the gradient carry the bits of a torch-fp32 restatement (tests/test_hip_progressive.py).
//
// All three passes are HBM-bound and small (at most 4 * b * c * hw floats).
#include "loss_common.h"
#include "sampler_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// element-wise over [b, c, hw]: `bps` blocks per sample; the row is one scalar load per block
template <int W>
__global__ __launch_bounds__(LOSS_BWD_THREADS) void pd_half_step_kernel(const float* __restrict__ x, const float* __restrict__ teach,
                                                                        int cfg_mode, const float* __restrict__ w_dev,
                                                                        const int64_t* __restrict__ idx,
                                                                        const sgd_pd_row* __restrict__ rows, int b, int c, int hw,
                                                                        unsigned bps, float* __restrict__ z_mid,
                                                                        float* __restrict__ head) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * LOSS_BWD_THREADS + threadIdx.x;
    if (u >= hw / W) return;
    const float w = cfg_mode ? *w_dev : 0.f;
    const sgd_pd_row r = rows[idx[n]];
    const int p = W * (int)u;
    for (int cc = 0; cc < c; ++cc) {
        const long i = ((long)n * c + cc) * hw + p;
        const loss_vec<W> xv = loss_load<W>(x, i);
        loss_vec<W> zm, hd;
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const float g = guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j);
            zm[j] = r.a1 * xv[j] + r.b1 * g;
            hd[j] = r.d0 * xv[j] + r.d1 * g;
        }
        loss_store<W>(z_mid, i, zm);
        loss_store<W>(head, i, hd);
    }
}

// distill_fwd_kernel (csrc/distill.hip) with target = head + d2 * guided(teach): one workgroup per sample, summed as
// loss_block_sum
template <int W>
__global__ __launch_bounds__(LOSS_FWD_THREADS) void pd_fwd_kernel(const float* __restrict__ out, const float* __restrict__ head,
                                                                  const float* __restrict__ teach, int cfg_mode,
                                                                  const float* __restrict__ w_dev, const int64_t* __restrict__ idx,
                                                                  const sgd_pd_row* __restrict__ rows, const int64_t* __restrict__ t,
                                                                  const float* __restrict__ wt, int kind, int b, int c, int hw,
                                                                  float* __restrict__ per_raw, float* __restrict__ per_w) {
    __shared__ double red[LOSS_FWD_THREADS / 64];
    const int n = blockIdx.x;
    const float w = cfg_mode ? *w_dev : 0.f;
    const float d2 = rows[idx[n]].d2;
    const float* __restrict__ o_n = out + (long)n * c * hw;
    const float* __restrict__ h_n = head + (long)n * c * hw;
    double acc = 0.0;
    for (int u = threadIdx.x; u < hw / W; u += LOSS_FWD_THREADS) {
        const int p = W * u;
        for (int cc = 0; cc < c; ++cc) {
            const loss_vec<W> o = loss_load<W>(o_n, (long)cc * hw + p);
            const loss_vec<W> h = loss_load<W>(h_n, (long)cc * hw + p);
#pragma unroll
            for (int j = 0; j < W; ++j)
                acc += (double)loss_elem(kind, o[j] - (h[j] + d2 * guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j)));
        }
    }
    const double s = loss_block_sum<LOSS_FWD_THREADS>(acc, red);
    if (threadIdx.x == 0) {
        const float raw = (float)(s / ((double)c * (double)hw));
        per_raw[n] = raw;
        per_w[n] = wt ? wt[t[n]] * raw : raw;
    }
}

// distill_bwd_kernel (csrc/distill.hip) with that target.  Nothing passed by value changes from step to step.
template <int W>
__global__ __launch_bounds__(LOSS_BWD_THREADS) void pd_bwd_kernel(const float* __restrict__ out, const float* __restrict__ head,
                                                                  const float* __restrict__ teach, int cfg_mode,
                                                                  const float* __restrict__ w_dev, const int64_t* __restrict__ idx,
                                                                  const sgd_pd_row* __restrict__ rows, const int64_t* __restrict__ t,
                                                                  const float* __restrict__ wt, const float* __restrict__ gper,
                                                                  float gscale, int kind, int b, int c, int hw, unsigned bps,
                                                                  float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * LOSS_BWD_THREADS + threadIdx.x;
    if (u >= hw / W) return;
    const float w = cfg_mode ? *w_dev : 0.f;
    const float d2 = rows[idx[n]].d2;
    float k = (gper[n] * (wt ? wt[t[n]] : 1.f)) / (float)((long)c * hw);
    k = k * gscale;
    const int p = W * (int)u;
    for (int cc = 0; cc < c; ++cc) {
        const long i = ((long)n * c + cc) * hw + p;
        const loss_vec<W> o = loss_load<W>(out, i);
        const loss_vec<W> h = loss_load<W>(head, i);
        loss_vec<W> g;
#pragma unroll
        for (int j = 0; j < W; ++j)
            g[j] = loss_grad(kind, o[j] - (h[j] + d2 * guided(teach, cfg_mode, w, b, n, c, hw, cc, p + j)), k);
        loss_store<W>(gout, i, g);
    }
}

}  // namespace

extern "C" int sgd_pd_half_step(const float* x, const float* teach, int32_t cfg_mode, const float* w_dev, const int64_t* idx,
                                const sgd_pd_row* rows, int32_t b, int32_t c, int32_t hw, float* z_mid, float* head,
                                void* stream) {
    SGD_CLEAR_ERR();
    // (guided_loss_args_ok's `t` is any per-sample int64 the kernel gathers with: here the grid index; kind is not read)
    if (!guided_loss_args_ok(x, teach, cfg_mode, w_dev, idx, 0, b, c, hw) || !rows || !z_mid || !head) return SGD_ERR_ARG;
    const bool vec = guided_loss_vec_ok(hw, x, z_mid, head);
    const unsigned bps = loss_bps(vec, hw, b);
    if (!bps) return SGD_ERR_ARG;
    return loss_launch(vec, pd_half_step_kernel<4>, pd_half_step_kernel<1>, bps * b, LOSS_BWD_THREADS, stream, x, teach, cfg_mode,
                       w_dev, idx, rows, b, c, hw, bps, z_mid, head);
}

extern "C" int sgd_pd_loss_fwd(const float* out, const float* head, const float* teach, int32_t cfg_mode, const float* w_dev,
                               const int64_t* idx, const sgd_pd_row* rows, const int64_t* t, const float* wt, int32_t kind,
                               int32_t b, int32_t c, int32_t hw, float* per_raw, float* per_w, void* stream) {
    SGD_CLEAR_ERR();
    if (!guided_loss_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !head || !idx || !rows || !per_raw || !per_w)
        return SGD_ERR_ARG;
    return loss_launch(guided_loss_vec_ok(hw, out, head), pd_fwd_kernel<4>, pd_fwd_kernel<1>, (unsigned)b, LOSS_FWD_THREADS, stream,
                       out, head, teach, cfg_mode, w_dev, idx, rows, t, wt, kind, b, c, hw, per_raw, per_w);
}

extern "C" int sgd_pd_loss_bwd(const float* out, const float* head, const float* teach, int32_t cfg_mode, const float* w_dev,
                               const int64_t* idx, const sgd_pd_row* rows, const int64_t* t, const float* wt, int32_t kind,
                               int32_t b, int32_t c, int32_t hw, const float* gper, float gscale, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!guided_loss_args_ok(out, teach, cfg_mode, w_dev, t, kind, b, c, hw) || !head || !idx || !rows || !gper || !gout)
        return SGD_ERR_ARG;
    const bool vec = guided_loss_vec_ok(hw, out, head, gout);
    const unsigned bps = loss_bps(vec, hw, b);
    if (!bps) return SGD_ERR_ARG;
    return loss_launch(vec, pd_bwd_kernel<4>, pd_bwd_kernel<1>, bps * b, LOSS_BWD_THREADS, stream, out, head, teach, cfg_mode, w_dev,
                       idx, rows, t, wt, gper, gscale, kind, b, c, hw, bps, gout);
}
