// Weighted diffusion loss and its gradient (gfx950; include/sgdm_hip.h: sgd_loss_fwd, sgd_loss_bwd; the reference weighs every
// timestep alike and leaves the loss to torch ops, diffusion/ddpm.py:67-103).  Per element
//   target = noise (par 0) | x0 (par 1) | sa[t] * noise - s1[t] * x0 (par 2: the bits of sgd_q_sample_v's v_out)
//   d = out - target;   l = d * d (kind 0) | |d| (kind 1) | |d| < 1 ? 0.5 * d * d : |d| - 0.5 (kind 2, smooth_l1 with beta 1)
// The target is formed on the fly in both passes: no target tensor is written.  All tensors are NCHW, [b, chw] flat.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like vpred.hip: every product is rounded before it is
// added, so the gradient reproduces a torch-fp32 restatement bit for bit (tests/test_hip_loss_weighting.py).
//
// sgd_loss_fwd is latency-bound: one workgroup per sample walks 3 * chw floats (144 KiB per sample at the flagship size, a few
// waves of 16-byte loads per thread) and ends in one barrier; at a training batch it occupies b of the 256 CUs for a few
// microseconds.  It is deliberately not tuned further (no split of a sample over several workgroups, which would need a second
// launch or atomics).  sgd_loss_bwd is a plain HBM-bound element-wise pass.
#include "loss_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// W == 4: chw % 4 == 0 and every tensor 16-byte aligned (then every sample starts on a 16-byte boundary): consecutive lanes
// read consecutive 16-byte quads.  W == 1: one float per lane.  Either way a thread walks its elements in ascending order and
// the workgroup sums as loss_block_sum (csrc/loss_common.h) says.
template <int W>
__global__ __launch_bounds__(LOSS_FWD_THREADS) void loss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                                    const float* __restrict__ noise,
                                                                    const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                                    const float* __restrict__ s1, const float* __restrict__ wt,
                                                                    int par, int kind, long chw, float* __restrict__ per_raw,
                                                                    float* __restrict__ per_w) {
    __shared__ double red[LOSS_FWD_THREADS / 64];
    const int n = blockIdx.x;
    const int64_t tt = t[n];
    float a = 0.f, s = 0.f;                         // sa[t], s1[t] of the sample (par 2 only)
    if (par == 2) { a = sa[tt]; s = s1[tt]; }
    const bool need_x = par != 0, need_n = par != 1;
    const long base = (long)n * chw;
    double acc = 0.0;
    for (long u = threadIdx.x; u < chw / W; u += LOSS_FWD_THREADS) {
        const long i = base + W * u;
        const loss_vec<W> o = loss_load<W>(out, i), xv = loss_load<W>(x0, i, need_x), nv = loss_load<W>(noise, i, need_n);
#pragma unroll
        for (int j = 0; j < W; ++j) acc += (double)loss_elem(kind, o[j] - loss_target(par, xv[j], nv[j], a, s));
    }
    const double sum = loss_block_sum<LOSS_FWD_THREADS>(acc, red);
    if (threadIdx.x == 0) {
        const float raw = (float)(sum / (double)chw);
        per_raw[n] = raw;
        per_w[n] = wt ? wt[tt] * raw : raw;
    }
}

// element-wise over [b, chw]: `bps` blocks per sample, a thread per quad (W == 4) or per float, so the sample index is one
// scalar division per block and t / wt / gper are scalar loads.  Nothing passed by value changes from step to step: the
// upstream gradient is read from device memory.
template <int W>
__global__ __launch_bounds__(LOSS_BWD_THREADS) void loss_bwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                                    const float* __restrict__ noise,
                                                                    const int64_t* __restrict__ t, const float* __restrict__ sa,
                                                                    const float* __restrict__ s1, const float* __restrict__ wt,
                                                                    const float* __restrict__ gper, float gscale, int par,
                                                                    int kind, long chw, unsigned bps, float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * LOSS_BWD_THREADS + threadIdx.x;
    if (u >= chw / W) return;
    const int64_t tt = t[n];
    float a = 0.f, s = 0.f;
    if (par == 2) { a = sa[tt]; s = s1[tt]; }
    float k = (gper[n] * (wt ? wt[tt] : 1.f)) / (float)chw;
    k = k * gscale;
    const long i = (long)n * chw + W * u;
    const loss_vec<W> o = loss_load<W>(out, i), xv = loss_load<W>(x0, i, par != 0), nv = loss_load<W>(noise, i, par != 1);
    loss_vec<W> g;
#pragma unroll
    for (int j = 0; j < W; ++j) g[j] = loss_grad(kind, o[j] - loss_target(par, xv[j], nv[j], a, s), k);
    loss_store<W>(gout, i, g);
}

bool loss_args_ok(const float* out, const float* x0, const float* noise, const int64_t* t, const float* sa, const float* s1,
                  int32_t par, int32_t kind, int32_t b, int64_t chw) {
    if (!out || !t || b <= 0 || chw <= 0 || par < 0 || par > 2 || kind < 0 || kind > 2) return false;
    if (par != 1 && !noise) return false;
    if (par != 0 && !x0) return false;
    if (par == 2 && (!sa || !s1)) return false;
    return chw <= INT64_MAX / b;
}

// the 16-byte path: a whole number of quads per sample and every tensor that is read or written on a 16-byte boundary
bool loss_vec_ok(const float* out, const float* x0, const float* noise, int32_t par, int64_t chw, const float* gout) {
    return chw % 4 == 0 && aligned16(out) && aligned16(gout) && (par == 0 || aligned16(x0)) && (par == 1 || aligned16(noise));
}

}  // namespace

extern "C" int sgd_loss_fwd(const float* out, const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                            const float* sqrt_1mac, const float* wt, int32_t par, int32_t kind, int32_t b, int64_t chw,
                            float* per_raw, float* per_w, void* stream) {
    SGD_CLEAR_ERR();
    if (!loss_args_ok(out, x0, noise, t, sqrt_ac, sqrt_1mac, par, kind, b, chw) || !per_raw || !per_w) return SGD_ERR_ARG;
    return loss_launch(loss_vec_ok(out, x0, noise, par, chw, nullptr), loss_fwd_kernel<4>, loss_fwd_kernel<1>, (unsigned)b,
                       LOSS_FWD_THREADS, stream, out, x0, noise, t, sqrt_ac, sqrt_1mac, wt, par, kind, (long)chw, per_raw, per_w);
}

extern "C" int sgd_loss_bwd(const float* out, const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                            const float* sqrt_1mac, const float* wt, const float* gper, float gscale, int32_t par, int32_t kind,
                            int32_t b, int64_t chw, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!loss_args_ok(out, x0, noise, t, sqrt_ac, sqrt_1mac, par, kind, b, chw) || !gper || !gout) return SGD_ERR_ARG;
    const bool vec = loss_vec_ok(out, x0, noise, par, chw, gout);
    const unsigned bps = loss_bps(vec, chw, b);
    if (!bps) return SGD_ERR_ARG;
    return loss_launch(vec, loss_bwd_kernel<4>, loss_bwd_kernel<1>, bps * b, LOSS_BWD_THREADS, stream, out, x0, noise, t, sqrt_ac,
                       sqrt_1mac, wt, gper, gscale, par, kind, (long)chw, bps, gout);
}
