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
#include "sgdm_common.h"
#include "../../include/sgdm_hip.h"

namespace {

constexpr int LOSS_THREADS = 1024;                  // forward: one workgroup per sample, 16 waves
constexpr int LOSS_WAVES = LOSS_THREADS / 64;

struct loss_coef { float a, s; };                   // sa[t], s1[t] of the sample (par 2 only)

__device__ __forceinline__ float loss_target(int par, float xi, float ni, loss_coef c) {
    if (par == 0) return ni;
    if (par == 1) return xi;
    return c.a * ni - c.s * xi;                     // two rounded products, as q_sample_v_kernel (csrc/vpred.hip)
}

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

// four consecutive floats of a tensor that the target may not need (then the pointer may be NULL and nothing is read)
__device__ __forceinline__ f32x4 load4(const float* __restrict__ p, long i, bool need) {
    return need ? *reinterpret_cast<const f32x4*>(p + i) : f32x4{0.f, 0.f, 0.f, 0.f};
}

// VEC: chw % 4 == 0 and every tensor 16-byte aligned (then every sample starts on a 16-byte boundary): consecutive lanes
// read consecutive 16-byte quads.  Otherwise one float per lane.  Per-thread partial sums in double (the fp32 value l of an
// element is exact in it), xor-shuffles inside each wave, one LDS slot per wave, folded in ascending order by thread 0: no
// atomics, the result depends on the inputs alone.
template <bool VEC>
__global__ __launch_bounds__(LOSS_THREADS) void loss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                                const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                                const float* __restrict__ sa, const float* __restrict__ s1,
                                                                const float* __restrict__ wt, int par, int kind, long chw,
                                                                float* __restrict__ per_raw, float* __restrict__ per_w) {
    __shared__ double red[LOSS_WAVES];
    const int n = blockIdx.x;
    const int64_t tt = t[n];
    loss_coef c = {0.f, 0.f};
    if (par == 2) c = {sa[tt], s1[tt]};
    const bool need_x = par != 0, need_n = par != 1;
    const long base = (long)n * chw;
    double acc = 0.0;
    if (VEC) {
        for (long q = threadIdx.x; q < chw / 4; q += LOSS_THREADS) {
            const long i = base + 4 * q;
            const f32x4 o = *reinterpret_cast<const f32x4*>(out + i);
            const f32x4 xv = load4(x0, i, need_x), nv = load4(noise, i, need_n);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc += (double)loss_elem(kind, o[j] - loss_target(par, xv[j], nv[j], c));
        }
    } else {
        for (long e = threadIdx.x; e < chw; e += LOSS_THREADS) {
            const long i = base + e;
            const float xi = need_x ? x0[i] : 0.f, ni = need_n ? noise[i] : 0.f;
            acc += (double)loss_elem(kind, out[i] - loss_target(par, xi, ni, c));
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < LOSS_WAVES; ++i) s += red[i];
        const float raw = (float)(s / (double)chw);
        per_raw[n] = raw;
        per_w[n] = wt ? wt[tt] * raw : raw;
    }
}

// element-wise over [b, chw]: `bps` blocks of 256 threads per sample, a thread per quad (VEC) or per float, so the sample
// index is one scalar division per block and t / wt / gper are scalar loads.  Nothing passed by value changes from step to
// step: the upstream gradient is read from device memory.
template <bool VEC>
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                       const float* __restrict__ noise, const int64_t* __restrict__ t,
                                                       const float* __restrict__ sa, const float* __restrict__ s1,
                                                       const float* __restrict__ wt, const float* __restrict__ gper, float gscale,
                                                       int par, int kind, long chw, unsigned bps, float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * 256 + threadIdx.x;            // quad (VEC) or element of the sample
    if (u >= (VEC ? chw / 4 : chw)) return;
    const int64_t tt = t[n];
    loss_coef c = {0.f, 0.f};
    if (par == 2) c = {sa[tt], s1[tt]};
    float k = (gper[n] * (wt ? wt[tt] : 1.f)) / (float)chw;
    k = k * gscale;
    const bool need_x = par != 0, need_n = par != 1;
    if (VEC) {
        const long i = (long)n * chw + 4 * u;
        const f32x4 o = *reinterpret_cast<const f32x4*>(out + i);
        const f32x4 xv = load4(x0, i, need_x), nv = load4(noise, i, need_n);
        f32x4 g;
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = loss_grad(kind, o[j] - loss_target(par, xv[j], nv[j], c), k);
        *reinterpret_cast<f32x4*>(gout + i) = g;
    } else {
        const long i = (long)n * chw + u;
        const float xi = need_x ? x0[i] : 0.f, ni = need_n ? noise[i] : 0.f;
        gout[i] = loss_grad(kind, out[i] - loss_target(par, xi, ni, c), k);
    }
}

bool loss_args_ok(const float* out, const float* x0, const float* noise, const int64_t* t, const float* sa, const float* s1,
                  int32_t par, int32_t kind, int32_t b, int64_t chw) {
    if (!out || !t || b <= 0 || chw <= 0 || par < 0 || par > 2 || kind < 0 || kind > 2) return false;
    if (par != 1 && !noise) return false;
    if (par != 0 && !x0) return false;
    if (par == 2 && (!sa || !s1)) return false;
    return chw <= INT64_MAX / b;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

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
    if (loss_vec_ok(out, x0, noise, par, chw, nullptr))
        hipLaunchKernelGGL(loss_fwd_kernel<true>, dim3(b), dim3(LOSS_THREADS), 0, (hipStream_t)stream, out, x0, noise, t, sqrt_ac,
                           sqrt_1mac, wt, par, kind, (long)chw, per_raw, per_w);
    else
        hipLaunchKernelGGL(loss_fwd_kernel<false>, dim3(b), dim3(LOSS_THREADS), 0, (hipStream_t)stream, out, x0, noise, t, sqrt_ac,
                           sqrt_1mac, wt, par, kind, (long)chw, per_raw, per_w);
    return sgd_check_launch();
}

extern "C" int sgd_loss_bwd(const float* out, const float* x0, const float* noise, const int64_t* t, const float* sqrt_ac,
                            const float* sqrt_1mac, const float* wt, const float* gper, float gscale, int32_t par, int32_t kind,
                            int32_t b, int64_t chw, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!loss_args_ok(out, x0, noise, t, sqrt_ac, sqrt_1mac, par, kind, b, chw) || !gper || !gout) return SGD_ERR_ARG;
    const bool vec = loss_vec_ok(out, x0, noise, par, chw, gout);
    const int64_t units = vec ? chw / 4 : chw;
    const int64_t bps = (units + 255) / 256;
    if (bps > INT32_MAX / b) return SGD_ERR_ARG;
    const dim3 grid((unsigned)(bps * b));
    if (vec)
        hipLaunchKernelGGL(loss_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, out, x0, noise, t, sqrt_ac, sqrt_1mac,
                           wt, gper, gscale, par, kind, (long)chw, (unsigned)bps, gout);
    else
        hipLaunchKernelGGL(loss_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, out, x0, noise, t, sqrt_ac, sqrt_1mac,
                           wt, gper, gscale, par, kind, (long)chw, (unsigned)bps, gout);
    return sgd_check_launch();
}
