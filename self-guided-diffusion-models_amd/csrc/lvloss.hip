// Hybrid loss of a learned-variance model (Nichol & Dhariwal 2021, "Improved DDPM": L_simple + lambda L_vlb) and its gradient
// (gfx950; include/sgdm_hip.h: sgd_lv_loss_fwd, sgd_lv_loss_bwd; the reference has no learned variance).  `out` is the model
// output [b, 2C, hw] in NCHW: m = out[:, :C] predicts the trained target, v = out[:, C:] interpolates the reverse-process
// log-variance between max_log[t] = log beta_t and min_log[t] = log beta~_t.  Per element, t = t[n]:
//   simple  l  = loss_elem(m - target)                          sgd_loss_fwd's term on the mean half (csrc/loss_common.h)
//   x_t     = sa x0 + s1 noise                                  (the bits of sgd_q_sample)
//   x0p     = r0 x_t - r1 m (par 0) | m (par 1) | sa x_t - s1 m (par 2),    not clipped
//   mu_th   = c1 x0p + c2 x_t,   mu_q = c1 x0 + c2 x_t
//   frac    = (v + 1) / 2,       lv = frac max_log + (1 - frac) min_log
//   t > 0 : L = 0.5 (-1 + lv - lq + exp(lq - lv) + (mu_q - mu_th)^2 exp(-lv)) / ln 2,      lq = min_log[t]
//   t == 0: L = -log max(P, 1e-12) / ln 2, the discretized-Gaussian decoder: inv = exp(-0.5 lv), d = x0 - mu_th,
//           Phi(u) = 0.5 (1 + tanh(sqrt(2/pi) (u + 0.044715 u^3))), cp = Phi(inv (d + 1/255)), cm = Phi(inv (d - 1/255)),
//           P = cp (x0 < -0.999) | 1 - cm (x0 > 0.999) | cp - cm
// The t == 0 branch runs in double from the fp32 inputs, forward and backward: cp - cm cancels in fp32 from about four standard
// deviations out.  t is per sample, so the branch is uniform per workgroup (forward) and per block (backward).
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like loss.hip: the simple term and the mean-half
// gradient are loss_elem / loss_grad / loss_target of csrc/loss_common.h, the code of sgd_loss_fwd / sgd_loss_bwd.  The gradient
// of L stops at the mean (the paper's rule): the mean half gets sgd_loss_bwd's gradient, the variance half
// gper_vlb / (C hw) * dL/dlv * 0.5 (max_log - min_log).
#include "loss_common.h"
#include "../../include/sgdm_hip.h"

namespace {

constexpr float LV_LN2 = 0.6931471805599453f;
constexpr double LV_LN2_D = 0.6931471805599453;
constexpr double LV_SQRT_2_PI = 0.7978845608028654;  // sqrt(2 / pi)

struct lv_coef { float sa, s1, r0, r1, c1, c2, mx, mn; };

struct lv_tables {
    const float *sa, *s1, *r0, *r1, *c1, *c2, *mx, *mn;
};

__device__ __forceinline__ lv_coef lv_load(const lv_tables& tb, int64_t tt, int par) {
    lv_coef c = {tb.sa[tt], tb.s1[tt], 0.f, 0.f, tb.c1[tt], tb.c2[tt], tb.mx[tt], tb.mn[tt]};
    if (par == 0) { c.r0 = tb.r0[tt]; c.r1 = tb.r1[tt]; }
    return c;
}

// t > 0, fp32: the KL of the two Gaussians in bits (dl == nullptr) and, for the backward, dL / dlv
__device__ __forceinline__ float lv_kl(int par, float m, float v, float xi, float ni, const lv_coef& c, float* dl) {
    const float xt = c.sa * xi + c.s1 * ni;
    const float x0p = par == 0 ? c.r0 * xt - c.r1 * m : par == 1 ? m : c.sa * xt - c.s1 * m;
    const float mu_th = c.c1 * x0p + c.c2 * xt, mu_q = c.c1 * xi + c.c2 * xt;
    const float frac = (v + 1.f) * 0.5f;
    const float lv = frac * c.mx + (1.f - frac) * c.mn;
    const float lq = c.mn;
    const float dm = mu_q - mu_th;
    const float e1 = expf(lq - lv), e2 = (dm * dm) * expf(-lv);
    if (dl) *dl = (0.5f * ((1.f - e1) - e2)) / LV_LN2;
    return (0.5f * ((((-1.f + lv) - lq) + e1) + e2)) / LV_LN2;
}

__device__ __forceinline__ double lv_phi(double u, double* dphi) {
    const double g = LV_SQRT_2_PI * (u + 0.044715 * u * u * u);
    const double th = tanh(g);
    if (dphi) *dphi = 0.5 * (1.0 - th * th) * (LV_SQRT_2_PI * (1.0 + 3.0 * 0.044715 * u * u));
    return 0.5 * (1.0 + th);
}

// t == 0, double from the fp32 inputs: the decoder NLL in bits and, for the backward, dL / dlv (0 where the clamp holds:
// torch's clamp passes the gradient where its input is >= the bound)
__device__ __forceinline__ double lv_decoder(int par, float m, float v, float xi, float ni, const lv_coef& c, double* dl) {
    const double xd = xi, md = m;
    const double xt = (double)c.sa * xd + (double)c.s1 * (double)ni;
    const double x0p = par == 0 ? (double)c.r0 * xt - (double)c.r1 * md : par == 1 ? md : (double)c.sa * xt - (double)c.s1 * md;
    const double mu_th = (double)c.c1 * x0p + (double)c.c2 * xt;
    const double frac = ((double)v + 1.0) * 0.5;
    const double lv = frac * (double)c.mx + (1.0 - frac) * (double)c.mn;
    const double inv = exp(-0.5 * lv), d = xd - mu_th;
    const double up = inv * (d + 1.0 / 255.0), um = inv * (d - 1.0 / 255.0);
    double dp = 0.0, dmn = 0.0;
    const double cp = lv_phi(up, dl ? &dp : nullptr), cm = lv_phi(um, dl ? &dmn : nullptr);
    // d u / d lv = -0.5 u
    double P, dP;
    if (xi < -0.999f) { P = cp; dP = dp * (-0.5 * up); }
    else if (xi > 0.999f) { P = 1.0 - cm; dP = -(dmn * (-0.5 * um)); }
    else { P = cp - cm; dP = dp * (-0.5 * up) - dmn * (-0.5 * um); }
    if (dl) *dl = P >= 1e-12 ? -(dP / P) / LV_LN2_D : 0.0;
    return -log(fmax(P, 1e-12)) / LV_LN2_D;
}

// W == 4: hw % 4 == 0 and every tensor 16-byte aligned (then both halves of every sample start on a 16-byte boundary):
// consecutive lanes read consecutive 16-byte quads of m, v, x0 and noise.  W == 1: one float per lane.  Two sums, each as
// loss_block_sum (csrc/loss_common.h).
template <int W>
__global__ __launch_bounds__(LOSS_FWD_THREADS) void lv_loss_fwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                                       const float* __restrict__ noise,
                                                                       const int64_t* __restrict__ t, lv_tables tb,
                                                                       const float* __restrict__ wt, int par, int kind, long chw,
                                                                       float* __restrict__ per_raw, float* __restrict__ per_w,
                                                                       float* __restrict__ per_vlb) {
    __shared__ double red_s[LOSS_FWD_THREADS / 64], red_v[LOSS_FWD_THREADS / 64];
    const int n = blockIdx.x;
    const int64_t tt = t[n];
    const lv_coef c = lv_load(tb, tt, par);
    const float* __restrict__ mp = out + 2 * (long)n * chw;
    const long base = (long)n * chw;
    const bool dec = tt == 0;
    double acc_s = 0.0, acc_v = 0.0;
    for (long u = threadIdx.x; u < chw / W; u += LOSS_FWD_THREADS) {
        const long e = W * u;
        const loss_vec<W> mv = loss_load<W>(mp, e), vv = loss_load<W>(mp, chw + e);
        const loss_vec<W> xv = loss_load<W>(x0, base + e), nv = loss_load<W>(noise, base + e);
#pragma unroll
        for (int j = 0; j < W; ++j) {
            acc_s += (double)loss_elem(kind, mv[j] - loss_target(par, xv[j], nv[j], c.sa, c.s1));
            acc_v += dec ? lv_decoder(par, mv[j], vv[j], xv[j], nv[j], c, nullptr)
                         : (double)lv_kl(par, mv[j], vv[j], xv[j], nv[j], c, nullptr);
        }
    }
    const double ss = loss_block_sum<LOSS_FWD_THREADS>(acc_s, red_s), sv = loss_block_sum<LOSS_FWD_THREADS>(acc_v, red_v);
    if (threadIdx.x == 0) {
        const float raw = (float)(ss / (double)chw);
        per_raw[n] = raw;
        per_w[n] = wt ? wt[tt] * raw : raw;
        per_vlb[n] = (float)(sv / (double)chw);
    }
}

// `bps` blocks per sample, a thread per quad (W == 4) or per element of [C, hw]: it writes the element's gradient in BOTH halves,
// so every input is read once.  gper_w / gper_vlb are read from device memory: nothing by value depends on the step.
template <int W>
__global__ __launch_bounds__(LOSS_BWD_THREADS) void lv_loss_bwd_kernel(const float* __restrict__ out, const float* __restrict__ x0,
                                                                       const float* __restrict__ noise,
                                                                       const int64_t* __restrict__ t, lv_tables tb,
                                                                       const float* __restrict__ wt,
                                                                       const float* __restrict__ gper_w,
                                                                       const float* __restrict__ gper_vlb, int par, int kind,
                                                                       long chw, unsigned bps, float* __restrict__ gout) {
    const int n = blockIdx.x / bps;
    const long u = (long)(blockIdx.x % bps) * LOSS_BWD_THREADS + threadIdx.x;
    if (u >= chw / W) return;
    const int64_t tt = t[n];
    const lv_coef c = lv_load(tb, tt, par);
    const float k = (gper_w[n] * (wt ? wt[tt] : 1.f)) / (float)chw;           // sgd_loss_bwd's factor (its gscale is 1)
    const float kv = (gper_vlb[n] / (float)chw) * (0.5f * (c.mx - c.mn));
    const double kvd = ((double)gper_vlb[n] / (double)chw) * (0.5 * ((double)c.mx - (double)c.mn));
    const bool dec = tt == 0;
    const long e = 2 * (long)n * chw + W * u, i = (long)n * chw + W * u;      // in out / gout (mean half), in x0 / noise
    const loss_vec<W> mv = loss_load<W>(out, e), vv = loss_load<W>(out, e + chw);
    const loss_vec<W> xv = loss_load<W>(x0, i), nv = loss_load<W>(noise, i);
    loss_vec<W> g, gv;
#pragma unroll
    for (int j = 0; j < W; ++j) {
        g[j] = loss_grad(kind, mv[j] - loss_target(par, xv[j], nv[j], c.sa, c.s1), k);
        if (dec) {
            double dl;
            lv_decoder(par, mv[j], vv[j], xv[j], nv[j], c, &dl);
            gv[j] = (float)(kvd * dl);
        } else {
            float dl;
            lv_kl(par, mv[j], vv[j], xv[j], nv[j], c, &dl);
            gv[j] = kv * dl;
        }
    }
    loss_store<W>(gout, e, g);
    loss_store<W>(gout, e + chw, gv);
}

bool lv_args_ok(const float* out, const float* x0, const float* noise, const int64_t* t, const sgd_lv_tables* tb, int32_t par,
                int32_t kind, int32_t b, int32_t c, int32_t hw) {
    if (!out || !x0 || !noise || !t || !tb || b <= 0 || c <= 0 || hw <= 0 || par < 0 || par > 2 || kind < 0 || kind > 2)
        return false;
    if (!tb->sqrt_ac || !tb->sqrt_1mac || !tb->mean_coef1 || !tb->mean_coef2 || !tb->max_log || !tb->min_log) return false;
    if (par == 0 && (!tb->sqrt_recip_ac || !tb->sqrt_recipm1_ac)) return false;
    return (int64_t)c * hw <= INT64_MAX / 2 / b;
}

bool lv_vec_ok(const float* out, const float* x0, const float* noise, int32_t hw, const float* gout) {
    return hw % 4 == 0 && aligned16(out) && aligned16(x0) && aligned16(noise) && aligned16(gout);
}

lv_tables lv_dev_tables(const sgd_lv_tables* tb) {
    return {tb->sqrt_ac, tb->sqrt_1mac, tb->sqrt_recip_ac, tb->sqrt_recipm1_ac, tb->mean_coef1, tb->mean_coef2, tb->max_log,
            tb->min_log};
}

}  // namespace

extern "C" int sgd_lv_loss_fwd(const float* out, const float* x0, const float* noise, const int64_t* t, const sgd_lv_tables* tables,
                               const float* wt, int32_t par, int32_t kind, int32_t b, int32_t c, int32_t hw, float* per_raw,
                               float* per_w, float* per_vlb, void* stream) {
    SGD_CLEAR_ERR();
    if (!lv_args_ok(out, x0, noise, t, tables, par, kind, b, c, hw) || !per_raw || !per_w || !per_vlb) return SGD_ERR_ARG;
    const long chw = (long)c * hw;
    return loss_launch(lv_vec_ok(out, x0, noise, hw, nullptr), lv_loss_fwd_kernel<4>, lv_loss_fwd_kernel<1>, (unsigned)b,
                       LOSS_FWD_THREADS, stream, out, x0, noise, t, lv_dev_tables(tables), wt, par, kind, chw, per_raw, per_w,
                       per_vlb);
}

extern "C" int sgd_lv_loss_bwd(const float* out, const float* x0, const float* noise, const int64_t* t, const sgd_lv_tables* tables,
                               const float* wt, const float* gper_w, const float* gper_vlb, int32_t par, int32_t kind, int32_t b,
                               int32_t c, int32_t hw, float* gout, void* stream) {
    SGD_CLEAR_ERR();
    if (!lv_args_ok(out, x0, noise, t, tables, par, kind, b, c, hw) || !gper_w || !gper_vlb || !gout) return SGD_ERR_ARG;
    const long chw = (long)c * hw;
    const bool vec = lv_vec_ok(out, x0, noise, hw, gout);
    const unsigned bps = loss_bps(vec, chw, b);
    if (!bps) return SGD_ERR_ARG;
    return loss_launch(vec, lv_loss_bwd_kernel<4>, lv_loss_bwd_kernel<1>, bps * b, LOSS_BWD_THREADS, stream, out, x0, noise, t,
                       lv_dev_tables(tables), wt, gper_w, gper_vlb, par, kind, chw, bps, gout);
}
