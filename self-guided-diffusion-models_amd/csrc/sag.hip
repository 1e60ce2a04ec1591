// Self-attention guidance (Hong et al., ICCV 2023), the two launches between the two evaluations of a SAG step (gfx950;
// the reference has no such guidance):
//   sgd_attention_colmass : the attention each KEY receives, averaged over the heads -- the column sums of the softmax map the
//                           flash-style cores never materialise, re-formed from q, k and the cores' log-sum-exp
//   sgd_sag_degrade       : x0 / eps of the first evaluation, a 9-tap Gaussian blur of x0 where the upsampled mass exceeds the
//                           threshold, and the re-noised image the second evaluation reads -- one stencil launch out of LDS
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS), like guide.hip and vpred.hip: every product is rounded
// before it is added, so the torch-fp32 restatement (sgdm_amd/sag.py: sag_degrade_torch) reproduces sgd_sag_degrade bit for
// bit.  Neither kernel uses atomics: results depend on the inputs alone, captured or eager.
#include "sgdm_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------ attention mass
// mass[b, j] = (1 / heads) sum_h sum_i exp(scale <q[b,i,h,:], k[b,j,h,:]> - lse[b,h,i])
// One workgroup (CM_WAVES waves) owns CM_KEYS keys of one sample and loops over the heads and the queries.  A lane is a key:
// it keeps its key row of the current head in registers.  A wave is a query slot: it walks the queries wave, wave + CM_WAVES,
// ...; the query index is wave-uniform, so a q row and its lse arrive through the scalar cache and the inner loop is one fma
// per element with no vector memory traffic.  The sum over queries folds in a fixed order: the lane's own queries ascending
// (the heads accumulate in the lane), then the waves through LDS in ascending order.  A lane owns its key, so no step of the
// fold crosses lanes.
constexpr int CM_KEYS = 64;
constexpr int CM_WAVES = 8;

template <int D>
__global__ __launch_bounds__(CM_KEYS * CM_WAVES) void colmass_kernel(const float* __restrict__ q, int q_ld, int q_hs,
                                                                     const float* __restrict__ k, int kv_ld, int kv_hs,
                                                                     const float* __restrict__ lse, int heads, int tq, int tk,
                                                                     float scale, float* __restrict__ mass) {
    __shared__ float red[CM_WAVES][CM_KEYS];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = blockIdx.x * CM_KEYS + lane;
    const bool live = j < tk;                       // (a dead lane holds a zero key row: finite terms, never written)
    float acc = 0.f;
    for (int h = 0; h < heads; ++h) {
        f32x4 kr[D / 4];
        const float* kp = k + ((long)b * tk + (live ? j : 0)) * kv_ld + (long)h * kv_hs;
#pragma unroll
        for (int c = 0; c < D / 4; ++c) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + 4 * c);
            kr[c] = live ? kv : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float* qh = q + (long)b * tq * q_ld + (long)h * q_hs;
        const float* lh = lse + ((long)b * heads + h) * tq;
        for (int i = wave; i < tq; i += CM_WAVES) {
            const float* qp = qh + (long)i * q_ld;
            float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
            for (int c = 0; c < D / 4; ++c) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(qp + 4 * c);
                d0 = fmaf(qv.x, kr[c].x, d0);
                d1 = fmaf(qv.y, kr[c].y, d1);
                d2 = fmaf(qv.z, kr[c].z, d2);
                d3 = fmaf(qv.w, kr[c].w, d3);
            }
            acc += expf(scale * ((d0 + d1) + (d2 + d3)) - lh[i]);
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (threadIdx.x < CM_KEYS && live) {
        float sum = red[0][lane];
#pragma unroll
        for (int wv = 1; wv < CM_WAVES; ++wv) sum += red[wv][lane];
        mass[(long)b * tk + j] = sum / (float)heads;
    }
}

// ------------------------------------------------------------------------------------------------------------- degrade
constexpr int SD_TILE = 64;                         // output tile (a 64x64 plane is one workgroup: x and out are read once)
constexpr int SD_R = 4;                             // 9 taps
constexpr int SD_SIDE = SD_TILE + 2 * SD_R;
constexpr int SD_THREADS = 256;

// torch's 'reflect' for -n < i < 2n - 1
__device__ __forceinline__ int reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// One workgroup per (plane, tile).  Pass 1 forms x0 (and, inside the tile, eps) once per staged element -- the tile plus its
// 4-pixel halo, image borders reflected at staging, so both blur passes index LDS without a branch -- and copies the
// network output's rows on the way.  Pass 2: horizontal taps, LDS -> LDS.  Pass 3: vertical taps, the mask, the re-noise.
__global__ __launch_bounds__(SD_THREADS) void sag_degrade_kernel(const float* __restrict__ x, const float* __restrict__ out,
                                                                 int out_ld, int par, const int64_t* __restrict__ t,
                                                                 const float* __restrict__ sa_tab, const float* __restrict__ s1_tab,
                                                                 const float* __restrict__ mass, int mh, int mw, float thr,
                                                                 const float* __restrict__ taps, int c, int h, int w, int tiles_x,
                                                                 float* __restrict__ x_deg, float* __restrict__ out_copy) {
    __shared__ float s_x0[SD_SIDE * SD_SIDE];       // x0, tile + halo
    __shared__ float s_hp[SD_SIDE * SD_TILE];       // horizontal pass: rows of the halo too, the tile's columns
    __shared__ float s_e[SD_TILE * SD_TILE];        // eps, the tile alone
    const int plane = blockIdx.x, n = plane / c, cc = plane % c;
    const int x0_ = (blockIdx.y % tiles_x) * SD_TILE, y0_ = (blockIdx.y / tiles_x) * SD_TILE;
    const int tw = min(SD_TILE, w - x0_), th = min(SD_TILE, h - y0_);       // this tile's extent
    const int sw = tw + 2 * SD_R, sh = th + 2 * SD_R;
    const int hw = h * w;
    const int64_t tt = t[n];
    const float sa = sa_tab[tt], s1 = s1_tab[tt];
    float g[2 * SD_R + 1];
#pragma unroll
    for (int i = 0; i < 2 * SD_R + 1; ++i) g[i] = taps[i];
    const float* xp = x + (long)plane * hw;

    for (int i = threadIdx.x; i < sh * sw; i += SD_THREADS) {
        const int sy = i / sw, sx = i % sw;
        const int ty = sy - SD_R, tx = sx - SD_R;
        const int iy = reflect(y0_ + ty, h), ix = reflect(x0_ + tx, w);
        const int p = iy * w + ix;
        const float xv = xp[p];
        const float o = out[((long)n * hw + p) * out_ld + cc];
        float x0v, ev;
        if (par == 0) {
            ev = o;
            x0v = (xv - s1 * ev) / sa;
        } else if (par == 1) {
            x0v = o;
            ev = (xv - sa * x0v) / s1;
        } else {
            x0v = sa * xv - s1 * o;
            ev = sa * o + s1 * xv;
        }
        s_x0[sy * SD_SIDE + sx] = x0v;
        if (ty >= 0 && ty < th && tx >= 0 && tx < tw) {
            s_e[ty * SD_TILE + tx] = ev;
            if (out_copy) out_copy[((long)n * hw + p) * c + cc] = o;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < sh * tw; i += SD_THREADS) {
        const int sy = i / tw, tx = i % tw;
        const float* row = s_x0 + sy * SD_SIDE + tx;                        // staged column tx is image column tx - 4
        float acc = g[0] * row[0];
#pragma unroll
        for (int kk = 1; kk < 2 * SD_R + 1; ++kk) acc += g[kk] * row[kk];
        s_hp[sy * SD_TILE + tx] = acc;
    }
    __syncthreads();
    const float* mp = mass + (long)n * mh * mw;
    for (int i = threadIdx.x; i < th * tw; i += SD_THREADS) {
        const int ty = i / tw, tx = i % tw;
        const int y = y0_ + ty, xx = x0_ + tx;
        const float* col = s_hp + ty * SD_TILE + tx;
        float acc = g[0] * col[0];
#pragma unroll
        for (int kk = 1; kk < 2 * SD_R + 1; ++kk) acc += g[kk] * col[kk * SD_TILE];
        const bool m = mp[(int)(((long)y * mh) / h) * mw + (int)(((long)xx * mw) / w)] > thr;
        const float x0d = m ? acc : s_x0[(ty + SD_R) * SD_SIDE + tx + SD_R];
        x_deg[(long)plane * hw + y * w + xx] = sa * x0d + s1 * s_e[ty * SD_TILE + tx];
    }
}

}  // namespace

extern "C" int sgd_attention_colmass(const float* q, int32_t q_ld, int32_t q_hs, const float* k, int32_t kv_ld, int32_t kv_hs,
                                     const float* lse, int32_t batch, int32_t heads, int32_t tq, int32_t tk, int32_t d,
                                     float scale, float* mass, void* stream) {
    SGD_CLEAR_ERR();
    if (!q || !k || !lse || !mass || batch <= 0 || heads <= 0 || tq <= 0 || tk <= 0) return SGD_ERR_ARG;
    if ((q_ld & 3) || (q_hs & 3) || (kv_ld & 3) || (kv_hs & 3) || q_ld <= 0 || kv_ld <= 0 || q_hs < 0 || kv_hs < 0)
        return SGD_ERR_ARG;
    if ((((uintptr_t)q) | ((uintptr_t)k)) & 15) return SGD_ERR_ARG;
    if (batch > 65535) return SGD_ERR_ARG;
    const dim3 grid((unsigned)((tk + CM_KEYS - 1) / CM_KEYS), (unsigned)batch);
    hipStream_t st = (hipStream_t)stream;
    switch (d) {
        case 16: hipLaunchKernelGGL((colmass_kernel<16>), grid, dim3(CM_KEYS * CM_WAVES), 0, st, q, q_ld, q_hs, k, kv_ld, kv_hs, lse, heads, tq, tk, scale, mass); break;
        case 32: hipLaunchKernelGGL((colmass_kernel<32>), grid, dim3(CM_KEYS * CM_WAVES), 0, st, q, q_ld, q_hs, k, kv_ld, kv_hs, lse, heads, tq, tk, scale, mass); break;
        case 64: hipLaunchKernelGGL((colmass_kernel<64>), grid, dim3(CM_KEYS * CM_WAVES), 0, st, q, q_ld, q_hs, k, kv_ld, kv_hs, lse, heads, tq, tk, scale, mass); break;
        case 128: hipLaunchKernelGGL((colmass_kernel<128>), grid, dim3(CM_KEYS * CM_WAVES), 0, st, q, q_ld, q_hs, k, kv_ld, kv_hs, lse, heads, tq, tk, scale, mass); break;
        default: return SGD_ERR_ARG;
    }
    return sgd_check_launch();
}

extern "C" int sgd_sag_degrade(const float* x, const float* out_nhwc, int32_t out_ld, int32_t par, const int64_t* t,
                               const float* sa_tab, const float* s1_tab, const float* mass, int32_t mh, int32_t mw, float thr,
                               const float* taps_dev, int32_t b, int32_t c, int32_t h, int32_t w, float* x_deg, float* out_copy,
                               void* stream) {
    SGD_CLEAR_ERR();
    if (!x || !out_nhwc || !t || !sa_tab || !s1_tab || !mass || !taps_dev || !x_deg || b <= 0 || c <= 0) return SGD_ERR_ARG;
    if (par < 0 || par > 2 || out_ld < c) return SGD_ERR_ARG;
    if (h <= SD_R || w <= SD_R) return SGD_ERR_ARG;                 // 'reflect' needs the pad to be smaller than the side
    if (mh <= 0 || mw <= 0 || mh > h || mw > w) return SGD_ERR_ARG;
    if (x_deg == x) return SGD_ERR_ARG;                             // the halo of a tile is another tile's output
    const long planes = (long)b * c, tiles_x = (w + SD_TILE - 1) / SD_TILE, tiles = tiles_x * ((h + SD_TILE - 1) / SD_TILE);
    if ((long)h * w > INT32_MAX || planes > INT32_MAX || tiles > 65535) return SGD_ERR_ARG;
    hipLaunchKernelGGL(sag_degrade_kernel, dim3((unsigned)planes, (unsigned)tiles), dim3(SD_THREADS), 0, (hipStream_t)stream, x,
                       out_nhwc, out_ld, par, t, sa_tab, s1_tab, mass, mh, mw, thr, taps_dev, c, h, w, (int)tiles_x, x_deg,
                       out_copy);
    return sgd_check_launch();
}
