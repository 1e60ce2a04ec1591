// Global-norm gradient clipping over the optimizer's tensor table (gfx950; include/sgdm_hip.h: sgd_grad_norm, sgd_grad_scale;
// the reference leaves clipping to Lightning's gradient_clip_val, i.e. torch.nn.utils.clip_grad_norm_ over ~390 tensors).
//
//   norm = sqrt(sum over every row with g != NULL of sum_e g[e]^2);   coef = min(1, max_norm / (norm + 1e-6f))
//
// The norm is two launches.  Stage 1: the grid of the optimizer step (one 256-thread block per 4096-element chunk of a tensor);
// a thread squares its 16 elements in double and adds them in ascending order, the block sums as loss_block_sum
// (csrc/loss_common.h) says and writes ONE double.  Stage 2: one block folds the per-chunk doubles in a fixed order and writes the
// record.  Why double: the square of an fp32 value is exact in it.  Gradients of order 1 / (B C H W) square into fp32's
// subnormals and vanish there, large ones overflow; in double neither happens, and the only rounding that matters is the last
// one, (float)sqrt(sum).  Both kernels are HBM-bound (4 bytes read per element, 8 flops), so the wider accumulator is free.
//
// Determinism: no atomics, no arrival counters.  Which elements a thread owns and the order in which anything is added depend on
// the list of n alone -- not on where a tensor lies (the 16-byte path below reads the same elements of the same thread as the
// 4-byte path), not on which block finishes first.  Data-parallel replicas hold bit-identical gradients after the exchange and so
// reach bit-identical coefficients without talking to each other again.
//
// This file is compiled with -ffp-contract=off (build.py: FILE_FLAGS): the coefficient is torch's fp32 formula operation by
// operation, and g * coef in sgd_grad_scale is one rounded product.
#include "loss_common.h"
#include "../../include/sgdm_hip.h"

namespace {
constexpr int OPT_CHUNK = 4096;                     // as csrc/misc.hip: the chunk of chunk_start
constexpr int CLIP_THREADS = 256;
constexpr int CLIP_QUADS = OPT_CHUNK / (4 * CLIP_THREADS);      // quads of a chunk per thread

// the tensor that owns chunk b: last t with chunk_start[t] <= b (as adamw_ema_kernel)
__device__ __forceinline__ int clip_owner(const int32_t* __restrict__ chunk_start, int count, int b) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_start[mid] <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// Thread i of a chunk owns the quads i, i + 256, i + 512, i + 768 of it.  A quad wholly inside the tensor is one 16-byte access
// when g sits on a 16-byte boundary (a chunk starts a multiple of 16 KiB behind it) and four 4-byte accesses otherwise; the quad
// that straddles the end is read element by element.  Elements past the end count as +0, which changes no sum.
__device__ __forceinline__ f32x4 clip_load_quad(const float* __restrict__ g, long e, long n, bool vec) {
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (vec && e + 4 <= n) return *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e + k < n) q[k] = g[e + k];
    return q;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_sq_kernel(const sgd_opt_tensor* __restrict__ table,
                                                               const int32_t* __restrict__ chunk_start, int count,
                                                               double* __restrict__ partials) {
    __shared__ double red[CLIP_THREADS / 64];
    const int b = blockIdx.x;
    const int ti = clip_owner(chunk_start, count, b);
    const float* __restrict__ g = table[ti].g;
    const long n = table[ti].n;
    const long base = (long)(b - chunk_start[ti]) * OPT_CHUNK;
    double acc = 0.0;
    if (g) {                                        // (block-uniform: every thread reaches the barrier below either way)
        const bool vec = ((uintptr_t)g & 15) == 0;
#pragma unroll
        for (int j = 0; j < CLIP_QUADS; ++j) {
            const long e = base + 4L * (threadIdx.x + j * CLIP_THREADS);
            if (e >= n) break;
            const f32x4 q = clip_load_quad(g, e, n, vec);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double x = (double)q[k];
                acc += x * x;
            }
        }
    }
    const double s = loss_block_sum<CLIP_THREADS>(acc, red);
    if (threadIdx.x == 0) partials[b] = s;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_norm_fold_kernel(const double* __restrict__ partials, int total_chunks,
                                                                      float max_norm, sgd_clip_record* __restrict__ rec) {
    __shared__ double red[CLIP_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < total_chunks; i += CLIP_THREADS) acc += partials[i];
    const double s = loss_block_sum<CLIP_THREADS>(acc, red);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(s);
    float coef = 1.f;
    if (isfinite(max_norm) && max_norm > 0.f) coef = fminf(1.f, __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f)));
    if (!isfinite(norm)) {                          // an inf or NaN gradient anywhere, or a sum past fp32's range
        rec->norm = norm;
        rec->coef = 0.f;
        rec->skip = 1;
        rec->nonfinite_steps += 1;
        return;
    }
    rec->norm = norm;
    rec->coef = coef;
    rec->skip = 0;
    if (coef < 1.f) rec->clipped_steps += 1;
}

__global__ __launch_bounds__(CLIP_THREADS) void grad_scale_kernel(const sgd_opt_tensor* __restrict__ table,
                                                                  const int32_t* __restrict__ chunk_start, int count,
                                                                  const sgd_clip_record* __restrict__ rec) {
    const float coef = rec->coef;
    if (coef == 1.f || rec->skip) return;           // an unclipped or a void step writes nothing
    const int b = blockIdx.x;
    const int ti = clip_owner(chunk_start, count, b);
    float* __restrict__ g = const_cast<float*>(table[ti].g);
    if (!g) return;
    const long n = table[ti].n;
    const long base = (long)(b - chunk_start[ti]) * OPT_CHUNK;
    const bool vec = ((uintptr_t)g & 15) == 0;
#pragma unroll
    for (int j = 0; j < CLIP_QUADS; ++j) {
        const long e = base + 4L * (threadIdx.x + j * CLIP_THREADS);
        if (e >= n) break;
        f32x4 q = clip_load_quad(g, e, n, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = __fmul_rn(q[k], coef);
        if (vec && e + 4 <= n) {
            *reinterpret_cast<f32x4*>(g + e) = q;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e + k < n) g[e + k] = q[k];
        }
    }
}
}  // namespace

extern "C" int sgd_grad_norm(const sgd_opt_tensor* table, const int32_t* chunk_start, int32_t count, int32_t total_chunks,
                             double* partials, float max_norm, sgd_clip_record* rec, void* stream) {
    SGD_CLEAR_ERR();
    if (!table || !chunk_start || !partials || !rec || count <= 0 || total_chunks <= 0) return SGD_ERR_ARG;
    hipLaunchKernelGGL(grad_sq_kernel, dim3(total_chunks), dim3(CLIP_THREADS), 0, (hipStream_t)stream, table, chunk_start,
                       count, partials);
    const int rc = sgd_check_launch();
    if (rc != SGD_OK) return rc;
    hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(CLIP_THREADS), 0, (hipStream_t)stream, partials, total_chunks,
                       max_norm, rec);
    return sgd_check_launch();
}

extern "C" int sgd_grad_scale(const sgd_opt_tensor* table, const int32_t* chunk_start, int32_t count, int32_t total_chunks,
                              const sgd_clip_record* rec, void* stream) {
    SGD_CLEAR_ERR();
    if (!table || !chunk_start || !rec || count <= 0 || total_chunks <= 0) return SGD_ERR_ARG;
    hipLaunchKernelGGL(grad_scale_kernel, dim3(total_chunks), dim3(CLIP_THREADS), 0, (hipStream_t)stream, table, chunk_start,
                       count, rec);
    return sgd_check_launch();
}
