// Perturbed-attention guidance (Ahn et al. 2024), the perturbed half of a self-attention layer (gfx950): the attention map is
// replaced by the identity, so every query's output is its own value row and the core (QK^T, softmax, PV) is not run at all.
// What is left is a strided gather of the v rows of the qkv buffer into the head-major attention output:
//   out[b, i, h*d + j] = v[b, i*kv_ld + h*kv_hs + j]
// -- what sgd_attention would write if every softmax row were the unit vector on the query's own key.  HBM-bound, no
// arithmetic: exact in every arithmetic mode (the qkv buffer is fp32 in all of them).  The reference has no such guidance.
//
// Addressing is sgd_attention's (include/sgdm_hip.h, "Attention cores"): the legacy layout (head stride 3*dp, the v offset
// folded into the pointer), the new-order layout (head stride dp) and zero-padded head widths (dp > d) are all strides.
#include "sgdm_common.h"
#include "../../include/sgdm_hip.h"

namespace {

// one lane per 16 bytes; consecutive lanes walk j, then h, then the row: the stores of a row are contiguous (heads*d floats),
// the loads contiguous per head.  Padding columns of either buffer are neither read nor written.
__global__ __launch_bounds__(256) void attention_identity_kernel(const float* __restrict__ v, int kv_ld, int kv_hs, long rows,
                                                                 int heads, int dq /* d / 4 */, float* __restrict__ out,
                                                                 int out_ld) {
    const long quads = rows * heads * dq;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (i >= quads) return;
    const int j = (int)(i % dq);
    const long hr = i / dq;
    const int h = (int)(hr % heads);
    const long row = hr / heads;
    const f32x4 val = *reinterpret_cast<const f32x4*>(v + row * kv_ld + (long)h * kv_hs + 4 * j);
    *reinterpret_cast<f32x4*>(out + row * out_ld + ((long)h * dq + j) * 4) = val;
}

}  // namespace

extern "C" int sgd_attention_identity(const float* v, int32_t kv_ld, int32_t kv_hs, int32_t batch, int32_t heads, int32_t t,
                                      int32_t d, float* out, int32_t out_ld, void* stream) {
    SGD_CLEAR_ERR();
    if (!v || !out || batch <= 0 || heads <= 0 || t <= 0) return SGD_ERR_ARG;
    if (d != 16 && d != 32 && d != 64 && d != 128) return SGD_ERR_ARG;
    if ((kv_ld & 3) || (kv_hs & 3) || (out_ld & 3) || kv_ld <= 0 || kv_hs < 0) return SGD_ERR_ARG;
    if ((long)heads * d > out_ld) return SGD_ERR_ARG;               // a row of the output holds every head
    if ((((uintptr_t)v) | ((uintptr_t)out)) & 15) return SGD_ERR_ARG;
    const long rows = (long)batch * t;
    const long quads = rows * heads * (d / 4);
    if (rows > INT32_MAX || (quads + 255) / 256 > INT32_MAX) return SGD_ERR_ARG;
    hipLaunchKernelGGL(attention_identity_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, v,
                       kv_ld, kv_hs, rows, heads, d / 4, out, out_ld);
    return sgd_check_launch();
}
