// out[r, h] = act(x[r, h] + bias[h]) over a contiguous fp32 [rows, H], in place or into `out`: the epilogue of a bias-free GEMM
// as ONE launch ("Distillation"; contract and activation codes: include/cusrl_hip.h).  A thread owns ONE column lane
// (4 floats when H % 4 == 0 and every pointer is 16-byte aligned, one float otherwise: the same arithmetic per element, so the
// same bits) and walks rows with a stride, so its slice of the bias is loaded once and stays in registers.  The 256 threads of
// a block are `cols` column lanes by 256 / cols rows, cols the power of two that covers a row's lanes (256 at most, then
// blockIdx.y tiles the row).  Each step is one rounded fp32 operation (the library is built with -ffp-contract=off) with the
// accurate expm1f / tanhf.  A lane loads its operand before it stores, so out may be x (hence no __restrict__).
#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kBiasActMaxBlocks = 2048;  // 8 blocks per CU; the row walk strides over what is left

template <int kAct>
__device__ __forceinline__ float bias_act_apply(float v, float alpha) {
    if (kAct == CUSRL_ACT_RELU) return v != v ? v : (v > 0.0f ? v : 0.0f);  // a NaN passes through, -0 -> +0
    if (kAct == CUSRL_ACT_ELU) return v > 0.0f ? v : alpha * expm1f(v);      // torch's formula; NaN: alpha * NaN
    if (kAct == CUSRL_ACT_TANH) return tanhf(v);                             // saturates at +-1, no exp of a large |v|
    return v;
}

// lanes: column lanes of a row (H / kWidth).  cols_log2: log2 of the column lanes of a block.
template <int kAct, int kWidth>
__global__ __launch_bounds__(kBlock) void bias_act_kernel(const float *x, const float *bias, float *out, int64_t rows,
                                                          int64_t lanes, int cols_log2, float alpha) {
    const int cols = 1 << cols_log2, rows_per_block = kBlock >> cols_log2;
    const int64_t lane = int64_t(blockIdx.y) * cols + (threadIdx.x & (cols - 1));
    if (lane >= lanes) return;
    const int64_t stride = int64_t(gridDim.x) * rows_per_block;
    int64_t row = int64_t(blockIdx.x) * rows_per_block + (threadIdx.x >> cols_log2);
    if constexpr (kWidth == 4) {
        const float4 b = reinterpret_cast<const float4 *>(bias)[lane];
        for (; row < rows; row += stride) {
            const int64_t i = row * lanes + lane;
            const float4 v = reinterpret_cast<const float4 *>(x)[i];
            reinterpret_cast<float4 *>(out)[i] =
                make_float4(bias_act_apply<kAct>(v.x + b.x, alpha), bias_act_apply<kAct>(v.y + b.y, alpha),
                            bias_act_apply<kAct>(v.z + b.z, alpha), bias_act_apply<kAct>(v.w + b.w, alpha));
        }
    } else {
        const float b = bias[lane];
        for (; row < rows; row += stride) {
            const int64_t i = row * lanes + lane;
            out[i] = bias_act_apply<kAct>(x[i] + b, alpha);
        }
    }
}

template <int kAct>
int launch_bias_act(const float *x, const float *bias, float *out, int64_t rows, int64_t H, float alpha, void *stream) {
    const bool vec = H % 4 == 0 && aligned(x, 16) && aligned(bias, 16) && aligned(out, 16);
    const int64_t lanes = vec ? H / 4 : H;
    int cols_log2 = 0;
    while (cols_log2 < 8 && (int64_t(1) << cols_log2) < lanes) ++cols_log2;
    const int64_t column_blocks = ceil_div(lanes, int64_t(1) << cols_log2);
    if (column_blocks > 65535) return CUSRL_E_UNSUPPORTED;  // gridDim.y
    int64_t row_blocks = ceil_div(rows, int64_t(kBlock >> cols_log2));
    const int64_t cap = kBiasActMaxBlocks / column_blocks > 0 ? kBiasActMaxBlocks / column_blocks : 1;
    if (row_blocks > cap) row_blocks = cap;
    const dim3 grid{uint32_t(row_blocks), uint32_t(column_blocks)}, block{kBlock};
    if (vec)
        hipLaunchKernelGGL((bias_act_kernel<kAct, 4>), grid, block, 0, as_stream(stream), x, bias, out, rows, lanes, cols_log2, alpha);
    else
        hipLaunchKernelGGL((bias_act_kernel<kAct, 1>), grid, block, 0, as_stream(stream), x, bias, out, rows, lanes, cols_log2, alpha);
    return launch_status();
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_bias_act(const float *x, const float *bias, float *out, int64_t rows, int64_t H, int activation, float alpha,
                              void *stream) {
    if (!x || !bias || !out || rows < 1 || H < 1) return CUSRL_E_INVALID;
    if (rows > INT64_MAX / H) return CUSRL_E_UNSUPPORTED;  // the element count beyond int64
    switch (activation) {
        case CUSRL_ACT_IDENTITY: return launch_bias_act<CUSRL_ACT_IDENTITY>(x, bias, out, rows, H, alpha, stream);
        case CUSRL_ACT_RELU: return launch_bias_act<CUSRL_ACT_RELU>(x, bias, out, rows, H, alpha, stream);
        case CUSRL_ACT_ELU: return launch_bias_act<CUSRL_ACT_ELU>(x, bias, out, rows, H, alpha, stream);
        case CUSRL_ACT_TANH: return launch_bias_act<CUSRL_ACT_TANH>(x, bias, out, rows, H, alpha, stream);
    }
    return CUSRL_E_UNSUPPORTED;
}
