// The reduction tail every "loss and gradient in one pass" kernel shares ("Loss reductions"): N fp64 sums per block,
// published in ONE fixed order —
//   per thread -> wave_sum -> one LDS slot per wave, added by thread 0 in index order (block_sum)
//   one block:      thread 0 finishes the sums itself (no second launch)
//   several blocks: partials[N * block + k], which ONE block of a finalize launch sums thread-strided (thread t takes rows
//                   t, t + kBlock, ...), block_sum again, then the same finish
// `finish(k, total)` turns sum k into the fp32 loss: ScaledLoss for a plain scale, a kernel's own callable for anything else.
// The host side of the same rule: loss_blocks (how many blocks such a pass launches) and finish_scaled_loss.
#pragma once

#include "common.hpp"

namespace cusrl {

// loss k = float(total k * scale[k]), the product in double.  Travels by value in the kernarg segment.
template <int N>
struct ScaledLoss {
    double scale[N];
    __device__ __forceinline__ float operator()(int k, double total) const { return float(total * scale[k]); }
};

// The epilogue of a loss pass: every thread of the block calls it with its N partial sums.  `scratch`: kWavesPerBlock doubles.
template <int N, typename Finish>
__device__ __forceinline__ void publish_loss_sums(const double (&acc)[N], double *scratch, double *__restrict__ partials,
                                                  float *__restrict__ loss_out, const Finish &finish) {
    double total[N];
#pragma unroll
    for (int k = 0; k < N; ++k) total[k] = block_sum(acc[k], scratch);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) loss_out[k] = finish(k, total[k]);
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) partials[N * blockIdx.x + k] = total[k];
        }
    }
}

// The body of a one-block finalize launch over the `blocks` partial rows publish_loss_sums left.
template <int N, typename Finish>
__device__ __forceinline__ void finalize_loss_sums(const double *__restrict__ partials, int blocks, double *scratch,
                                                   float *__restrict__ loss_out, const Finish &finish) {
    double acc[N];
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kBlock) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += partials[N * b + k];
    }
    double total[N];
#pragma unroll
    for (int k = 0; k < N; ++k) total[k] = block_sum(acc[k], scratch);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) loss_out[k] = finish(k, total[k]);
    }
}

template <int N>
__global__ __launch_bounds__(kBlock) void scaled_loss_finalize_kernel(const double *__restrict__ partials, int blocks,
                                                                      ScaledLoss<N> scales, float *__restrict__ loss_out) {
    __shared__ double scratch[kWavesPerBlock];
    finalize_loss_sums<N>(partials, blocks, scratch, loss_out, scales);
}

// Blocks of a loss pass over n elements: one block, which finalises itself, up to 16 K elements (a discriminator batch is
// 6 K); beyond that 2048 elements per block, at most 1024 blocks (every thread strides from there on).
inline int64_t loss_blocks(int64_t n) {
    if (n <= 0) return 0;
    if (n <= int64_t(kBlock) * 64) return 1;
    const int64_t want = ceil_div(n, int64_t(kBlock) * 8);
    return want > 1024 ? 1024 : want;
}

// What follows the launch of a loss pass of `blocks` blocks: its status, and beyond one block the finalize launch.
template <int N>
inline int finish_scaled_loss(int64_t blocks, const double *partials, const ScaledLoss<N> &scales, float *loss_out,
                              hipStream_t stream) {
    if (int rc = launch_status()) return rc;
    if (blocks == 1) return 0;  // the one block finalised itself
    hipLaunchKernelGGL(scaled_loss_finalize_kernel<N>, dim3(1), dim3(kBlock), 0, stream, partials, int(blocks), scales, loss_out);
    return launch_status();
}

}  // namespace cusrl
