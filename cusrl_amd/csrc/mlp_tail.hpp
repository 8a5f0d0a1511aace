// What the one-launch MLP inference passes share (mlp_forward.hip: two hidden layers, mlp3_forward.hip: three,
// mlp2_wave_forward.hip: two small ones in one wave): the MFMA accumulator type, the workgroup shape, the activations as torch
// evaluates them, and the TAIL of a 16-row tile — the head's four per-wave partial sums added in wave order (mlp_tail; a kernel
// whose head is complete inside one wave skips that), then mlp_tail_body: the store of the mean and the acting path's sampling
// epilogue (Normal.rsample + log_prob with the expressions and the association of cusrl_normal_sample_logp, rollout.hip).  One
// body: all three kernels give the same bits for the same mean.
#pragma once

#include "common.hpp"

namespace cusrl {

typedef float mfma_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMlpWaves = 4;
constexpr int kMlpThreads = kMlpWaves * kWave;
constexpr int kMlpRows = 16;  // rows of one tile (the N dimension of the MFMA)

__device__ __forceinline__ float log_sqrt_2pi_f() { return 0.91893853320467274178f; }

// relu as torch evaluates it: a NaN stays a NaN (v <= 0 is false for it), -0 becomes +0
__device__ __forceinline__ mfma_f32x4 relu4(mfma_f32x4 v) {
    v[0] = v[0] <= 0.f ? 0.f : v[0], v[1] = v[1] <= 0.f ? 0.f : v[1], v[2] = v[2] <= 0.f ? 0.f : v[2], v[3] = v[3] <= 0.f ? 0.f : v[3];
    return v;
}

// the activation on a tile's accumulator registers, with the expressions of cusrl_bias_act (bias_act.hip)
template <int ACT>
__device__ __forceinline__ mfma_f32x4 act4(mfma_f32x4 v, float alpha) {
    if constexpr (ACT == CUSRL_ACT_RELU) {
        return relu4(v);
    } else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            if constexpr (ACT == CUSRL_ACT_ELU) v[reg] = v[reg] > 0.0f ? v[reg] : alpha * expm1f(v[reg]);  // torch's formula
            else v[reg] = tanhf(v[reg]);
        }
        return v;
    }
}

__device__ __forceinline__ float pick(const float4 &v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

__device__ __forceinline__ mfma_f32x4 from_bias(const float *b) {
    const float4 v = *reinterpret_cast<const float4 *>(b);
    return mfma_f32x4{v.x, v.y, v.z, v.w};
}

// sampling epilogue operands of a lane (kk = lane >> 4 owns actions 4 kk .. 4 kk + 3 of row lane & 15): its four std values,
// once per launch; its four eps values, once per tile (indices clamped: lanes past A or past the last row re-read valid ones)
__device__ __forceinline__ void mlp_tail_sigma(const float *std, int A, int kk, float (&sigma)[4]) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) sigma[reg] = std[min(4 * kk + reg, A - 1)];
}

__device__ __forceinline__ void mlp_tail_noise(const float *eps, int64_t rows, int A, int64_t row0, int lane, float (&noise)[4]) {
    const int64_t first = min(row0 + (lane & 15), rows - 1) * A;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) noise[reg] = eps[first + min(4 * (lane >> 4) + reg, A - 1)];
}

// Everything behind the head's sum: `sum` is out^T[a = 4 kk + reg][m = i] of this lane, complete.  Args: out, eps, action, logp,
// std_out, rows, A as in MlpForwardArgs.
template <class Args>
__device__ __forceinline__ void mlp_tail_body(const Args &p, const float4 sum, int64_t row0, int lane, const float (&sigma)[4],
                                              const float (&noise)[4]) {
    const int i = lane & 15, kk = lane >> 4;
    const int A = p.A;
    const bool live = row0 + i < p.rows;
    const int a0 = 4 * kk;
    const int64_t at = (row0 + i) * A + a0;
    const float mu[4] = {sum.x, sum.y, sum.z, sum.w};
    if (live && p.out) {
        if (A % 4 == 0) {
            if (a0 < A) *reinterpret_cast<float4 *>(p.out + at) = sum;
        } else {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (a0 + reg < A) p.out[at + reg] = mu[reg];
        }
    }
    if (p.eps) {
        // Normal.rsample + log_prob with the expressions of normal_sample_logp_kernel (rollout.hip): a lane evaluates its
        // four actions, lane kk == 0 of a row adds the row's terms up in action order (its own, then the other three
        // lanes' through shuffles): the association of the one-lane-per-row kernel
        float term[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int a = a0 + reg;
            if (a < A) {
                const float sg = sigma[reg];
                const float act = mu[reg] + noise[reg] * sg;
                const float diff = act - mu[reg];
                term[reg] = -(diff * diff) / (2.0f * (sg * sg)) - logf(sg) - log_sqrt_2pi_f();
                if (live) {
                    p.action[at + reg] = act;
                    if (p.std_out) p.std_out[at + reg] = sg;
                }
            }
        }
        float lp = 0.f;
#pragma unroll
        for (int src = 0; src < 4; ++src)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const float t = __shfl(term[reg], i + 16 * src, kWave);
                if (4 * src + reg < A) lp += t;
            }
        if (live && kk == 0) p.logp[row0 + i] = lp;
    }
}

// Run by wave 0 behind the barrier that publishes `partial` ([wave][lane]: out^T[a = 4 kk + reg][m = i] of every wave's slice
// of the head's contraction): the waves added in wave order (fixed), then the body above.
template <class Args>
__device__ __forceinline__ void mlp_tail(const Args &p, const float4 (*partial)[kWave], int64_t row0, int lane,
                                         const float (&sigma)[4], const float (&noise)[4]) {
    float4 sum = partial[0][lane];
#pragma unroll
    for (int w = 1; w < kMlpWaves; ++w) {
        const float4 v = partial[w][lane];
        sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
    }
    mlp_tail_body(p, sum, row0, lane, sigma, noise);
}

}  // namespace cusrl
