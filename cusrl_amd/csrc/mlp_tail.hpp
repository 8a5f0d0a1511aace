// What the one-launch MLP inference passes share (mlp_forward.hip: two hidden layers, mlp3_forward.hip: three): the MFMA
// accumulator type, the workgroup shape, ReLU as torch evaluates it, and the TAIL of a 16-row tile — the head's four per-wave
// partial sums added in wave order, the store of the mean, and the acting path's sampling epilogue (Normal.rsample + log_prob
// with the expressions and the association of cusrl_normal_sample_logp, rollout.hip).  One body: both kernels give the same
// bits for the same mean.
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

// Run by wave 0 behind the barrier that publishes `partial` ([wave][lane]: out^T[a = 4 kk + reg][m = i] of every wave's slice
// of the head's contraction).  Args: out, eps, action, logp, std_out, rows, A as in MlpForwardArgs.
template <class Args>
__device__ __forceinline__ void mlp_tail(const Args &p, const float4 (*partial)[kWave], int64_t row0, int lane,
                                         const float (&sigma)[4], const float (&noise)[4]) {
    const int i = lane & 15, kk = lane >> 4;
    const int A = p.A;
    // out^T[a = 4 kk + reg][m = i]: waves added in wave order (fixed)
    float4 sum = partial[0][lane];
#pragma unroll
    for (int w = 1; w < kMlpWaves; ++w) {
        const float4 v = partial[w][lane];
        sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
    }
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

}  // namespace cusrl
