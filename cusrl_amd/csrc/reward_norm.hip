// RewardNormalization.post_step (cusrl_amd/hook/mdp/reward.py; DESIGN.md §7 "Reward normalisation"; contract, formulas and the
// summation order: include/cusrl_hip.h): the discounted return per env, its running mean / variance / count per reward column,
// the rescaled and clamped reward and the zeroed returns of finished envs.
//   cusrl_reward_normalize   ONE launch, ONE BLOCK OF 1024 THREADS PER REWARD COLUMN (R is 1 for every shipped task)
// The statistics need every row of a column before any reward of it can be rescaled.  A column is therefore one block: its 16 waves
// meet at __syncthreads and nothing else — no atomics, no hand-off between blocks, no fence beyond the block's own.
//   pass 1  G = G * gamma + r in place, thread-local float64 (s, q) of G - pivot
//   meet    wave tree, 16 wave totals through LDS, thread 0 merges into the running triple and publishes the scale through LDS
//   pass 2  r = clamp(r / scale), G = 0 where done
// A thread owns the same rows in both passes (chunks of 4 consecutive rows, chunk k to thread k % 1024), so the G it zeroes in
// pass 2 is the G it wrote in pass 1 and no row is touched by two threads.  The pivot, the column's first new return, is read by
// every thread BEFORE the barrier in front of pass 1, which overwrites it.  The element, merge and scale bodies are
// __host__ __device__; cusrl_reward_normalize_cpu runs them on the host and adds in the kernel's tree order, so the two differ only
// where the device's float64 division and square root would.  Plain vector stores only.  No loop's trip count depends on data.
#include "common.hpp"
#include "running_stats.hpp"

#include <math.h>

namespace cusrl {
namespace {

constexpr int kNormBlock = 1024, kNormWaves = kNormBlock / kWave, kChunk = 4;

struct Moments {
    double s, q;
};

__host__ __device__ __forceinline__ float discounted_return(float G, float gamma, float r) { return G * gamma + r; }

__host__ __device__ __forceinline__ void accumulate(Moments &m, float G, float pivot) {
    const double d = double(G) - double(pivot);
    m.s = m.s + d;
    m.q = m.q + d * d;
}

__host__ __device__ __forceinline__ float scaled_reward(float r, float scale, float clip, int has_clip) {
    float v = r / scale;
    if (has_clip) {
        v = v < -clip ? -clip : v;  // (a NaN fails both compares and stays)
        v = v > clip ? clip : v;
    }
    return v;
}

// Column c's sums into its running triple (stats points at mean[c]; var and count are R and 2 R further on), then the scale of
// the column's rewards: RunningMeanStd's two bodies (running_stats.hpp), the merge in float64.  update == 0: the triple is only read.
__host__ __device__ __forceinline__ float merge_and_scale(double *stats, int64_t R, Moments m, int64_t N, float pivot, double epsilon,
                                                          int update) {
    double mean = stats[0], var = stats[R];
    if (update) {
        const double n = double(N);
        const MeanVar batch = shifted_mean_var(m.s, m.q, n, double(pivot));
        stats[2 * R] = chan_merge(mean, var, stats[2 * R], batch.mean, batch.var, n);
        stats[0] = mean;
        stats[R] = var;
    }
    return float(sqrt(var + epsilon));
}

// rows i0 .. i0 + n of column c; kVec (R == 1, c == 0): a whole chunk as one 16-byte access
template <bool kVec>
__device__ __forceinline__ void load_chunk(const float *p, int64_t i0, int64_t c, int64_t R, int n, float *v) {
    if (kVec && n == kChunk) {
        const float4 r = *reinterpret_cast<const float4 *>(p + i0);
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
        if (j < n) v[j] = p[(i0 + j) * R + c];
}
template <bool kVec>
__device__ __forceinline__ void store_chunk(float *p, int64_t i0, int64_t c, int64_t R, int n, const float *v) {
    if (kVec && n == kChunk) {
        *reinterpret_cast<float4 *>(p + i0) = make_float4(v[0], v[1], v[2], v[3]);
        return;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
        if (j < n) p[(i0 + j) * R + c] = v[j];
}
template <bool kVec>
__device__ __forceinline__ void load_flags(const uint8_t *p, int64_t i0, int n, uint8_t *v) {
    if (kVec && n == kChunk) {
        const uchar4 f = *reinterpret_cast<const uchar4 *>(p + i0);
        v[0] = f.x, v[1] = f.y, v[2] = f.z, v[3] = f.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
        if (j < n) v[j] = p[i0 + j];
}

template <bool kVec>
__global__ __launch_bounds__(kNormBlock) void reward_normalize_kernel(float *reward, float *G, const uint8_t *__restrict__ terminated,
                                                                      const uint8_t *__restrict__ truncated, double *stats, float gamma,
                                                                      double epsilon, float clip, int has_clip, int update, int64_t N,
                                                                      int64_t R) {
    __shared__ double s_waves[2][kNormWaves];
    __shared__ float s_scale;
    const int64_t c = blockIdx.x;
    const int64_t chunks = (N + kChunk - 1) / kChunk;
    const float pivot = discounted_return(G[c], gamma, reward[c]);  // row 0 of the column
    __syncthreads();  // ... read by everyone before its owner overwrites G[0, c]
    Moments m = {0.0, 0.0};
    for (int64_t k = threadIdx.x; k < chunks; k += kNormBlock) {
        const int64_t i0 = k * kChunk;
        const int n = N - i0 < kChunk ? int(N - i0) : kChunk;
        float g[kChunk], r[kChunk];
        load_chunk<kVec>(G, i0, c, R, n, g);
        load_chunk<kVec>(reward, i0, c, R, n, r);
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (j < n) {
                g[j] = discounted_return(g[j], gamma, r[j]);
                accumulate(m, g[j], pivot);
            }
        store_chunk<kVec>(G, i0, c, R, n, g);
    }
    if (update) {  // (uniform over the block: the barriers inside are met by every thread or by none)
        m.s = block_sum<double, kNormWaves>(m.s, s_waves[0]);
        m.q = block_sum<double, kNormWaves>(m.q, s_waves[1]);
    }
    if (threadIdx.x == 0) s_scale = merge_and_scale(stats + c, R, m, N, pivot, epsilon, update);
    __syncthreads();
    const float scale = s_scale;
    for (int64_t k = threadIdx.x; k < chunks; k += kNormBlock) {
        const int64_t i0 = k * kChunk;
        const int n = N - i0 < kChunk ? int(N - i0) : kChunk;
        float r[kChunk];
        uint8_t ended[kChunk], cut[kChunk];
        load_chunk<kVec>(reward, i0, c, R, n, r);
        load_flags<kVec>(terminated, i0, n, ended);
        load_flags<kVec>(truncated, i0, n, cut);
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (j < n) r[j] = scaled_reward(r[j], scale, clip, has_clip);
        store_chunk<kVec>(reward, i0, c, R, n, r);
#pragma unroll
        for (int j = 0; j < kChunk; ++j)
            if (j < n && (ended[j] | cut[j])) G[(i0 + j) * R + c] = 0.0f;
    }
}

int check_normalize(const void *reward, const void *G, const void *terminated, const void *truncated, const void *stats, float clip,
                    int has_clip, int64_t N, int64_t R) {
    if (N < 0 || R < 1) return CUSRL_E_INVALID;
    if (has_clip && !(clip >= 0.0f)) return CUSRL_E_INVALID;
    if (N > 0 && (!reward || !G || !terminated || !truncated || !stats)) return CUSRL_E_INVALID;
    if (N > 0 && (!aligned(reward, 4) || !aligned(G, 4) || !aligned(stats, 8))) return CUSRL_E_INVALID;
    if (R > 65535 || N > INT64_MAX / kChunk / R) return CUSRL_E_UNSUPPORTED;
    return 0;
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_reward_normalize(float *reward, float *G, const uint8_t *terminated, const uint8_t *truncated, double *stats,
                                      float gamma, double epsilon, float clip, int has_clip, int update, int64_t N, int64_t R,
                                      void *stream) {
    if (int rc = check_normalize(reward, G, terminated, truncated, stats, clip, has_clip, N, R)) return rc;
    if (N == 0) return 0;
    const dim3 grid{uint32_t(R)}, block{kNormBlock};
    const bool vec = R == 1 && aligned(reward, 16) && aligned(G, 16) && aligned(terminated, 4) && aligned(truncated, 4);
    if (vec)
        hipLaunchKernelGGL(reward_normalize_kernel<true>, grid, block, 0, as_stream(stream), reward, G, terminated, truncated, stats,
                           gamma, epsilon, clip, has_clip, update, N, R);
    else
        hipLaunchKernelGGL(reward_normalize_kernel<false>, grid, block, 0, as_stream(stream), reward, G, terminated, truncated, stats,
                           gamma, epsilon, clip, has_clip, update, N, R);
    return launch_status();
}

extern "C" int cusrl_reward_normalize_cpu(float *reward, float *G, const uint8_t *terminated, const uint8_t *truncated, double *stats,
                                          float gamma, double epsilon, float clip, int has_clip, int update, int64_t N, int64_t R) {
    if (int rc = check_normalize(reward, G, terminated, truncated, stats, clip, has_clip, N, R)) return rc;
    if (N == 0) return 0;
    const int64_t chunks = (N + kChunk - 1) / kChunk;
    for (int64_t c = 0; c < R; ++c) {
        const float pivot = discounted_return(G[c], gamma, reward[c]);
        static thread_local Moments part[kNormBlock];  // what each thread of the block holds after pass 1
        for (int t = 0; t < kNormBlock; ++t) part[t] = {0.0, 0.0};
        for (int64_t k = 0; k < chunks; ++k)  // (ascending k visits the chunks of thread k % 1024 in that thread's order)
            for (int64_t i = k * kChunk; i < N && i < (k + 1) * kChunk; ++i) {
                G[i * R + c] = discounted_return(G[i * R + c], gamma, reward[i * R + c]);
                accumulate(part[k % kNormBlock], G[i * R + c], pivot);
            }
        Moments total = {0.0, 0.0};
        for (int w = 0; update && w < kNormWaves; ++w) {  // wave_sum's halving tree, then block_sum's wave order
            Moments *lane = part + w * kWave;
            for (int off = kWave / 2; off > 0; off >>= 1)
                for (int l = 0; l < off; ++l) lane[l] = {lane[l].s + lane[l + off].s, lane[l].q + lane[l + off].q};
            total = {total.s + lane[0].s, total.q + lane[0].q};
        }
        const float scale = merge_and_scale(stats + c, R, total, N, pivot, epsilon, update);
        for (int64_t i = 0; i < N; ++i) {
            reward[i * R + c] = scaled_reward(reward[i * R + c], scale, clip, has_clip);
            if (terminated[i] | truncated[i]) G[i * R + c] = 0.0f;
        }
    }
    return 0;
}
