// Residual add + LayerNorm, forward and backward ("Residual add + LayerNorm"): the row-wise work between the GEMMs
// of a pre-LayerNorm residual backbone (cusrl/nn/module/simba.py:28-73).  One wavefront owns one row, which it reads from
// memory once and keeps in registers: lane l holds the 4-column chunks l, l + 64, ... (at most kMaxChunks of them, 16 values).
// The chunk a lane owns does not depend on how it is loaded — one 16-byte access when every pointer is 16-byte aligned and
// H % 4 == 0, four guarded 4-byte accesses otherwise — so every sum runs in the same order on both paths and an offset view
// gives the bits of the aligned call.  Statistics and column sums are accumulated in float64 and rounded to fp32 once.
#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kMaxChunks = CUSRL_MAX_LAYER_NORM_WIDTH / (4 * kWave);  // 16-byte chunks of the widest row per lane
constexpr int kBwdWaves = 8;                                         // waves (= rows in flight) per block of the backward
constexpr int kBwdBlock = kBwdWaves * kWave;
constexpr int kBwdMaxBlocks = 256;  // partial rows the one-block finalize sums
constexpr int kBwdRowsPerWave = 4;  // below the cap a wave walks this many rows, so small batches leave few partial rows

// Row `p` [H] into v[k][j] = p[(lane + 64 k) * 4 + j], zeros beyond H.
template <int kChunks, bool kVec>
__device__ __forceinline__ void load_row(const float *__restrict__ p, int H, int lane, float (&v)[kChunks][4]) {
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
        const int c = (lane + kWave * k) * 4;
        if (kVec) {
            const float4 q = c < H ? *reinterpret_cast<const float4 *>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            v[k][0] = q.x, v[k][1] = q.y, v[k][2] = q.z, v[k][3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[k][j] = c + j < H ? p[c + j] : 0.f;
        }
    }
}

template <int kChunks, bool kVec>
__device__ __forceinline__ void store_row(float *__restrict__ p, int H, int lane, const float (&v)[kChunks][4]) {
#pragma unroll
    for (int k = 0; k < kChunks; ++k) {
        const int c = (lane + kWave * k) * 4;
        if (kVec) {
            if (c < H) *reinterpret_cast<float4 *>(p + c) = make_float4(v[k][0], v[k][1], v[k][2], v[k][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + j < H) p[c + j] = v[k][j];
        }
    }
}

// The wave's total in every lane (wave_sum's fixed order, then a broadcast of lane 0).
__device__ __forceinline__ double wave_total(double v) { return __shfl(wave_sum(v), 0, kWave); }

template <int kChunks, bool kVec>
__global__ __launch_bounds__(kBlock) void add_layer_norm_fwd_kernel(const float *__restrict__ x, const float *__restrict__ residual,
                                                                    const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                    float eps, float *__restrict__ sum_out, float *__restrict__ y,
                                                                    float *__restrict__ mean_out, float *__restrict__ rstd_out,
                                                                    int64_t B, int H) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = int64_t(blockIdx.x) * kWavesPerBlock + threadIdx.x / kWave;
    if (row >= B) return;  // (whole waves leave; the kernel has no barrier)
    const int64_t base = row * H;
    float s[kChunks][4];
    load_row<kChunks, kVec>(x + base, H, lane, s);
    if (residual != nullptr) {
        float r[kChunks][4];
        load_row<kChunks, kVec>(residual + base, H, lane, r);
#pragma unroll
        for (int k = 0; k < kChunks; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[k][j] = s[k][j] + r[k][j];  // one fp32 add: torch's x + residual
        store_row<kChunks, kVec>(sum_out + base, H, lane, s);
    }
    // two passes over the registers: the mean, then the squared distances from it (the padding adds exact zeros to the first)
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kChunks; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += double(s[k][j]);
    const double mean = wave_total(acc) / double(H);
    acc = 0.0;
#pragma unroll
    for (int k = 0; k < kChunks; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double d = double(s[k][j]) - mean;
            if ((lane + kWave * k) * 4 + j < H) acc += d * d;
        }
    const double var = wave_total(acc) / double(H);  // biased, like torch
    const float mean_f = float(mean), rstd_f = float(1.0 / sqrt(var + double(eps)));
    if (mean_out != nullptr && lane == 0) mean_out[row] = mean_f, rstd_out[row] = rstd_f;
    float g[kChunks][4], b[kChunks][4];
    load_row<kChunks, kVec>(gamma, H, lane, g);
    load_row<kChunks, kVec>(beta, H, lane, b);
#pragma unroll
    for (int k = 0; k < kChunks; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[k][j] = (s[k][j] - mean_f) * rstd_f * g[k][j] + b[k][j];
    store_row<kChunks, kVec>(y + base, H, lane, s);
}

// d_s = rstd * (g - mean(g) - xhat * mean(g * xhat)) + ds with g = dy * gamma, xhat = (s - mean) * rstd; the block's column
// sums of dy * xhat and dy (float64) go to its row of `partials` [2 H] — or, from the only block, straight to d_gamma / d_beta.
template <int kChunks, bool kVec>
__global__ __launch_bounds__(kBwdBlock) void add_layer_norm_bwd_kernel(const float *__restrict__ dy, const float *__restrict__ ds,
                                                                       const float *__restrict__ s, const float *__restrict__ mean,
                                                                       const float *__restrict__ rstd, const float *__restrict__ gamma,
                                                                       float *__restrict__ d_s, float *__restrict__ d_gamma,
                                                                       float *__restrict__ d_beta, double *__restrict__ partials,
                                                                       int64_t B, int H) {
    __shared__ double columns[2 * CUSRL_MAX_LAYER_NORM_WIDTH];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    float w[kChunks][4];
    load_row<kChunks, kVec>(gamma, H, lane, w);
    double acc_gamma[kChunks][4], acc_beta[kChunks][4];
#pragma unroll
    for (int k = 0; k < kChunks; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc_gamma[k][j] = acc_beta[k][j] = 0.0;

    const int64_t stride = int64_t(gridDim.x) * kBwdWaves;
    for (int64_t row = int64_t(blockIdx.x) * kBwdWaves + wave; row < B; row += stride) {  // ascending rows: a fixed order
        const int64_t base = row * H;
        float g[kChunks][4], xhat[kChunks][4];
        load_row<kChunks, kVec>(dy + base, H, lane, g);
        load_row<kChunks, kVec>(s + base, H, lane, xhat);
        const float m = mean[row], rs = rstd[row];
        double sum_g = 0.0, sum_gx = 0.0;
#pragma unroll
        for (int k = 0; k < kChunks; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool inside = (lane + kWave * k) * 4 + j < H;
                xhat[k][j] = inside ? (xhat[k][j] - m) * rs : 0.f;
                acc_gamma[k][j] += double(g[k][j]) * double(xhat[k][j]);
                acc_beta[k][j] += double(g[k][j]);
                g[k][j] = g[k][j] * w[k][j];
                sum_g += double(g[k][j]);
                sum_gx += double(g[k][j]) * double(xhat[k][j]);
            }
        const float c1 = float(wave_total(sum_g) / double(H)), c2 = float(wave_total(sum_gx) / double(H));
#pragma unroll
        for (int k = 0; k < kChunks; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) g[k][j] = (g[k][j] - c1 - xhat[k][j] * c2) * rs;
        if (ds != nullptr) {
            load_row<kChunks, kVec>(ds + base, H, lane, xhat);
#pragma unroll
            for (int k = 0; k < kChunks; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) g[k][j] = g[k][j] + xhat[k][j];
        }
        store_row<kChunks, kVec>(d_s + base, H, lane, g);
    }

    // the block's column sums: wave 0 lays its sums down, waves 1 .. 7 add theirs in turn
    for (int turn = 0; turn < kBwdWaves; ++turn) {
        if (wave == turn) {
#pragma unroll
            for (int k = 0; k < kChunks; ++k)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = (lane + kWave * k) * 4 + j;
                    if (c < H) {
                        columns[c] = turn == 0 ? acc_gamma[k][j] : columns[c] + acc_gamma[k][j];
                        columns[H + c] = turn == 0 ? acc_beta[k][j] : columns[H + c] + acc_beta[k][j];
                    }
                }
        }
        __syncthreads();
    }
    if (gridDim.x == 1) {
        for (int c = threadIdx.x; c < H; c += kBwdBlock) d_gamma[c] = float(columns[c]), d_beta[c] = float(columns[H + c]);
    } else {
        double *out = partials + int64_t(blockIdx.x) * 2 * H;
        for (int c = threadIdx.x; c < 2 * H; c += kBwdBlock) out[c] = columns[c];
    }
}

// One block: thread t sums columns t, t + kBlock, ... of the `blocks` partial rows [2 H] in row order.
__global__ __launch_bounds__(kBlock) void add_layer_norm_finalize_kernel(const double *__restrict__ partials, int blocks, int H,
                                                                         float *__restrict__ d_gamma, float *__restrict__ d_beta) {
    for (int c = threadIdx.x; c < 2 * H; c += kBlock) {
        double total = 0.0;
#pragma unroll 8
        for (int b = 0; b < blocks; ++b) total += partials[int64_t(b) * 2 * H + c];
        if (c < H) d_gamma[c] = float(total);
        else d_beta[c - H] = float(total);
    }
}

inline int64_t bwd_blocks(int64_t B) {
    const int64_t want = ceil_div(B, int64_t(kBwdWaves) * kBwdRowsPerWave);
    return want < 1 ? 1 : want > kBwdMaxBlocks ? kBwdMaxBlocks : want;
}

inline int chunks_per_lane(int64_t H) { return int(ceil_div(ceil_div(H, 4), kWave)); }

template <typename... P>
inline bool all_aligned16(P... p) { return (aligned(p, 16) && ...); }

}  // namespace
}  // namespace cusrl

using namespace cusrl;

// (one instantiation per chunk count and access width; `call` receives the kernel)
#define CUSRL_LN_DISPATCH(kernel, chunks, vec, ...)                                                   \
    switch ((chunks) * 2 + ((vec) ? 1 : 0)) {                                                         \
        case 2: { auto fn = kernel<1, false>; __VA_ARGS__; } break;                                    \
        case 3: { auto fn = kernel<1, true>; __VA_ARGS__; } break;                                     \
        case 4: { auto fn = kernel<2, false>; __VA_ARGS__; } break;                                    \
        case 5: { auto fn = kernel<2, true>; __VA_ARGS__; } break;                                     \
        case 6: { auto fn = kernel<3, false>; __VA_ARGS__; } break;                                    \
        case 7: { auto fn = kernel<3, true>; __VA_ARGS__; } break;                                     \
        case 8: { auto fn = kernel<4, false>; __VA_ARGS__; } break;                                    \
        default: { auto fn = kernel<4, true>; __VA_ARGS__; } break;                                    \
    }

extern "C" int cusrl_add_layer_norm_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float eps,
                                        float *sum_out, float *y, float *mean, float *rstd, int64_t B, int64_t H, void *stream) {
    if (B < 0 || H < 0 || !x || !gamma || !beta || !y || (residual && !sum_out) || (mean == nullptr) != (rstd == nullptr))
        return CUSRL_E_INVALID;
    if (H < 1 || H > CUSRL_MAX_LAYER_NORM_WIDTH || ceil_div(B, kWavesPerBlock) > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    if (B == 0) return 0;
    const bool vec = H % 4 == 0 && all_aligned16(x, residual, gamma, beta, sum_out, y);
    const dim3 grid(uint32_t(ceil_div(B, kWavesPerBlock)));
    CUSRL_LN_DISPATCH(add_layer_norm_fwd_kernel, chunks_per_lane(H), vec,
                      hipLaunchKernelGGL(fn, grid, dim3(kBlock), 0, as_stream(stream), x, residual, gamma, beta, eps, sum_out, y, mean,
                                         rstd, B, int(H)))
    return launch_status();
}

extern "C" int64_t cusrl_add_layer_norm_num_partials(int64_t B, int64_t H) {
    if (B <= 0 || H <= 0) return 0;
    const int64_t blocks = bwd_blocks(B);
    return blocks == 1 ? 0 : blocks * 2 * H;
}

extern "C" int cusrl_add_layer_norm_bwd(const float *dy, const float *ds, const float *s, const float *mean, const float *rstd,
                                        const float *gamma, float *d_s, float *d_gamma, float *d_beta, double *partials, int64_t B,
                                        int64_t H, void *stream) {
    if (B < 0 || H < 0 || !dy || !s || !mean || !rstd || !gamma || !d_s || !d_gamma || !d_beta) return CUSRL_E_INVALID;
    if (H < 1 || H > CUSRL_MAX_LAYER_NORM_WIDTH) return CUSRL_E_UNSUPPORTED;
    if (B == 0) return 0;
    const int64_t blocks = bwd_blocks(B);
    if (blocks > 1 && !partials) return CUSRL_E_INVALID;
    const bool vec = H % 4 == 0 && all_aligned16(dy, ds, s, gamma, d_s);
    hipStream_t q = as_stream(stream);
    CUSRL_LN_DISPATCH(add_layer_norm_bwd_kernel, chunks_per_lane(H), vec,
                      hipLaunchKernelGGL(fn, dim3(uint32_t(blocks)), dim3(kBwdBlock), 0, q, dy, ds, s, mean, rstd, gamma, d_s, d_gamma,
                                         d_beta, partials, B, int(H)))
    if (int rc = launch_status()) return rc;
    if (blocks == 1) return 0;  // the one block finished its column sums itself
    hipLaunchKernelGGL(add_layer_norm_finalize_kernel, dim3(1), dim3(kBlock), 0, q, partials, int(blocks), int(H), d_gamma, d_beta);
    return launch_status();
}
