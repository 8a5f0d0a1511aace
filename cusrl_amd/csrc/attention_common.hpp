// What the attention translation units share (attention.hip: the VALU bodies; attention_mfma.hip and attention_mfma_bwd.hip: the
// dense fp32-MFMA forward and backward; attention_bf16.hip: the dense forward on bf16 operands, with a `Rows` of its own;
// attention_mfma_band.hip: the band's fp32-MFMA forward): the operand and shape structs, the
// two visibilities `Mask` (dense) and `Band` (sliding window) with the two tile constants their spans are written in, the
// online-softmax step, the backward's `probability`, and the host's size and 16-byte rules.  Moved here from attention.hip as they
// stood; formulas: include/cusrl_hip.h.
#pragma once

#include <math.h>

#include <initializer_list>

#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kOwn = 16;    // rows a workgroup owns
constexpr int kTile = 32;   // rows of the streamed side per step

struct Rows {  // [N, L, H, D] with element (n, l, h, d) at p + n * sn + l * sl + h * D + d
    const float *p;
    int64_t sn, sl;
};

struct Shape {
    int64_t N, H, Lq, Lk;
    int D;
    float scale;
};

struct Span {  // tiles [begin, begin + kTile), ... of the streamed side up to `end`
    int64_t begin, end;
};

struct Mask {  // dense: element strides (n, h, q, k) of the keep-mask or of the bias (at most one of the two is present)
    const uint8_t *keep;
    const float *bias;
    int64_t sn, sh, sq, sk;
    int causal;
    static constexpr bool kSkipsKeys = false;

    // scale * (q . k) + bias
    __device__ __forceinline__ float score(float qk, float scale, int64_t n, int64_t h, int64_t i, int64_t j, int64_t) const {
        if (causal && j > i) return -INFINITY;
        float s = qk * scale;
        if (keep || bias) {
            const int64_t at = n * sn + h * sh + i * sq + j * sk;
            if (keep && !keep[at]) return -INFINITY;
            if (bias) s = s + bias[at];
        }
        return s;
    }
    // (top-left causal: keys past the tile's last query are masked for every row of it)
    __device__ __forceinline__ Span keys(int64_t q0, const Shape &s) const { return {0, causal ? min(s.Lk, q0 + kOwn) : s.Lk}; }
    // (top-left causal: queries in front of the tile's first key see none of its keys)
    __device__ __forceinline__ Span queries(int64_t j0, const Shape &s) const { return {causal ? j0 / kTile * kTile : 0, s.Lq}; }
};

struct Band {  // Lk = Lq + W, the first W keys are the cache, and query i sees keys i ... i + W
    const uint8_t *valid;  // [N, Lq + W] contiguous, nonzero = a key that exists; or NULL
    const int32_t *seg;    // [N, Lq] contiguous segment id of every query; the cache is segment 0; or NULL
    const float *slopes;   // [H] ALiBi slopes; or NULL
    int64_t W;
    static constexpr bool kSkipsKeys = true;  // (the cache keys' gradients are not always wanted: key_grad_from)

    // scale * (q . k) - slope[h] * (i + W - j)
    __device__ __forceinline__ float score(float qk, float scale, int64_t n, int64_t h, int64_t i, int64_t j, int64_t Lq) const {
        if (j < i || j > i + W) return -INFINITY;
        if (valid && !valid[n * (Lq + W) + j]) return -INFINITY;
        if (seg && seg[n * Lq + i] != (j < W ? 0 : seg[n * Lq + j - W])) return -INFINITY;
        const float s = qk * scale;
        return slopes ? fmaf(-slopes[h], float(i + W - j), s) : s;  // (one rounding, the same in all four kernels)
    }
    // (the last query of the tile sees key q0 + kOwn - 1 + W)
    __device__ __forceinline__ Span keys(int64_t q0, const Shape &s) const { return {q0, min(s.Lk, q0 + kOwn + W)}; }
    // (key j is seen by queries j - W ... j)
    __device__ __forceinline__ Span queries(int64_t j0, const Shape &s) const { return {j0 > W ? j0 - W : 0, min(s.Lq, j0 + kOwn)}; }
};

// One step of a row's online softmax: m becomes max(m, top), where top is the largest of the step's scores over the whole row
// group; the scores become exp(score - m) in place (0 for -inf) and the factor that rescales what the row has accumulated
// so far is returned.  A row that has seen no key yet keeps m = -inf, weights of 0 and a factor of 1.
template <int kScores>
__device__ __forceinline__ float softmax_step(float &m, float top, float (&score)[kScores]) {
    const float m_new = fmaxf(m, top);
    float alpha = 1.0f;
    if (m_new != -INFINITY) {
        alpha = (m == -INFINITY) ? 0.0f : expf(m - m_new);
#pragma unroll
        for (int c = 0; c < kScores; ++c) score[c] = (score[c] == -INFINITY) ? 0.0f : expf(score[c] - m_new);
    } else {
#pragma unroll
        for (int c = 0; c < kScores; ++c) score[c] = 0.0f;
    }
    m = m_new;
    return alpha;
}

// exp(s - lse) for a visible score of a row with a visible key, exactly 0 otherwise (never exp(-inf - (-inf))).
__device__ __forceinline__ float probability(float s, float lse) { return (s == -INFINITY || lse == -INFINITY) ? 0.0f : expf(s - lse); }

// --------------------------------------------------------------------------------------------------------------- host
inline bool rows_vectorise(std::initializer_list<Rows> tensors, int D) {  // 16-byte loads: every row of every tensor starts on one
    for (const Rows &t : tensors)
        if (!aligned(t.p, 16) || t.sn % 4 || t.sl % 4) return false;
    return D % 4 == 0;
}

inline bool sizes_fit(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {  // every contiguous extent within int64
    const int64_t L = Lq > Lk ? Lq : Lk;
    if (H > INT64_MAX / D) return false;
    if (L > INT64_MAX / (H * D)) return false;
    return N == 0 || L * H * D <= INT64_MAX / N;
}

inline bool valid_sizes(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {
    return N >= 0 && H >= 1 && Lq >= 1 && Lk >= 1 && D >= 1 && D <= CUSRL_MAX_SDPA_HEAD_DIM;
}

inline bool valid_band_sizes(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D) {
    return N >= 0 && H >= 1 && Lq >= 1 && W >= 1 && D >= 1 && D <= CUSRL_MAX_SDPA_HEAD_DIM;
}

inline bool band_sizes_fit(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D) {
    return W <= INT64_MAX - Lq && sizes_fit(N, H, Lq, Lq + W, D);
}

}  // namespace
}  // namespace cusrl
