// Scaled dot-product attention, forward and backward, dense and causal sliding-window ("band"), and the rotary embedding
// ("Attention" and "Causal sliding-window attention"): what cusrl/nn/layer/mha.py hands to
// F.scaled_dot_product_attention, what cusrl/nn/module/causal_attn.py:135-258 hands to flex_attention, and
// cusrl/nn/layer/encoding.py:112-125, with the scores never written to memory.  Formulas, layouts and error codes:
// include/cusrl_hip.h.
//
// Three kernel bodies — forward, query-major dQ + delta, key-major dK / dV — each written once over <kWidth, Visibility>.
// Visibility is what differs between the dense and the band entries and nothing else does: the score of a (query, key) pair or
// -inf (Mask: keep-mask, bias or top-left causal; Band: the window, key validity, segments, ALiBi), and which tiles of the
// streamed side can hold a visible entry at all.  One host launcher per pass, templated the same way, builds grid, block and
// LDS size and picks kWidth.  The band's Lq == 1 step has a kernel of its own (no LDS, one wave per block) on the same
// softmax_step.
//
// One body shape for the three kernels.  A workgroup of 256 threads owns kOwn = 16 rows of one (batch, head) and
// streams the other side in tiles of kTile = 32; 16 lanes share a row.  Per tile: (a) lane g of row r computes the scores of
// r against tile entries g and g + 16 as ordered fmaf chains over the head dimension out of LDS, (b) the row's statistics go
// round its 16 lanes by xor shuffles, (c) the probabilities (or dS) cross LDS once, (d) lane g accumulates columns g, g + 16,
// ... of the row's output as ordered fmaf chains over the tile.  Rows are queries in the forward and in the dQ pass (keys
// stream), keys in the dK / dV pass (queries stream): every output element has exactly one owner, which adds its terms in
// index order — no atomics, no sums across workgroups, the same bits on every call.  The products are VALU fmaf chains, not
// MFMA: the tiles a 16-lane row group needs are narrower than an MFMA fragment, and the layers this serves are short
// sequences of small heads.
//
// LDS rows are padded to an odd stride (head_dim | 1): lanes that walk different rows at one column hit different banks.
// The region is dynamic and nothing static sits in front of it.
#include <math.h>

#include <initializer_list>
#include <type_traits>

#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kOwn = 16;    // rows a workgroup owns
constexpr int kTile = 32;   // rows of the streamed side per step
constexpr int kGroup = 16;  // lanes per owned row (kOwn * kGroup == kBlock)
constexpr int kPerLane = kTile / kGroup;                    // scores per lane and tile
constexpr int kAcc = CUSRL_MAX_SDPA_HEAD_DIM / kGroup;      // output columns per lane
constexpr int64_t kSdpaMaxBlocks = 1 << 16;                 // the grid strides over what is left
static_assert(kOwn * kGroup == kBlock, "one lane group per owned row");

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

// The two visibilities.  score(): the score of query i < Lq against key j < Lk, or -inf where i must not see j.  keys(): the
// key tiles that can hold a key visible to a query of q0 ... q0 + kOwn - 1; queries(): the query tiles that can hold a query
// that sees a key of j0 ... j0 + kOwn - 1.  Every (i, j) outside those spans scores -inf.  kSkipsKeys: whether the key-major
// pass may be told to start behind key 0 (its key_from); where it may not, key_from is the constant 0 in the kernel.

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

__device__ __forceinline__ float group_max(float v) {
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kGroup));
    return v;
}

__device__ __forceinline__ float group_sum(float v) {  // (a + b on both partners: every lane ends with the same bits)
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kGroup);
    return v;
}

// `rows` rows of a tensor starting at l0 into dst[r * ld + c]; rows at or past L are zeros.
template <int kWidth>
__device__ __forceinline__ void load_rows(float *dst, int ld, const Rows &t, int64_t n, int64_t h, int64_t l0, int rows, int64_t L,
                                          int D) {
    const int per_row = D / kWidth;
    const float *base = t.p + n * t.sn + h * D;
    for (int i = threadIdx.x; i < rows * per_row; i += kBlock) {
        const int r = i / per_row, c = (i - r * per_row) * kWidth;
        float v[kWidth];
#pragma unroll
        for (int k = 0; k < kWidth; ++k) v[k] = 0.0f;
        if (l0 + r < L) {
            const float *src = base + (l0 + r) * t.sl + c;
            if constexpr (kWidth == 4) {
                const float4 q = *reinterpret_cast<const float4 *>(src);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            } else {
                v[0] = *src;
            }
        }
#pragma unroll
        for (int k = 0; k < kWidth; ++k) dst[r * ld + c + k] = v[k];
    }
}

__device__ __forceinline__ float dot(const float *a, const float *b, int D) {
    float s = 0.0f;
    for (int d = 0; d < D; ++d) s = fmaf(a[d], b[d], s);
    return s;
}

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

// Store a lane's output columns of one owned row: dst row `row` of a contiguous [N, L, H, D] tensor.
__device__ __forceinline__ void store_columns(float *dst, const float (&acc)[kAcc], int g, int D) {
#pragma unroll
    for (int e = 0; e < kAcc; ++e)
        if (g + e * kGroup < D) dst[g + e * kGroup] = acc[e];
}

// ------------------------------------------------------------------------------------------------------------ forward
template <int kWidth, typename Visibility>
__global__ __launch_bounds__(kBlock) void sdpa_fwd_kernel(Rows q, Rows k, Rows v, Visibility vis, float *out, float *lse, Shape s,
                                                          int64_t q_tiles, int64_t items) {
    extern __shared__ float lds[];
    const int D = s.D, ld = D | 1;
    float *sq = lds, *sk = sq + kOwn * ld, *sv = sk + kTile * ld, *sp = sv + kTile * ld;  // sp: [kOwn][kTile]
    const int r = threadIdx.x / kGroup, g = threadIdx.x % kGroup;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kOwn, i = q0 + r;
        load_rows<kWidth>(sq, ld, q, n, h, q0, kOwn, s.Lq, D);
        float m = -INFINITY, l = 0.0f, acc[kAcc];
#pragma unroll
        for (int e = 0; e < kAcc; ++e) acc[e] = 0.0f;
        const Span keys = vis.keys(q0, s);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kTile) {
            __syncthreads();  // the previous tile's readers are done (and sq is not being written over a reader)
            load_rows<kWidth>(sk, ld, k, n, h, k0, kTile, s.Lk, D);
            load_rows<kWidth>(sv, ld, v, n, h, k0, kTile, s.Lk, D);
            __syncthreads();
            float score[kPerLane], top = -INFINITY;
#pragma unroll
            for (int c = 0; c < kPerLane; ++c) {
                const int64_t j = k0 + g + c * kGroup;
                score[c] = (i < s.Lq && j < s.Lk) ? vis.score(dot(sq + r * ld, sk + (g + c * kGroup) * ld, D), s.scale, n, h, i, j, s.Lq)
                                                  : -INFINITY;
                top = fmaxf(top, score[c]);
            }
            const float alpha = softmax_step(m, group_max(top), score);
            float part = 0.0f;
#pragma unroll
            for (int c = 0; c < kPerLane; ++c) {
                sp[r * kTile + g + c * kGroup] = score[c];
                part += score[c];
            }
            l = l * alpha + group_sum(part);
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kAcc; ++e) {
                const int d = g + e * kGroup;
                if (d < D) {
                    float a = acc[e] * alpha;
                    for (int j = 0; j < kTile; ++j) a = fmaf(sp[r * kTile + j], sv[j * ld + d], a);
                    acc[e] = a;
                }
            }
        }
        if (i < s.Lq) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // a row with no visible key: zeros and lse = -inf
#pragma unroll
            for (int e = 0; e < kAcc; ++e) acc[e] = acc[e] * inv;
            store_columns(out + ((n * s.Lq + i) * s.H + h) * D, acc, g, D);
            if (g == 0) lse[(n * s.H + h) * s.Lq + i] = l > 0.0f ? m + logf(l) : -INFINITY;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------- backward, query-major: dQ
// Owns 16 queries; also lays down delta[n, h, i] = sum_d dout * out for the key-major pass that follows on the stream.
template <int kWidth, typename Visibility>
__global__ __launch_bounds__(kBlock) void sdpa_bwd_dq_kernel(Rows q, Rows k, Rows v, Rows o, Rows dout, const float *lse, Visibility vis,
                                                             float *dq, float *delta, Shape s, int64_t q_tiles, int64_t items) {
    extern __shared__ float lds[];
    const int D = s.D, ld = D | 1;
    float *sq = lds, *sdo = sq + kOwn * ld, *sk = sdo + kOwn * ld, *sv = sk + kTile * ld, *sds = sv + kTile * ld;  // sds: [kOwn][kTile]
    const int r = threadIdx.x / kGroup, g = threadIdx.x % kGroup;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kOwn, i = q0 + r;
        load_rows<kWidth>(sq, ld, q, n, h, q0, kOwn, s.Lq, D);
        load_rows<kWidth>(sdo, ld, dout, n, h, q0, kOwn, s.Lq, D);
        load_rows<kWidth>(sk, ld, o, n, h, q0, kOwn, s.Lq, D);  // (out passes through the key tile's place once)
        __syncthreads();
        float part = 0.0f;
        for (int d = g; d < D; d += kGroup) part = fmaf(sdo[r * ld + d], sk[r * ld + d], part);
        const float row_delta = group_sum(part);
        const float row_lse = i < s.Lq ? lse[(n * s.H + h) * s.Lq + i] : -INFINITY;
        if (i < s.Lq && g == 0) delta[(n * s.H + h) * s.Lq + i] = row_delta;
        float acc[kAcc];
#pragma unroll
        for (int e = 0; e < kAcc; ++e) acc[e] = 0.0f;
        const Span keys = vis.keys(q0, s);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kTile) {
            __syncthreads();
            load_rows<kWidth>(sk, ld, k, n, h, k0, kTile, s.Lk, D);
            load_rows<kWidth>(sv, ld, v, n, h, k0, kTile, s.Lk, D);
            __syncthreads();
#pragma unroll
            for (int c = 0; c < kPerLane; ++c) {
                const int t = g + c * kGroup;
                const int64_t j = k0 + t;
                float ds = 0.0f;
                if (i < s.Lq && j < s.Lk) {
                    const float sc = vis.score(dot(sq + r * ld, sk + t * ld, D), s.scale, n, h, i, j, s.Lq);
                    const float p = probability(sc, row_lse);
                    if (p != 0.0f) ds = p * (dot(sdo + r * ld, sv + t * ld, D) - row_delta) * s.scale;
                }
                sds[r * kTile + t] = ds;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kAcc; ++e) {
                const int d = g + e * kGroup;
                if (d < D) {
                    float a = acc[e];
                    for (int j = 0; j < kTile; ++j) a = fmaf(sds[r * kTile + j], sk[j * ld + d], a);
                    acc[e] = a;
                }
            }
        }
        if (i < s.Lq) store_columns(dq + ((n * s.Lq + i) * s.H + h) * D, acc, g, D);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------- backward, key-major: dK and dV
// Owns keys j0 ... j0 + 15 with j0 = key_from + 16 * tile and streams the queries with their dout, lse and delta: the keys in
// front of key_from are not visited, and dk / dv [N, Lk - key_from, H, D] hold rows j - key_from.
template <int kWidth, typename Visibility>
__global__ __launch_bounds__(kBlock) void sdpa_bwd_dkv_kernel(Rows q, Rows k, Rows v, Rows dout, const float *lse, const float *delta,
                                                              Visibility vis, float *dk, float *dv, Shape s, int64_t key_from,
                                                              int64_t k_tiles, int64_t items) {
    extern __shared__ float lds[];
    const int D = s.D, ld = D | 1;
    float *sk = lds, *sv = sk + kOwn * ld, *sq = sv + kOwn * ld, *sdo = sq + kTile * ld;
    float *sp = sdo + kTile * ld, *sds = sp + kOwn * kTile, *slse = sds + kOwn * kTile, *sdelta = slse + kTile;  // sp, sds: [kOwn][kTile]
    const int r = threadIdx.x / kGroup, g = threadIdx.x % kGroup;
    if (!Visibility::kSkipsKeys) key_from = 0;  // (known when the kernel is compiled: the dense pass pays nothing for the offset)
    const int64_t rows_out = s.Lk - key_from;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item % k_tiles, nh = item / k_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t j0 = key_from + tile * kOwn, j = j0 + r;
        load_rows<kWidth>(sk, ld, k, n, h, j0, kOwn, s.Lk, D);
        load_rows<kWidth>(sv, ld, v, n, h, j0, kOwn, s.Lk, D);
        float acc_k[kAcc], acc_v[kAcc];
#pragma unroll
        for (int e = 0; e < kAcc; ++e) acc_k[e] = acc_v[e] = 0.0f;
        const Span queries = vis.queries(j0, s);
        for (int64_t q0 = queries.begin; q0 < queries.end; q0 += kTile) {
            __syncthreads();
            load_rows<kWidth>(sq, ld, q, n, h, q0, kTile, s.Lq, D);
            load_rows<kWidth>(sdo, ld, dout, n, h, q0, kTile, s.Lq, D);
            if (threadIdx.x < kTile) {
                const int64_t i = q0 + threadIdx.x;
                slse[threadIdx.x] = i < s.Lq ? lse[(n * s.H + h) * s.Lq + i] : -INFINITY;
                sdelta[threadIdx.x] = i < s.Lq ? delta[(n * s.H + h) * s.Lq + i] : 0.0f;
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < kPerLane; ++c) {
                const int t = g + c * kGroup;
                const int64_t i = q0 + t;
                float p = 0.0f, ds = 0.0f;
                if (i < s.Lq && j < s.Lk) {
                    const float sc = vis.score(dot(sq + t * ld, sk + r * ld, D), s.scale, n, h, i, j, s.Lq);
                    p = probability(sc, slse[t]);
                    if (p != 0.0f) ds = p * (dot(sdo + t * ld, sv + r * ld, D) - sdelta[t]) * s.scale;
                }
                sp[r * kTile + t] = p;
                sds[r * kTile + t] = ds;
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kAcc; ++e) {
                const int d = g + e * kGroup;
                if (d < D) {
                    float a = acc_v[e], b = acc_k[e];
                    for (int t = 0; t < kTile; ++t) {
                        a = fmaf(sp[r * kTile + t], sdo[t * ld + d], a);
                        b = fmaf(sds[r * kTile + t], sq[t * ld + d], b);
                    }
                    acc_v[e] = a, acc_k[e] = b;
                }
            }
        }
        if (j < s.Lk) {
            store_columns(dk + ((n * rows_out + (j - key_from)) * s.H + h) * D, acc_k, g, D);
            store_columns(dv + ((n * rows_out + (j - key_from)) * s.H + h) * D, acc_v, g, D);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ forward of the band, Lq == 1
// The step of a rollout: one query per (n, h) and W + 1 candidate keys, each read once, so nothing goes through LDS.  One
// 16-lane group per (n, h): lane g scores key c0 + g of a chunk of 16 straight from global memory (its own K row, kWidth
// floats per load), the statistics go round the group, and lane g accumulates columns g, g + 16, ... of the output over the
// chunk's V rows (a row's columns are adjacent lanes: coalesced).  A block is one wave of four groups: it has no barrier and
// no LDS, and a small batch spreads over four times the compute units a 256-thread block would reach.
constexpr int kStepBlock = 64;
constexpr int kStepGroups = kStepBlock / kGroup;

template <int kWidth>
__global__ __launch_bounds__(kStepBlock) void band_step_kernel(Rows q, Rows k, Rows v, Band band, float *out, float *lse, Shape s, int64_t items) {
    const int r = threadIdx.x / kGroup, g = threadIdx.x % kGroup;
    const int D = s.D;
    for (int64_t nh = int64_t(blockIdx.x) * kStepGroups + r; nh < items; nh += int64_t(gridDim.x) * kStepGroups) {
        const int64_t h = nh % s.H, n = nh / s.H;
        const float *q_row = q.p + n * q.sn + h * D, *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        float m = -INFINITY, l = 0.0f, acc[kAcc];
#pragma unroll
        for (int e = 0; e < kAcc; ++e) acc[e] = 0.0f;
        for (int64_t c0 = 0; c0 < s.Lk; c0 += kGroup) {  // (Lk = W + 1: every key is a candidate of the one query)
            const int64_t j = c0 + g;
            float score = -INFINITY;
            if (j < s.Lk) {
                const float *k_row = k_base + j * k.sl;
                float qk = 0.0f;
                if constexpr (kWidth == 4) {
                    for (int d = 0; d < D; d += 4) {
                        const float4 a = *reinterpret_cast<const float4 *>(q_row + d), b = *reinterpret_cast<const float4 *>(k_row + d);
                        qk = fmaf(a.x, b.x, qk), qk = fmaf(a.y, b.y, qk), qk = fmaf(a.z, b.z, qk), qk = fmaf(a.w, b.w, qk);
                    }
                } else {
                    qk = dot(q_row, k_row, D);
                }
                score = band.score(qk, s.scale, n, h, 0, j, 1);
            }
            float weight[1] = {score};
            const float alpha = softmax_step(m, group_max(score), weight), p = weight[0];
            l = l * alpha + group_sum(p);
#pragma unroll
            for (int e = 0; e < kAcc; ++e) acc[e] = acc[e] * alpha;
            for (int t = 0; t < kGroup; ++t) {
                const float pt = __shfl(p, t, kGroup);  // (every lane of the group takes part; the loads below are guarded)
                if (c0 + t < s.Lk) {
                    const float *v_row = v_base + (c0 + t) * v.sl;
#pragma unroll
                    for (int e = 0; e < kAcc; ++e)
                        if (g + e * kGroup < D) acc[e] = fmaf(pt, v_row[g + e * kGroup], acc[e]);
                }
            }
        }
        const float inv = l > 0.0f ? 1.0f / l : 0.0f;
#pragma unroll
        for (int e = 0; e < kAcc; ++e) acc[e] = acc[e] * inv;
        store_columns(out + nh * D, acc, g, D);
        if (g == 0) lse[nh] = l > 0.0f ? m + logf(l) : -INFINITY;
    }
}

// --------------------------------------------------------------------------------------------------------------- host
bool rows_vectorise(std::initializer_list<Rows> tensors, int D) {  // 16-byte loads: every row of every tensor starts on one
    for (const Rows &t : tensors)
        if (!aligned(t.p, 16) || t.sn % 4 || t.sl % 4) return false;
    return D % 4 == 0;
}

// launch(width) with the kernels' kWidth as a compile-time constant: 4 where the operands vectorise, else 1.
template <typename Launch>
void with_width(bool vec, Launch launch) {
    if (vec)
        launch(std::integral_constant<int, 4>{});
    else
        launch(std::integral_constant<int, 1>{});
}

bool sizes_fit(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {  // every contiguous extent within int64
    const int64_t L = Lq > Lk ? Lq : Lk;
    if (H > INT64_MAX / D) return false;
    if (L > INT64_MAX / (H * D)) return false;
    return N == 0 || L * H * D <= INT64_MAX / N;
}

uint32_t grid_for(int64_t items) { return uint32_t(items < kSdpaMaxBlocks ? items : kSdpaMaxBlocks); }

size_t lds_bytes(int rows, int extra, int D) { return (size_t(rows) * (D | 1) + extra) * sizeof(float); }

bool valid_sizes(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {
    return N >= 0 && H >= 1 && Lq >= 1 && Lk >= 1 && D >= 1 && D <= CUSRL_MAX_SDPA_HEAD_DIM;
}

bool valid_band_sizes(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D) {
    return N >= 0 && H >= 1 && Lq >= 1 && W >= 1 && D >= 1 && D <= CUSRL_MAX_SDPA_HEAD_DIM;
}

bool band_sizes_fit(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D) {
    return W <= INT64_MAX - Lq && sizes_fit(N, H, Lq, Lq + W, D);
}

// The launchers take validated sizes with N >= 1 and return the entry's status.
template <typename Visibility>
int launch_fwd(const Rows &q, const Rows &k, const Rows &v, const Visibility &vis, float *out, float *lse, const Shape &s, void *stream) {
    const int64_t q_tiles = ceil_div(s.Lq, kOwn);
    if (s.N * s.H > INT64_MAX / q_tiles) return CUSRL_E_UNSUPPORTED;
    const int64_t items = s.N * s.H * q_tiles;
    const dim3 grid{grid_for(items)}, block{kBlock};
    const size_t lds = lds_bytes(kOwn + 2 * kTile, kOwn * kTile, s.D);
    with_width(rows_vectorise({q, k, v}, s.D), [&](auto width) {
        hipLaunchKernelGGL((sdpa_fwd_kernel<decltype(width)::value, Visibility>), grid, block, lds, as_stream(stream), q, k, v, vis, out, lse,
                           s, q_tiles, items);
    });
    return launch_status();
}

int launch_step(const Rows &q, const Rows &k, const Rows &v, const Band &band, float *out, float *lse, const Shape &s, void *stream) {
    const int64_t items = s.N * s.H;  // one 16-lane group per (n, h)
    const dim3 grid{grid_for(ceil_div(items, int64_t(kStepGroups)))}, block{kStepBlock};
    with_width(rows_vectorise({q, k, v}, s.D), [&](auto width) {
        hipLaunchKernelGGL((band_step_kernel<decltype(width)::value>), grid, block, 0, as_stream(stream), q, k, v, band, out, lse, s, items);
    });
    return launch_status();
}

// The backward: the query-major pass lays dq and delta down, the key-major pass that follows on the stream reads delta and owns
// dk / dv [N, Lk - key_from, H, D].
template <typename Visibility>
int launch_bwd(const Rows &q, const Rows &k, const Rows &v, const Rows &o, const Rows &dout, const float *lse, const Visibility &vis,
               float *dq, float *dk, float *dv, float *delta, const Shape &s, int64_t key_from, void *stream) {
    const int64_t q_tiles = ceil_div(s.Lq, kOwn), k_tiles = ceil_div(s.Lk - key_from, kOwn);
    if (s.N * s.H > INT64_MAX / q_tiles || s.N * s.H > INT64_MAX / k_tiles) return CUSRL_E_UNSUPPORTED;
    const bool vec = rows_vectorise({q, k, v, o, dout}, s.D);
    const dim3 block{kBlock};
    with_width(vec, [&](auto width) {
        const int64_t items = s.N * s.H * q_tiles;
        const size_t lds = lds_bytes(2 * kOwn + 2 * kTile, kOwn * kTile, s.D);
        hipLaunchKernelGGL((sdpa_bwd_dq_kernel<decltype(width)::value, Visibility>), dim3{grid_for(items)}, block, lds, as_stream(stream), q,
                           k, v, o, dout, lse, vis, dq, delta, s, q_tiles, items);
    });
    if (const int status = launch_status()) return status;
    with_width(vec, [&](auto width) {
        const int64_t items = s.N * s.H * k_tiles;
        const size_t lds = lds_bytes(2 * kOwn + 2 * kTile, 2 * kOwn * kTile + 2 * kTile, s.D);
        hipLaunchKernelGGL((sdpa_bwd_dkv_kernel<decltype(width)::value, Visibility>), dim3{grid_for(items)}, block, lds, as_stream(stream),
                           q, k, v, dout, lse, delta, vis, dk, dv, s, key_from, k_tiles, items);
    });
    return launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- RoPE
// One lane per kWidth adjacent pairs (x[d], x[d + D / 2]) of one (n, l, h).
template <int kWidth, bool kTranspose>
__global__ __launch_bounds__(kBlock) void rope_kernel(const float *x, int64_t sn, int64_t sl, const float *cos_rows, const float *sin_rows,
                                                      float *out, int64_t L, int64_t H, int half, int64_t lanes) {
    const int per_head = half / kWidth;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t at = int64_t(blockIdx.x) * kBlock + threadIdx.x; at < lanes; at += stride) {
        const int c = int(at % per_head) * kWidth;
        const int64_t nlh = at / per_head, h = nlh % H, nl = nlh / H, l = nl % L, n = nl / L;
        const float *src = x + n * sn + l * sl + h * (2 * half) + c;
        float *dst = out + nlh * (2 * half) + c;
        float a[kWidth], b[kWidth], co[kWidth], si[kWidth];
        if constexpr (kWidth == 4) {
            const float4 va = *reinterpret_cast<const float4 *>(src), vb = *reinterpret_cast<const float4 *>(src + half);
            const float4 vc = *reinterpret_cast<const float4 *>(cos_rows + l * half + c), vs = *reinterpret_cast<const float4 *>(sin_rows + l * half + c);
            a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w, b[0] = vb.x, b[1] = vb.y, b[2] = vb.z, b[3] = vb.w;
            co[0] = vc.x, co[1] = vc.y, co[2] = vc.z, co[3] = vc.w, si[0] = vs.x, si[1] = vs.y, si[2] = vs.z, si[3] = vs.w;
        } else {
            a[0] = src[0], b[0] = src[half], co[0] = cos_rows[l * half + c], si[0] = sin_rows[l * half + c];
        }
        float first[kWidth], second[kWidth];
#pragma unroll
        for (int k = 0; k < kWidth; ++k) {
            if (kTranspose) {
                first[k] = a[k] * co[k] + b[k] * si[k];
                second[k] = b[k] * co[k] - a[k] * si[k];
            } else {
                first[k] = a[k] * co[k] + (-b[k]) * si[k];  // x cos + rotate_half(x) sin, as the reference rounds it
                second[k] = b[k] * co[k] + a[k] * si[k];
            }
        }
        if constexpr (kWidth == 4) {
            *reinterpret_cast<float4 *>(dst) = make_float4(first[0], first[1], first[2], first[3]);
            *reinterpret_cast<float4 *>(dst + half) = make_float4(second[0], second[1], second[2], second[3]);
        } else {
            dst[0] = first[0], dst[half] = second[0];
        }
    }
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_sdpa_fwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                              int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *keep_mask,
                              const float *bias, int64_t mask_stride_n, int64_t mask_stride_h, int64_t mask_stride_q,
                              int64_t mask_stride_k, int causal, float scale, float *out, float *lse, int64_t N, int64_t H, int64_t Lq,
                              int64_t Lk, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || (keep_mask && bias) || !valid_sizes(N, H, Lq, Lk, D)) return CUSRL_E_INVALID;
    if (!sizes_fit(N, H, Lq, Lk, D)) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Mask mask{keep_mask, bias, mask_stride_n, mask_stride_h, mask_stride_q, mask_stride_k, causal != 0};
    const Shape shape{N, H, Lq, Lk, int(D), scale};
    return launch_fwd(rq, rk, rv, mask, out, lse, shape, stream);
}

extern "C" int64_t cusrl_sdpa_bwd_workspace(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D) {
    if (!valid_sizes(N, H, Lq, Lk, D) || !sizes_fit(N, H, Lq, Lk, D)) return -1;
    return N * H * Lq;  // delta, one fp32 per query row and head
}

extern "C" int cusrl_sdpa_bwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                              int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const float *out,
                              const float *lse, const float *dout, int64_t dout_stride_n, int64_t dout_stride_l,
                              const uint8_t *keep_mask, const float *bias, int64_t mask_stride_n, int64_t mask_stride_h,
                              int64_t mask_stride_q, int64_t mask_stride_k, int causal, float scale, float *dq, float *dk, float *dv,
                              float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || (keep_mask && bias) || !valid_sizes(N, H, Lq, Lk, D))
        return CUSRL_E_INVALID;
    if (!sizes_fit(N, H, Lq, Lk, D)) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!workspace) return CUSRL_E_INVALID;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Rows ro{out, Lq * H * D, H * D}, rdo{dout, dout_stride_n, dout_stride_l};
    const Mask mask{keep_mask, bias, mask_stride_n, mask_stride_h, mask_stride_q, mask_stride_k, causal != 0};
    const Shape shape{N, H, Lq, Lk, int(D), scale};
    return launch_bwd(rq, rk, rv, ro, rdo, lse, mask, dq, dk, dv, workspace, shape, 0, stream);
}

extern "C" int cusrl_rope_apply(const float *x, int64_t x_stride_n, int64_t x_stride_l, const float *cos_rows, const float *sin_rows,
                                float *out, int64_t N, int64_t L, int64_t H, int64_t D, int transpose, void *stream) {
    if (!x || !cos_rows || !sin_rows || !out || N < 0 || L < 1 || H < 1 || D < 2 || D % 2 || (transpose != 0 && transpose != 1))
        return CUSRL_E_INVALID;
    if (D > INT32_MAX || !sizes_fit(N, H, L, L, D)) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const int half = int(D / 2);
    const bool vec = half % 4 == 0 && aligned(x, 16) && aligned(cos_rows, 16) && aligned(sin_rows, 16) && aligned(out, 16) &&
                     x_stride_n % 4 == 0 && x_stride_l % 4 == 0;
    const int64_t lanes = N * L * H * (half / (vec ? 4 : 1));
    int64_t blocks = ceil_div(lanes, kBlock);
    if (blocks > 2048) blocks = 2048;
    const dim3 grid{uint32_t(blocks)}, block{kBlock};
#define CUSRL_ROPE_LAUNCH(W, T) \
    hipLaunchKernelGGL((rope_kernel<W, T>), grid, block, 0, as_stream(stream), x, x_stride_n, x_stride_l, cos_rows, sin_rows, out, L, H, half, lanes)
    if (vec && transpose) CUSRL_ROPE_LAUNCH(4, true);
    else if (vec) CUSRL_ROPE_LAUNCH(4, false);
    else if (transpose) CUSRL_ROPE_LAUNCH(1, true);
    else CUSRL_ROPE_LAUNCH(1, false);
#undef CUSRL_ROPE_LAUNCH
    return launch_status();
}

// ================================================================================================ band (sliding window)
// Causal sliding-window attention ("Causal sliding-window attention"; cusrl/nn/module/causal_attn.py:135-258 with
// cusrl/nn/utils/attention.py:117-124, 158-159 in flex_attention's place): the kernels and launchers above with Band as the
// visibility, so only the tiles the band touches are streamed, plus the step kernel for Lq == 1.  key_grad_from is the
// key-major pass's key_from.
extern "C" int cusrl_band_sdpa_fwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                   int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                                   const int32_t *q_segment, const float *alibi_slopes, float scale, float *out, float *lse, int64_t N,
                                   int64_t H, int64_t Lq, int64_t W, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || !valid_band_sizes(N, H, Lq, W, D)) return CUSRL_E_INVALID;
    if (!band_sizes_fit(N, H, Lq, W, D)) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Band band{key_valid, q_segment, alibi_slopes, W};
    const Shape shape{N, H, Lq, Lq + W, int(D), scale};
    return Lq == 1 ? launch_step(rq, rk, rv, band, out, lse, shape, stream) : launch_fwd(rq, rk, rv, band, out, lse, shape, stream);
}

extern "C" int64_t cusrl_band_sdpa_bwd_workspace(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D) {
    if (!valid_band_sizes(N, H, Lq, W, D) || !band_sizes_fit(N, H, Lq, W, D)) return -1;
    return N * H * Lq;  // delta, one fp32 per query row and head
}

extern "C" int cusrl_band_sdpa_bwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                   int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                                   const int32_t *q_segment, const float *alibi_slopes, float scale, const float *out, const float *lse,
                                   const float *dout, int64_t dout_stride_n, int64_t dout_stride_l, int64_t key_grad_from, float *dq,
                                   float *dk, float *dv, float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D,
                                   void *stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !valid_band_sizes(N, H, Lq, W, D) || key_grad_from < 0 ||
        key_grad_from > W)
        return CUSRL_E_INVALID;
    if (!band_sizes_fit(N, H, Lq, W, D)) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!workspace) return CUSRL_E_INVALID;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Rows ro{out, Lq * H * D, H * D}, rdo{dout, dout_stride_n, dout_stride_l};
    const Band band{key_valid, q_segment, alibi_slopes, W};
    const Shape shape{N, H, Lq, Lq + W, int(D), scale};
    return launch_bwd(rq, rk, rv, ro, rdo, lse, band, dq, dk, dv, workspace, shape, key_grad_from, stream);
}
