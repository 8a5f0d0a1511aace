// ONE no-grad time step of causal sliding-window attention for gfx950 as ONE launch on v_mfma_f32_16x16x4_f32 (DESIGN.md,
// "Attention step on the matrix cores"; formulas: include/cusrl_hip.h, cusrl_attn_step_forward).  At Lq == 1 without RoPE
// everything between a layer's input and its output is linear except the softmax, so the step is attention IN INPUT SPACE: every
// head h of sequence n scores its folded query qf[n, h] (Wk_h^T (Wq_h x_n + bq_h), built by the caller) against the sequence's RAW
// window X_n [W + 1, C] - the W cached inputs, then the new input x_n - and returns ctx[n, h] = sum_j p_j X_j; the value and output
// projections follow as one GEMM on ctx.  The same launch writes the cache and its mask rolled by one step.
//
// Formulation: the band forward's (attention_mfma_band.hip; read its header first) with HEAD m = lane & 15 in place of query
// q0 + m: the H <= 16 heads of ONE sequence are the 16 rows of the MFMA tile, and they all share one key / value operand.  Lane
// (i = m, kk = lane >> 4) supplies A[i][kk] and B[kk][m] and holds D[4 kk + reg][m]:
//   * scores  S^T = X Qf^T of a 16-key sub-tile: the A operands of d-block t are one float4 X[k0 + i][16 t + 4 kk .. + 3], the B
//     operands one float4 of qf[n, m], loaded once per sequence and kept unscaled (zeros for m >= H; nothing is stored for those
//     rows).  Afterwards the lane holds head m against keys k0 + 4 kk + reg; the score is Band::score's expression at i = 0;
//   * online softmax per head through softmax_step as it stands, row maximum and row sum combined with lanes ^ 16 and ^ 32;
//   * ctx^T += X^T P^T: the B operand of MFMA j is the lane's own probability register j, the A operand X[k0 + 4 kk + j][16 t + i];
//     ceil(C / 16) accumulator tiles; lane (m, kk) stores ctx[n, m][16 t + 4 kk .. + 3] as one float4 per tile.
//
// What is new against the band kernel:
//   * ONE key / value tensor for all heads: a sub-tile of X is fetched once per sequence and serves 16 heads in both products, not
//     once per (n, h);
//   * key W comes from x, not from the cache (a per-lane row pointer; keys past W re-read x's row and are selected to zero);
//   * the cache roll rides on the score operands: the float4 a lane loads as X[k0 + i][16 t + 4 kk ..] is the one it stores, as
//     loaded, to cache_out row k0 + i - 1 (keys 1 .. W); the mask bytes the m == 0 lanes load for keys k0 + 4 kk + j go to mask_out
//     likewise.  Never in place: the host refuses outputs that overlap an input.
//
// The transposed operand of P.X re-reads the sub-tile's rows from global memory (4 bytes per lane, 16 lanes on 64 contiguous
// bytes of a row) instead of staging it through LDS: the rows were requested by the same wave one instruction earlier, so the
// re-read is an L1 / L2 hit and adds no HBM traffic, and a wave keeps no LDS and needs no fence between its own lanes (DESIGN.md has
// the numbers).  A hidden key's row is selected to zero there - never multiplied by its zero probability - so NaN in a hidden row
// reaches nothing.  The next sub-tile's loads are issued in front of the current sub-tile's MFMAs.
//
// Work split: ONE WAVE PER SEQUENCE; a workgroup is 4 waves on 4 consecutive sequences and the grid strides over the sequences
// with 64-bit indices.  No __syncthreads(), no LDS, no atomics.
//
// Determinism: one owning lane per output element, a head's keys summed in one fixed order (sub-tile, MFMA).  A row's bits depend
// on its own qf, window, mask, slope, W and C - not on N, lane, wave, workgroup or its place in the grid.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kSub = 16;       // keys of one MFMA sub-tile
constexpr int kMaxHeads = 16;  // rows of the MFMA tile

// Waves per SIMD of each instantiation by its registers (profiles/sdpa_mfma/resource_usage.txt: 106 + 4 / 129 + 8 / 187 + 16 /
// 255 + 76 VGPRs + AGPRs of 512 for DB = 1 / 2 / 4 / 8, no scratch, no LDS); a workgroup puts one wave on each of a CU's four SIMDs,
// so this is also the workgroups a CU holds at once.
constexpr int step_groups_per_cu(int DB) { return DB == 1 ? 4 : DB == 2 ? 3 : DB == 4 ? 2 : 1; }

struct StepArgs {
    const float *qf, *x, *cache;   // cache NULL: an empty one (zeros, every cached step hidden)
    const uint8_t *cache_mask;     // NULL with cache
    const float *slopes;           // or NULL
    float *ctx, *cache_out;        // cache_out may be NULL
    uint8_t *mask_out;             // may be NULL
    int64_t N, W;
    int H, C;
    float scale;
};

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// DB: 16-wide d-blocks (C <= 16 DB, C % 4 == 0).
template <int DB>
__global__ __launch_bounds__(kBlock) void attn_step_kernel(const StepArgs p) {
    const int C = p.C;
    const int64_t W = p.W;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const bool head = i < p.H;
    const float slope = (p.slopes && head) ? p.slopes[i] : 0.0f;
    // (the loop's condition is the wave's: all 64 lanes take every shuffle below)
    for (int64_t n = int64_t(blockIdx.x) * kWavesPerBlock + wave; n < p.N; n += int64_t(gridDim.x) * kWavesPerBlock) {
        const float *x_row = p.x + n * C;
        // the lane's folded query, once (heads past H: zeros)
        const float *q_row = p.qf + (n * p.H + (head ? i : 0)) * C;
        float4 qb[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) {
            const int d = 16 * t + 4 * kk;
            const float4 q = *reinterpret_cast<const float4 *>(q_row + (d < C ? d : 0));
            qb[t] = (head && d < C) ? q : zero4();
        }
        native_float4 o[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) o[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};
        float m = -INFINITY, l = 0.0f;

        // row `key` of the window: the cache's for key < W, x for key == W; keys past W and a NULL cache re-read x's row (selected away)
        auto window_row = [&](int64_t key) { return (p.cache && key < W) ? p.cache + (n * W + key) * C : x_row; };

        float4 k_ahead[DB];    // X[k0 + i][16 t + 4 kk .. + 3] as loaded (zeros for a NULL cache)
        float v_ahead[DB][4];  // X[k0 + 4 kk + j][16 t + i], zero where the key is hidden
        uint8_t bit_ahead[4];  // cache_mask[n][k0 + 4 kk + j] as loaded; 0 for a NULL cache and past key W, 1 for key W: nonzero = visible
        auto request = [&](int64_t k0) {
            const int64_t key = k0 + i;
            const float *k_row = window_row(key);
            const bool stored = p.cache || key >= W;  // (an empty cache holds zeros)
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + 4 * kk;
                const float4 a = *reinterpret_cast<const float4 *>(k_row + (d < C ? d : 0));
                k_ahead[t] = stored ? a : zero4();
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = k0 + 4 * kk + j;
                const uint8_t bit = (p.cache_mask && row < W) ? p.cache_mask[n * W + row] : uint8_t(row == W);
                bit_ahead[j] = bit;
                const float *v_row = window_row(row);
#pragma unroll
                for (int t = 0; t < DB; ++t) {
                    const int d = 16 * t + i;
                    const float a = v_row[d < C ? d : 0];
                    v_ahead[t][j] = (bit && d < C) ? a : 0.0f;
                }
            }
        };
        request(0);
        for (int64_t k0 = 0; k0 <= W; k0 += kSub) {
            float4 ka[DB];
            float va[DB][4];
            uint8_t bit[4];
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                ka[t] = k_ahead[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) va[t][j] = v_ahead[t][j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) bit[j] = bit_ahead[j];
            if (k0 + kSub <= W) request(k0 + kSub);  // in flight across this sub-tile's MFMAs
            // ---- the roll: key k0 + i becomes row k0 + i - 1 of the new cache, as loaded
            const int64_t key = k0 + i;
            if (p.cache_out && key >= 1 && key <= W) {
                float *dst = p.cache_out + (n * W + key - 1) * C;
#pragma unroll
                for (int t = 0; t < DB; ++t) {
                    const int d = 16 * t + 4 * kk;
                    if (d < C) *reinterpret_cast<float4 *>(dst + d) = ka[t];
                }
            }
            if (p.mask_out && i == 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t row = k0 + 4 * kk + j;
                    if (row >= 1 && row <= W) p.mask_out[n * W + row - 1] = bit[j];  // (key W: 1)
                }
            }
            // ---- S^T of the sub-tile: the lane ends with head i against keys k0 + 4 kk + reg
            native_float4 st{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const bool in = key <= W && 16 * t + 4 * kk < C;
                const float4 a = in ? ka[t] : zero4();
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, qb[t].x, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, qb[t].y, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, qb[t].z, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, qb[t].w, st, 0, 0, 0);
            }
            float score[4], top = -INFINITY;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t j = k0 + 4 * kk + reg;
                // Band::score at i = 0: one rounding of qk * scale, one of the fmaf
                const float s = st[reg] * p.scale;
                score[reg] = bit[reg] ? (p.slopes ? fmaf(-slope, float(W - j), s) : s) : -INFINITY;
                top = fmaxf(top, score[reg]);
            }
            top = fmaxf(top, __shfl_xor(top, 16));
            top = fmaxf(top, __shfl_xor(top, 32));
            const float alpha = softmax_step(m, top, score);
            float part = (score[0] + score[1]) + (score[2] + score[3]);
            part += __shfl_xor(part, 16);  // (a + b on both partners: the four lanes of a head end with the same bits)
            part += __shfl_xor(part, 32);
            l = l * alpha + part;
            // ---- ctx^T += X^T P^T: the probabilities are B operands where they are
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                native_float4 acc = o[t] * alpha;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t][j], score[j], acc, 0, 0, 0);
                o[t] = acc;
            }
        }
        if (head) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // (key W is always visible: l >= 1)
            float *dst = p.ctx + (n * p.H + i) * C;
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + 4 * kk;
                if (d < C) *reinterpret_cast<float4 *>(dst + d) = make_float4(o[t][0] * inv, o[t][1] * inv, o[t][2] * inv, o[t][3] * inv);
            }
        }
    }
}

template <int DB>
void launch_attn_step(const StepArgs &p, int cus, void *stream) {
    const int64_t groups = ceil_div(p.N, int64_t(kWavesPerBlock)), resident = int64_t(step_groups_per_cu(DB)) * cus;
    const dim3 grid{uint32_t(groups < resident ? groups : resident)};
    hipLaunchKernelGGL((attn_step_kernel<DB>), grid, dim3{kBlock}, 0, as_stream(stream), p);
}

struct Bytes {  // [at, at + size) of one operand; absent when at is NULL
    const void *at;
    int64_t size;
};

bool overlap(const Bytes &a, const Bytes &b) {
    if (!a.at || !b.at || a.size == 0 || b.size == 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.at), b0 = reinterpret_cast<uintptr_t>(b.at);
    return a0 < b0 + uintptr_t(b.size) && b0 < a0 + uintptr_t(a.size);
}

bool valid_step_sizes(int64_t N, int64_t H, int64_t W, int64_t C) {
    return N >= 0 && H >= 1 && W >= 1 && C >= 1 && C <= CUSRL_MAX_SDPA_HEAD_DIM;
}

// The ONE statement of what the step kernel takes, on valid sizes (slopes: checked by the forward entry too; NULL here for the twin).
bool step_supported(const float *qf, const float *x, const float *cache, const uint8_t *cache_mask, const float *slopes, const float *ctx,
                    const float *cache_out, const uint8_t *mask_out, int64_t N, int64_t H, int64_t W, int64_t C) {
    if (H > kMaxHeads || C < 4 || C % 4 != 0) return false;
    if ((cache == nullptr) != (cache_mask == nullptr)) return false;
    if (!sizes_fit(N, H, 1, W, C)) return false;  // N * W * C and N * H * C within int64
    for (const void *ptr : {(const void *)qf, (const void *)x, (const void *)cache, (const void *)ctx, (const void *)cache_out})
        if (!aligned(ptr, 16)) return false;
    if (!aligned(slopes, 4)) return false;
    const int64_t f = int64_t(sizeof(float));
    const Bytes in[5] = {{qf, N * H * C * f}, {x, N * C * f}, {cache, N * W * C * f}, {cache_mask, N * W}, {slopes, H * f}};
    const Bytes out[3] = {{ctx, N * H * C * f}, {cache_out, N * W * C * f}, {mask_out, N * W}};
    for (int a = 0; a < 3; ++a) {
        for (const Bytes &r : in)
            if (overlap(out[a], r)) return false;  // the roll is never done in place: another wave may still read those rows
        for (int b = a + 1; b < 3; ++b)
            if (overlap(out[a], out[b])) return false;
    }
    return true;
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_attn_step_forward_supported(const float *qf, const float *x, const float *cache, const uint8_t *cache_mask,
                                                 const float *ctx, const float *cache_out, const uint8_t *mask_out, int64_t N, int64_t H,
                                                 int64_t W, int64_t C) {
    return qf && x && ctx && valid_step_sizes(N, H, W, C) && step_supported(qf, x, cache, cache_mask, nullptr, ctx, cache_out, mask_out, N, H, W, C);
}

extern "C" int cusrl_attn_step_forward(const float *qf, const float *x, const float *cache, const uint8_t *cache_mask,
                                       const float *alibi_slopes, float scale, float *ctx, float *cache_out, uint8_t *mask_out, int64_t N,
                                       int64_t H, int64_t W, int64_t C, void *stream) {
    if (!valid_step_sizes(N, H, W, C)) return CUSRL_E_INVALID;
    if (N == 0) return 0;  // (before the pointers: an empty tensor has none)
    if (!qf || !x || !ctx) return CUSRL_E_INVALID;
    if (!step_supported(qf, x, cache, cache_mask, alibi_slopes, ctx, cache_out, mask_out, N, H, W, C)) return CUSRL_E_UNSUPPORTED;
    StepArgs p;
    p.qf = qf, p.x = x, p.cache = cache, p.cache_mask = cache_mask, p.slopes = alibi_slopes, p.ctx = ctx, p.cache_out = cache_out;
    p.mask_out = mask_out, p.N = N, p.W = W, p.H = int(H), p.C = int(C), p.scale = scale;
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    if (C <= 16) launch_attn_step<1>(p, cus, stream);
    else if (C <= 32) launch_attn_step<2>(p, cus, stream);
    else if (C <= 64) launch_attn_step<4>(p, cus, stream);
    else launch_attn_step<8>(p, cus, stream);
    return launch_status();
}
