// Dense scaled dot-product attention, forward only, on v_mfma_f32_16x16x4_f32 ("Attention on the matrix cores"): the
// formulas and the visibility of cusrl_sdpa_fwd (include/cusrl_hip.h; `Mask` of attention_common.hpp, passed by value) for long
// keys and large heads, where the VALU body of attention.hip walks D-long dot products out of LDS lane by lane.  Opt-in
// (ops.sdpa(matrix_core=True)): the sum over d and over keys is ordered differently, so the bits are not that kernel's.
//
// Formulation (transposed, as in mlp_forward.hip).  The instruction's operands: lane (i = lane & 15, kk = lane >> 4) supplies
// A[i][kk] and B[kk][m] (m = lane & 15) and holds D[4 kk + reg][m]; the four k values a lane feeds to four consecutive MFMAs are
// k = 16 t + 4 kk + j.  A wave owns 16 queries q0 .. q0 + 15 of one (n, h) and a lane is bound to ONE of them, query q0 + m:
//   * scores  S^T[key][query] = sum_d K[key][d] Q[query][d] of a 16-key sub-tile: the A operands of d-block t are one float4 of a
//     K row out of LDS (K[k0 + i][16 t + 4 kk .. + 3]), the B operands one float4 of the lane's Q row (Q[q0 + m][16 t + 4 kk .. + 3]),
//     which the wave loads once per query tile from global memory and keeps in registers, unscaled (score = qk * scale (+ bias)
//     rounds as Mask::score does).  Afterwards the lane holds the scores of query q0 + m against keys k0 + 4 kk + reg;
//   * online softmax per query: m, l and alpha are per-lane scalars; the sub-tile's row maximum and row sum are the lane's four
//     registers combined with the three lanes that share m (lane ^ 16, lane ^ 32; a + b on both partners: the same bits in all
//     four), through softmax_step as it stands;
//   * O^T[d][query] += sum_key V[key][d] P[query][key]: the B operand of MFMA j is the lane's own probability register j
//     (P^T[4 kk + j][m]) - the probabilities never leave the registers - and the A operand is V[k0 + 4 kk + j][16 t + i] out of LDS.
//     The wave keeps ceil(D / 16) accumulator tiles of O^T, scales them by the lane's alpha before a sub-tile's MFMAs and by 1 / l at
//     the end; lane (m, kk) stores out[q0 + m][16 t + 4 kk .. + 3] as one float4 per tile, the kk == 0 lanes store lse.
// D % 16 != 0 is zero-padded inside the last d-block in A and in B, in registers.
//
// Work split.  A workgroup is 4 waves = 64 queries of one (n, h); K and V stream through LDS in tiles of 32 keys (two 16-key
// sub-tiles) staged ONCE per workgroup and read by all four waves.  The next tile's global loads are issued into registers in front
// of the current tile's MFMAs and written to LDS behind the next barrier (one LDS buffer, two barriers per tile).  Every wave passes
// every barrier: the key span is the workgroup's (that of its last wave), and a wave whose sub-tile is wholly masked still walks it -
// softmax_step gives alpha = 1 and p = 0 there, so it adds exact zeros.  Work items N * H * ceil(Lq / 64); the grid is
// min(items, c * CUs) workgroups that stride over them with 64-bit indices.
//
// LDS rows have a stride of ld = D | 4 floats, i.e. ld / 4 is odd.  (a) The scores' A read is 16 bytes per lane at rows i = 0 .. 15
// of one column: i * ld / 4 mod 16 takes 16 different values, so the 16 lanes of a kk group cover the 64 banks once.  (b) The PV read
// is 4 bytes per lane, 16 lanes along d and the four kk groups 4 rows apart: 4 * ld = 16 * odd floats, so the groups start at banks
// 0, 16, 32, 48 in some order.  Both patterns are conflict-free, and rows stay 16-byte aligned for the float4 stores that fill them.
//
// Determinism: one owning lane per output element, a query's keys summed in one fixed order (tile, sub-tile, MFMA), no atomics and
// no sums across workgroups.  A query row's bits depend on its keys, values, mask row and D - not on lane, wave, workgroup or Lq.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kQueries = kWavesPerBlock * kOwn;  // queries of a workgroup: 16 per wave
constexpr int kSub = 16;                          // keys of one MFMA sub-tile (kTile = 32 keys are staged per step)

// Workgroups a CU holds at once, one wave each on its four SIMDs = the kernel's waves per SIMD by its registers
// (profiles/sdpa_mfma/resource_usage.txt: 115 / 128 / 177 / 282 of 512 for DB = 1 / 2 / 4 / 8); LDS (at most 33 KiB of 160) allows four.
constexpr int groups_per_cu(int DB) { return DB <= 2 ? 4 : DB == 4 ? 2 : 1; }

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// DB: 16-wide d-blocks (D <= 16 DB, D % 4 == 0).
template <int DB>
__global__ __launch_bounds__(kBlock) void sdpa_fwd_mfma_kernel(Rows q, Rows k, Rows v, Mask vis, float *out, float *lse, Shape s,
                                                               int64_t q_tiles, int64_t items) {
    extern __shared__ float4 lds[];
    constexpr int kLoads = DB >= 2 ? DB / 2 : 1;  // float4 per thread, tensor and key tile: 32 rows of at most 4 DB float4 over 256 threads
    const int D = s.D, ld = D | 4, per_row = D / 4;
    float *sk = reinterpret_cast<float *>(lds), *sv = sk + kTile * ld;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;

    // this thread's slots of a staged tile: (row, column) of float4 number threadIdx.x + 256 u; rows at or past kTile do not exist
    int slot_row[kLoads], slot_col[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
        const int at = threadIdx.x + u * kBlock;
        slot_row[u] = at / per_row;
        slot_col[u] = (at - slot_row[u] * per_row) * 4;
    }

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kQueries, iq = q0 + wave * kOwn + i;  // the lane's query
        // the lane's Q row, once (queries past the end re-read the last one; nothing is stored for them)
        const float *q_row = q.p + n * q.sn + min(iq, s.Lq - 1) * q.sl + h * D;
        float4 qb[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) {
            const int d = 16 * t + 4 * kk;
            const float4 x = *reinterpret_cast<const float4 *>(q_row + (d < D ? d : 0));
            qb[t] = d < D ? x : zero4();
        }
        native_float4 o[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) o[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};
        float m = -INFINITY, l = 0.0f;

        const Span keys = vis.keys(q0 + kQueries - kOwn, s);  // the span of the workgroup's last wave covers every wave's
        const float *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        float4 k_ahead[kLoads], v_ahead[kLoads];
        // keys at or past Lk are zeros (unpredicated loads from clamped addresses, then a select)
        auto request = [&](int64_t k0) {
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int64_t key = k0 + min(slot_row[u], kTile - 1), from = min(key, s.Lk - 1);
                const float4 a = *reinterpret_cast<const float4 *>(k_base + from * k.sl + slot_col[u]);
                const float4 b = *reinterpret_cast<const float4 *>(v_base + from * v.sl + slot_col[u]);
                k_ahead[u] = key < s.Lk ? a : zero4();
                v_ahead[u] = key < s.Lk ? b : zero4();
            }
        };
        request(keys.begin);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kTile) {
            __syncthreads();  // the previous tile's readers are done
#pragma unroll
            for (int u = 0; u < kLoads; ++u)
                if (slot_row[u] < kTile) {
                    *reinterpret_cast<float4 *>(sk + slot_row[u] * ld + slot_col[u]) = k_ahead[u];
                    *reinterpret_cast<float4 *>(sv + slot_row[u] * ld + slot_col[u]) = v_ahead[u];
                }
            __syncthreads();
            if (k0 + kTile < keys.end) request(k0 + kTile);  // in flight across this tile's MFMAs
#pragma unroll
            for (int ks = 0; ks < kTile; ks += kSub) {
                // ---- S^T of the sub-tile: the lane ends with query iq against keys k0 + ks + 4 kk + reg
                native_float4 st{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int t = 0; t < DB; ++t) {
                    const int d = 16 * t + 4 * kk;
                    const float4 a = d < D ? *reinterpret_cast<const float4 *>(sk + (ks + i) * ld + d) : zero4();
                    st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, qb[t].x, st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, qb[t].y, st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, qb[t].z, st, 0, 0, 0);
                    st = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, qb[t].w, st, 0, 0, 0);
                }
                float score[4], top = -INFINITY;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int64_t j = k0 + ks + 4 * kk + reg;
                    score[reg] = (iq < s.Lq && j < s.Lk) ? vis.score(st[reg], s.scale, n, h, iq, j, s.Lq) : -INFINITY;
                    top = fmaxf(top, score[reg]);
                }
                top = fmaxf(top, __shfl_xor(top, 16));
                top = fmaxf(top, __shfl_xor(top, 32));
                const float alpha = softmax_step(m, top, score);
                float part = (score[0] + score[1]) + (score[2] + score[3]);
                part += __shfl_xor(part, 16);  // (a + b on both partners: the four lanes of a query end with the same bits)
                part += __shfl_xor(part, 32);
                l = l * alpha + part;
                // ---- O^T += V^T P^T: the probabilities are B operands where they are
#pragma unroll
                for (int t = 0; t < DB; ++t) {
                    const int d = 16 * t + i;
                    native_float4 acc = o[t] * alpha;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float a = d < D ? sv[(ks + 4 * kk + j) * ld + d] : 0.0f;
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, score[j], acc, 0, 0, 0);
                    }
                    o[t] = acc;
                }
            }
        }
        if (iq < s.Lq) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // a row with no visible key: zeros and lse = -inf
            float *dst = out + ((n * s.Lq + iq) * s.H + h) * D;
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + 4 * kk;
                if (d < D) *reinterpret_cast<float4 *>(dst + d) = make_float4(o[t][0] * inv, o[t][1] * inv, o[t][2] * inv, o[t][3] * inv);
            }
            if (kk == 0) lse[(n * s.H + h) * s.Lq + iq] = l > 0.0f ? m + logf(l) : -INFINITY;
        }
    }
}

template <int DB>
void launch_fwd_mfma(const Rows &q, const Rows &k, const Rows &v, const Mask &mask, float *out, float *lse, const Shape &s, int cus,
                     int64_t q_tiles, int64_t items, void *stream) {
    const int64_t resident = int64_t(groups_per_cu(DB)) * cus;
    const dim3 grid{uint32_t(items < resident ? items : resident)};
    const size_t lds = size_t(2) * kTile * (s.D | 4) * sizeof(float);  // K and V tile: 33 KiB at D = 128
    hipLaunchKernelGGL((sdpa_fwd_mfma_kernel<DB>), grid, dim3{kBlock}, lds, as_stream(stream), q, k, v, mask, out, lse, s, q_tiles, items);
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_sdpa_fwd_mfma_supported(int64_t Lq, int64_t Lk, int64_t D) {
    return Lq >= 1 && Lk >= 1 && D >= 4 && D <= CUSRL_MAX_SDPA_HEAD_DIM && D % 4 == 0;
}

extern "C" int cusrl_sdpa_fwd_mfma(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                   int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *keep_mask,
                                   const float *bias, int64_t mask_stride_n, int64_t mask_stride_h, int64_t mask_stride_q,
                                   int64_t mask_stride_k, int causal, float scale, float *out, float *lse, int64_t N, int64_t H,
                                   int64_t Lq, int64_t Lk, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || (keep_mask && bias) || !valid_sizes(N, H, Lq, Lk, D)) return CUSRL_E_INVALID;
    if (!sizes_fit(N, H, Lq, Lk, D) || !cusrl_sdpa_fwd_mfma_supported(Lq, Lk, D)) return CUSRL_E_UNSUPPORTED;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    if (!rows_vectorise({rq, rk, rv}, int(D)) || !aligned(out, 16)) return CUSRL_E_UNSUPPORTED;
    const int64_t q_tiles = ceil_div(Lq, kQueries);
    if (N * H > INT64_MAX / q_tiles) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const Mask mask{keep_mask, bias, mask_stride_n, mask_stride_h, mask_stride_q, mask_stride_k, causal != 0};
    const Shape shape{N, H, Lq, Lk, int(D), scale};
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t items = N * H * q_tiles;
    if (D <= 16) launch_fwd_mfma<1>(rq, rk, rv, mask, out, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 32) launch_fwd_mfma<2>(rq, rk, rv, mask, out, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 64) launch_fwd_mfma<4>(rq, rk, rv, mask, out, lse, shape, cus, q_tiles, items, stream);
    else launch_fwd_mfma<8>(rq, rk, rv, mask, out, lse, shape, cus, q_tiles, items, stream);
    return launch_status();
}
