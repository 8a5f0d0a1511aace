// Dense scaled dot-product attention, forward only, with bf16 operands on v_mfma_f32_16x16x32_bf16 ("The forward on
// bf16 operands"): cusrl_sdpa_fwd_mfma's argument list, masks (`Mask` of attention_common.hpp, passed by value) and formulas, with
// q, k, v and out in bf16 - what the attention layers hold under bf16 autocast.  Opt-in (ops.sdpa(matrix_core=True) on bf16 tensors).
//
// Numerics.  The scores are bf16 x bf16 products accumulated in fp32 by the MFMA; score = qk * scale (+ bias) in fp32 through
// Mask::score; m, l, alpha and lse are fp32 and l sums the UNROUNDED fp32 probabilities; the probabilities that go into P V are rounded
// to bf16 (nearest even); the O accumulators are fp32, scaled by 1 / l and rounded to bf16 once, on the store.
//
// Formulation (transposed, as in attention_mfma.hip).  The instruction's operands: lane (i = lane & 15, kk = lane >> 4) supplies the
// eight k slots (kk, j), j = 0 .. 7, of row i of A and of column m = lane & 15 of B, and holds D[4 kk + reg][m].  Which k index of the
// hardware a slot is does not matter: a slot is a summation label, the same one in A and in B.  A wave owns 16 queries q0 .. q0 + 15
// of one (n, h) and a lane is bound to ONE of them, query q0 + m:
//   * scores  S^T[key][query] = sum_d K[key][d] Q[query][d] of a 16-key sub-tile: slot (kk, j) of d-block t is d = 32 t + 8 kk + j;
//     the A operand is one 16-byte LDS read K[k0 + i][32 t + 8 kk .. + 7], the B operand 8 bf16 of the lane's own Q row, loaded once
//     per item and kept in registers.  One MFMA per 32-wide d-block; D % 32 != 0 is zero-padded in registers in A and in B.
//     Afterwards the lane holds query q0 + m against keys k0 + 4 kk + reg;
//   * online softmax per query over the whole 32-key tile (both sub-tiles, 8 scores per lane): the tile's row maximum and row sum
//     are the lane's eight registers, ((s0 + s1) + (s2 + s3)) + ((s4 + s5) + (s6 + s7)), combined with the three lanes that share m
//     (lane ^ 16, then lane ^ 32; a + b on both partners: the same bits in all four), through softmax_step as it stands;
//   * O^T[d][query] += sum_key V[key][d] P[query][key]: ONE MFMA per 16-wide d-block and 32-key tile.  Slot (kk, j) is key 4 kk + j
//     of sub-tile 0 for j < 4 and key 16 + 4 kk + (j - 4) of sub-tile 1 for j >= 4 - exactly the eight keys whose probabilities the
//     lane holds, so its eight registers, rounded to bf16 and packed, ARE its B operand: the probabilities never leave the
//     registers.  The A operand is V^T[16 t + i][those eight keys]: one 16-byte LDS read, because V is staged transposed and
//     key-permuted (below).  The wave keeps ceil(D / 16) accumulator tiles of O^T, scales them by alpha before a tile's MFMAs and
//     by 1 / l at the end; lane (m, kk) stores out[q0 + m][16 t + 4 kk .. + 3] as 8 bytes per tile, the kk == 0 lanes store lse.
//
// Sum order.  Over d: d-blocks of 32 in index order, inside a block the 32 products of one MFMA (the hardware's order, the same
// for every row).  Over keys: tiles of 32 in index order from the span's first key; inside a tile l adds the 32 probabilities in
// the tree above, and O adds the 32 products of one MFMA.  One owning lane per output element, no atomics, no sums across
// workgroups: a query row's bits depend on its keys, values, mask row and D - not on lane, wave, workgroup, batch position or Lq.
// (A tile that lies wholly behind a causal row's last key adds exact zeros with alpha = 1.)
//
// Work split.  A workgroup is 4 waves = 64 queries of one (n, h); K and V stream through LDS in tiles of 32 keys staged ONCE per
// workgroup as bf16 and read by all four waves.  The next tile's global loads are issued into registers in front of the current
// tile's MFMAs and written to LDS behind the next barrier (one buffer, two barriers per tile); every wave passes every barrier
// (the key span is that of the workgroup's last wave).  Work items N * H * ceil(Lq / 64); min(items, c * CUs) workgroups stride
// over them with 64-bit indices.
//
// LDS.  K tile: row-major, 32 rows of ld = D | 8 bf16, so a row is an odd number of 16-byte units: the scores' A read (16 bytes per
// lane at rows i = 0 .. 15 of one column) starts at unit i * odd + const, 16 different units mod 16 - the 16 lanes of a kk group
// cover the 64 banks once.  Staged d-fastest (thread -> 16 bytes of a row, neighbours along the row): coalesced global reads,
// contiguous LDS writes.  V tile: TRANSPOSED, D rows of 40 bf16 (32 keys + 8 of padding = 5 units, odd), key kappa of the tile at
// column 8 ((kappa & 15) >> 2) + 4 (kappa >> 4) + (kappa & 3), so a lane's eight keys are one aligned 16-byte read at unit
// 5 (16 t + i) + kk: again 16 different units mod 16 per kk group, no conflict.  The transposition is paid on the write: a thread
// takes 16 bytes of one V row and writes eight 2-byte values into eight rows of V^T.  Staged key-fastest (thread -> key at & 31,
// 16-byte chunk at >> 5): the 32 keys of a chunk write 64 contiguous bytes of one V^T row (16 banks, two keys per word) and the
// wave's second chunk lies 8 rows = 640 bytes further, 32 banks away - conflict-free, where a d-fastest order would put 16 chunks
// of one key 0 or 32 banks apart (8-way).  The price is global reads of 32 bytes per row and wave instruction instead of whole rows.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kQueries = kWavesPerBlock * kOwn;  // queries of a workgroup: 16 per wave
constexpr int kLdv = kTile + 8;                   // bf16 per row of the transposed V tile

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t word4 __attribute__((ext_vector_type(4)));  // 16 opaque bytes = 8 bf16

struct Rows16 {  // Rows of attention_common.hpp with bf16 elements (strides in elements)
    const uint16_t *p;
    int64_t sn, sl;
};

// Workgroups a CU holds at once, one wave each on its four SIMDs = the kernel's waves per SIMD by its registers
// (profiles/sdpa_mfma/resource_usage.txt, "bf16": 115 / 121 / 135 / 183 of 512 for DB = 1 / 2 / 4 / 8); LDS (at most 18.5 KiB of
// 160) allows four.
constexpr int groups_per_cu(int DB) { return DB <= 2 ? 4 : DB == 4 ? 3 : 2; }

// DB: 16-wide d-blocks of O (D <= 16 DB, D % 8 == 0); the scores take SB = ceil(DB / 2) 32-wide d-blocks.
template <int DB>
__global__ __launch_bounds__(kBlock) void sdpa_fwd_bf16_kernel(Rows16 q, Rows16 k, Rows16 v, Mask vis, uint16_t *out, float *lse,
                                                               Shape s, int64_t q_tiles, int64_t items) {
    extern __shared__ word4 lds[];
    constexpr int SB = (DB + 1) / 2;
    constexpr int kLoads = DB == 8 ? 2 : 1;  // 16-byte chunks per thread, tensor and key tile: 32 rows of at most 2 DB chunks over 256 threads
    const int D = s.D, ld = D | 8, per_row = D / 8;
    uint16_t *sk = reinterpret_cast<uint16_t *>(lds), *svt = sk + kTile * ld;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const word4 zero{0u, 0u, 0u, 0u};

    // this thread's chunks of a staged tile.  K, d-fastest: chunk number at = (row, column); V, key-fastest: at = (chunk, key);
    // rows at or past kTile and chunks at or past per_row do not exist
    int k_row[kLoads], k_col[kLoads], v_key[kLoads], v_col[kLoads], v_at[kLoads];
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
        const int at = threadIdx.x + u * kBlock;
        k_row[u] = at / per_row;
        k_col[u] = (at - k_row[u] * per_row) * 8;
        v_key[u] = at & (kTile - 1);
        v_col[u] = (at / kTile) * 8;
        v_at[u] = 8 * ((v_key[u] & 15) >> 2) + 4 * (v_key[u] >> 4) + (v_key[u] & 3);  // the key's column of V^T
    }

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kQueries, iq = q0 + wave * kOwn + i;  // the lane's query
        // the lane's Q row, once (queries past the end re-read the last one; nothing is stored for them)
        const uint16_t *q_row = q.p + n * q.sn + min(iq, s.Lq - 1) * q.sl + h * D;
        bf16x8 qb[SB];
#pragma unroll
        for (int t = 0; t < SB; ++t) {
            const int d = 32 * t + 8 * kk;
            const word4 x = *reinterpret_cast<const word4 *>(q_row + (d < D ? d : 0));
            qb[t] = __builtin_bit_cast(bf16x8, d < D ? x : zero);
        }
        native_float4 o[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) o[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};
        float m = -INFINITY, l = 0.0f;

        const Span keys = vis.keys(q0 + kQueries - kOwn, s);  // the span of the workgroup's last wave covers every wave's
        const uint16_t *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        word4 k_ahead[kLoads], v_ahead[kLoads];
        // keys at or past Lk are zeros (unpredicated loads from clamped addresses, then a select)
        auto request = [&](int64_t k0) {
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                const int64_t key = k0 + min(k_row[u], kTile - 1), key_v = k0 + v_key[u];
                const word4 a = *reinterpret_cast<const word4 *>(k_base + min(key, s.Lk - 1) * k.sl + k_col[u]);
                const word4 b = *reinterpret_cast<const word4 *>(v_base + min(key_v, s.Lk - 1) * v.sl + (v_col[u] < D ? v_col[u] : 0));
                k_ahead[u] = key < s.Lk ? a : zero;
                v_ahead[u] = key_v < s.Lk ? b : zero;
            }
        };
        request(keys.begin);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kTile) {
            __syncthreads();  // the previous tile's readers are done
#pragma unroll
            for (int u = 0; u < kLoads; ++u) {
                if (k_row[u] < kTile) *reinterpret_cast<word4 *>(sk + k_row[u] * ld + k_col[u]) = k_ahead[u];
                if (v_col[u] < D) {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        svt[(v_col[u] + e) * kLdv + v_at[u]] = uint16_t(e & 1 ? v_ahead[u][e >> 1] >> 16 : v_ahead[u][e >> 1] & 0xffffu);
                }
            }
            __syncthreads();
            if (k0 + kTile < keys.end) request(k0 + kTile);  // in flight across this tile's MFMAs
            // ---- S^T of both sub-tiles: the lane ends with query iq against keys k0 + 16 sub + 4 kk + reg
            native_float4 st[2] = {native_float4{0.0f, 0.0f, 0.0f, 0.0f}, native_float4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
            for (int t = 0; t < SB; ++t) {
                const int d = 32 * t + 8 * kk;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const word4 a = d < D ? *reinterpret_cast<const word4 *>(sk + (16 * sub + i) * ld + d) : zero;
                    st[sub] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), qb[t], st[sub], 0, 0, 0);
                }
            }
            float score[8], top = -INFINITY;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int64_t j = k0 + 16 * (c >> 2) + 4 * kk + (c & 3);
                score[c] = (iq < s.Lq && j < s.Lk) ? vis.score(st[c >> 2][c & 3], s.scale, n, h, iq, j, s.Lq) : -INFINITY;
                top = fmaxf(top, score[c]);
            }
            top = fmaxf(top, __shfl_xor(top, 16));
            top = fmaxf(top, __shfl_xor(top, 32));
            const float alpha = softmax_step(m, top, score);
            float part = ((score[0] + score[1]) + (score[2] + score[3])) + ((score[4] + score[5]) + (score[6] + score[7]));
            part += __shfl_xor(part, 16);  // (a + b on both partners: the four lanes of a query end with the same bits)
            part += __shfl_xor(part, 32);
            l = l * alpha + part;
            // ---- O^T += V^T P^T: the lane's eight probabilities, rounded to bf16, are its B operand
            bf16x8 pb;
#pragma unroll
            for (int c = 0; c < 8; ++c) pb[c] = static_cast<__bf16>(score[c]);
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + i;
                const word4 a = d < D ? *reinterpret_cast<const word4 *>(svt + d * kLdv + 8 * kk) : zero;
                o[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), pb, o[t] * alpha, 0, 0, 0);
            }
        }
        if (iq < s.Lq) {
            const float inv = l > 0.0f ? 1.0f / l : 0.0f;  // a row with no visible key: zeros and lse = -inf
            uint16_t *dst = out + ((n * s.Lq + iq) * s.H + h) * D;
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + 4 * kk;
                if (d < D) {
                    bf16x4 r;
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) r[reg] = static_cast<__bf16>(o[t][reg] * inv);
                    *reinterpret_cast<bf16x4 *>(dst + d) = r;
                }
            }
            if (kk == 0) lse[(n * s.H + h) * s.Lq + iq] = l > 0.0f ? m + logf(l) : -INFINITY;
        }
    }
}

template <int DB>
void launch_fwd_bf16(const Rows16 &q, const Rows16 &k, const Rows16 &v, const Mask &mask, uint16_t *out, float *lse, const Shape &s,
                     int cus, int64_t q_tiles, int64_t items, void *stream) {
    const int64_t resident = int64_t(groups_per_cu(DB)) * cus;
    const dim3 grid{uint32_t(items < resident ? items : resident)};
    const size_t lds = (size_t(kTile) * (s.D | 8) + size_t(s.D) * kLdv) * sizeof(uint16_t);  // K and V^T tile: 18.5 KiB at D = 128
    hipLaunchKernelGGL((sdpa_fwd_bf16_kernel<DB>), grid, dim3{kBlock}, lds, as_stream(stream), q, k, v, mask, out, lse, s, q_tiles, items);
}

// 16-byte loads of 8 bf16: every row of every tensor starts on one
bool rows16_vectorise(std::initializer_list<Rows16> tensors) {
    for (const Rows16 &t : tensors)
        if (!aligned(t.p, 16) || t.sn % 8 || t.sl % 8) return false;
    return true;
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_sdpa_fwd_bf16_supported(int64_t Lq, int64_t Lk, int64_t D) {
    return Lq >= 1 && Lk >= 1 && D >= 8 && D <= CUSRL_MAX_SDPA_HEAD_DIM && D % 8 == 0;
}

extern "C" int cusrl_sdpa_fwd_bf16(const void *q, int64_t q_stride_n, int64_t q_stride_l, const void *k, int64_t k_stride_n,
                                   int64_t k_stride_l, const void *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *keep_mask,
                                   const float *bias, int64_t mask_stride_n, int64_t mask_stride_h, int64_t mask_stride_q,
                                   int64_t mask_stride_k, int causal, float scale, void *out, float *lse, int64_t N, int64_t H,
                                   int64_t Lq, int64_t Lk, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || (keep_mask && bias) || !valid_sizes(N, H, Lq, Lk, D)) return CUSRL_E_INVALID;
    if (!sizes_fit(N, H, Lq, Lk, D) || !cusrl_sdpa_fwd_bf16_supported(Lq, Lk, D)) return CUSRL_E_UNSUPPORTED;
    const Rows16 rq{static_cast<const uint16_t *>(q), q_stride_n, q_stride_l}, rk{static_cast<const uint16_t *>(k), k_stride_n, k_stride_l},
        rv{static_cast<const uint16_t *>(v), v_stride_n, v_stride_l};
    if (!rows16_vectorise({rq, rk, rv}) || !aligned(out, 16)) return CUSRL_E_UNSUPPORTED;
    const int64_t q_tiles = ceil_div(Lq, kQueries);
    if (N * H > INT64_MAX / q_tiles) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const Mask mask{keep_mask, bias, mask_stride_n, mask_stride_h, mask_stride_q, mask_stride_k, causal != 0};
    const Shape shape{N, H, Lq, Lk, int(D), scale};
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    uint16_t *o = static_cast<uint16_t *>(out);
    const int64_t items = N * H * q_tiles;
    if (D <= 16) launch_fwd_bf16<1>(rq, rk, rv, mask, o, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 32) launch_fwd_bf16<2>(rq, rk, rv, mask, o, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 64) launch_fwd_bf16<4>(rq, rk, rv, mask, o, lse, shape, cus, q_tiles, items, stream);
    else launch_fwd_bf16<8>(rq, rk, rv, mask, o, lse, shape, cus, q_tiles, items, stream);
    return launch_status();
}
