// Causal sliding-window ("band") attention, forward only, on v_mfma_f32_16x16x4_f32 ("The band on the matrix cores"):
// the formulas, edge rules and visibility of cusrl_band_sdpa_fwd (include/cusrl_hip.h; `Band` of attention_common.hpp, passed by
// value, its score() called per pair) for the Lq >= 2 passes of the recurrent transformer modules.  Opt-in
// (ops.band_sdpa(matrix_core=True)): the sum over d and over keys is ordered differently, so the bits are not the VALU kernel's.
//
// Formulation: the dense forward's (attention_mfma.hip).  Lane (i = m = lane & 15, kk = lane >> 4) supplies A[i][kk] and B[kk][m]
// and holds D[4 kk + reg][m]; a wave owns 16 queries q0 .. q0 + 15 of one (n, h) and a lane is bound to ONE of them, query q0 + m:
//   * scores  S^T = K Q^T of a 16-key sub-tile: the A operands of d-block t are one float4 K[k0 + i][16 t + 4 kk .. + 3], the B
//     operands one float4 of the lane's Q row, loaded once per item and kept unscaled (Band::score rounds qk * scale and the ALiBi
//     fmaf).  Afterwards the lane holds query q0 + m against keys k0 + 4 kk + reg;
//   * online softmax per query through softmax_step as it stands: row maximum and row sum are the lane's four registers combined
//     with lanes ^ 16 and ^ 32 (a + b on both partners: the same bits in all four lanes of a query);
//   * O^T += V^T P^T: the B operand of MFMA j is the lane's own probability register j - the probabilities never leave the
//     registers - and the A operand is V[k0 + 4 kk + j][16 t + i].  ceil(D / 16) accumulator tiles, scaled by alpha before a
//     sub-tile's MFMAs and by 1 / l at the end; lane (m, kk) stores out[q0 + m][16 t + 4 kk .. + 3] as one float4 per tile, the
//     kk == 0 lanes store lse.
// D % 16 != 0 is zero-padded inside the last d-block in A and in B, in registers.
//
// Work split - the band's own, not the dense kernel's 64-query workgroup.  The work item is ONE WAVE's 16 queries: items
// N * H * ceil(Lq / 16) with the query tile as the fast index; a workgroup is 4 waves on 4 consecutive items, which need not share
// an (n, h) (Lq = 24 pads 8 of 32 rows per sequence).  Each wave walks its own keys only, the 16-key sub-tiles from q0 up to
// min(Lk, q0 + 16 + W) = ceil((16 + W) / 16) of them, and the waves never wait for each other: no __syncthreads(), no LDS.  The
// grid is min(ceil(items / 4), c * CUs) workgroups that stride over the items with 64-bit indices.
//
// K and V come straight from global memory.  A key is seen by at most ceil((W + 16) / 16) + 1 query tiles and L2 serves that
// overlap; there is nothing a workgroup's waves share for LDS to stage.  The scores' A read is 16 bytes per lane, the four kk lanes
// of a key row on 64 contiguous bytes; the P.V read is 4 bytes per lane, 16 lanes on adjacent columns: one 64-byte segment per key
// row.  Keys at or past Lk are read from clamped addresses and selected to zero.  The next sub-tile's K and V loads are issued into
// registers in front of the current sub-tile's MFMAs.
//
// Determinism: one owning lane per output element, a query's keys summed in one fixed order (sub-tile, MFMA), no atomics.  A query
// row's bits depend on its keys, values, side-tensor rows, D, W and its place in its 16-query tile - not on lane, wave, workgroup,
// batch position or Lq.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kSub = 16;  // keys of one MFMA sub-tile = queries of a wave (kOwn)

// Waves per SIMD of each instantiation by its registers (profiles/sdpa_mfma/resource_usage.txt: 105 + 4 / 145 + 8 / 175 + 16 /
// 255 + 60 VGPRs + AGPRs of 512 for DB = 1 / 2 / 4 / 8, no scratch); a workgroup puts one wave on each of a CU's four SIMDs, so this
// is also the workgroups a CU holds at once.
constexpr int band_groups_per_cu(int DB) { return DB == 1 ? 4 : DB == 2 ? 3 : DB == 4 ? 2 : 1; }

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// DB: 16-wide d-blocks (D <= 16 DB, D % 4 == 0).
template <int DB>
__global__ __launch_bounds__(kBlock) void band_sdpa_fwd_mfma_kernel(Rows q, Rows k, Rows v, Band band, float *out, float *lse, Shape s,
                                                                    int64_t q_tiles, int64_t items) {
    const int D = s.D;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    // (the loop's condition is the wave's: all 64 lanes take every shuffle below)
    for (int64_t item = int64_t(blockIdx.x) * kWavesPerBlock + wave; item < items; item += int64_t(gridDim.x) * kWavesPerBlock) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kOwn, iq = q0 + i;  // the lane's query
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

        const Span keys = band.keys(q0, s);  // this wave's, nobody else's
        const float *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        float4 k_ahead[DB];
        float v_ahead[DB][4];
        // A operands of the sub-tile at k0: K[k0 + i][16 t + 4 kk .. + 3] and V[k0 + 4 kk + j][16 t + i]; keys at or past Lk and
        // columns at or past D are zeros (unpredicated loads from clamped addresses, then a select)
        auto request = [&](int64_t k0) {
            const int64_t key = k0 + i;
            const float *k_row = k_base + min(key, s.Lk - 1) * k.sl;
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                const int d = 16 * t + 4 * kk;
                const float4 a = *reinterpret_cast<const float4 *>(k_row + (d < D ? d : 0));
                k_ahead[t] = (key < s.Lk && d < D) ? a : zero4();
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = k0 + 4 * kk + j;
                const float *v_row = v_base + min(row, s.Lk - 1) * v.sl;
#pragma unroll
                for (int t = 0; t < DB; ++t) {
                    const int d = 16 * t + i;
                    const float a = v_row[d < D ? d : 0];
                    v_ahead[t][j] = (row < s.Lk && d < D) ? a : 0.0f;
                }
            }
        };
        request(keys.begin);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kSub) {
            float4 ka[DB];
            float va[DB][4];
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                ka[t] = k_ahead[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) va[t][j] = v_ahead[t][j];
            }
            if (k0 + kSub < keys.end) request(k0 + kSub);  // in flight across this sub-tile's MFMAs
            // ---- S^T of the sub-tile: the lane ends with query iq against keys k0 + 4 kk + reg
            native_float4 st{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].x, qb[t].x, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].y, qb[t].y, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].z, qb[t].z, st, 0, 0, 0);
                st = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[t].w, qb[t].w, st, 0, 0, 0);
            }
            float score[4], top = -INFINITY;
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t j = k0 + 4 * kk + reg;
                score[reg] = (iq < s.Lq && j < s.Lk) ? band.score(st[reg], s.scale, n, h, iq, j, s.Lq) : -INFINITY;
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
                native_float4 acc = o[t] * alpha;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(va[t][j], score[j], acc, 0, 0, 0);
                o[t] = acc;
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
void launch_band_fwd_mfma(const Rows &q, const Rows &k, const Rows &v, const Band &band, float *out, float *lse, const Shape &s, int cus,
                          int64_t q_tiles, int64_t items, void *stream) {
    const int64_t groups = ceil_div(items, int64_t(kWavesPerBlock)), resident = int64_t(band_groups_per_cu(DB)) * cus;
    const dim3 grid{uint32_t(groups < resident ? groups : resident)};
    hipLaunchKernelGGL((band_sdpa_fwd_mfma_kernel<DB>), grid, dim3{kBlock}, 0, as_stream(stream), q, k, v, band, out, lse, s, q_tiles, items);
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_band_sdpa_fwd_mfma_supported(int64_t Lq, int64_t W, int64_t D) {
    return Lq >= 2 && W >= 1 && D >= 4 && D <= CUSRL_MAX_SDPA_HEAD_DIM && D % 4 == 0;  // (Lq == 1 is the step kernel's)
}

extern "C" int cusrl_band_sdpa_fwd_mfma(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                        int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                                        const int32_t *q_segment, const float *alibi_slopes, float scale, float *out, float *lse, int64_t N,
                                        int64_t H, int64_t Lq, int64_t W, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || !valid_band_sizes(N, H, Lq, W, D)) return CUSRL_E_INVALID;
    if (!band_sizes_fit(N, H, Lq, W, D) || !cusrl_band_sdpa_fwd_mfma_supported(Lq, W, D)) return CUSRL_E_UNSUPPORTED;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    if (!rows_vectorise({rq, rk, rv}, int(D)) || !aligned(out, 16)) return CUSRL_E_UNSUPPORTED;
    const int64_t q_tiles = ceil_div(Lq, kOwn);
    if (N * H > INT64_MAX / q_tiles) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    const Band band{key_valid, q_segment, alibi_slopes, W};
    const Shape shape{N, H, Lq, Lq + W, int(D), scale};
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t items = N * H * q_tiles;
    if (D <= 16) launch_band_fwd_mfma<1>(rq, rk, rv, band, out, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 32) launch_band_fwd_mfma<2>(rq, rk, rv, band, out, lse, shape, cus, q_tiles, items, stream);
    else if (D <= 64) launch_band_fwd_mfma<4>(rq, rk, rv, band, out, lse, shape, cus, q_tiles, items, stream);
    else launch_band_fwd_mfma<8>(rq, rk, rv, band, out, lse, shape, cus, q_tiles, items, stream);
    return launch_status();
}
