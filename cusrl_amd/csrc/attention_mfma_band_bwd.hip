// Causal sliding-window ("band") attention, backward, on v_mfma_f32_16x16x4_f32 ("The band's backward on the matrix
// cores"): the formulas, edge rules, visibility, workspace (delta) and key_grad_from of cusrl_band_sdpa_bwd (include/cusrl_hip.h;
// `Band` of attention_common.hpp, passed by value, its score() called per pair) for Lq >= 2.  Opt-in
// (ops.band_sdpa(matrix_core_backward=True)): the sums run in another order, so the bits are not the VALU kernels'.  out and lse
// may come from either forward.
//
// Formulation: the dense backward's (attention_mfma_bwd.hip), its operands straight from global memory.  Lane (i = m = lane & 15,
// kk = lane >> 4) supplies A[i][kk] and B[kk][m] and holds D[4 kk + reg][m]; a wave owns 16 rows of one (n, h) and a lane is bound
// to ONE of them, row r0 + m: queries in the first launch, keys in the second.  Per 16-row sub-tile of the streamed side:
//   * two score-shaped products (score_product): the A operands of d-block t are one float4 of streamed row i (columns
//     16 t + 4 kk .. + 3), the B operands one float4 of a row the lane holds.  Afterwards the lane has the product of ITS row against
//     streamed rows 4 kk + reg of the sub-tile;
//   * p = probability(score, lse) and ds = p != 0 ? p (dp - delta) scale : 0 are per-lane arithmetic on those four registers and
//     never leave them: a masked pair or a row with lse = -inf gives p = 0 and ds = 0 exactly, exp(-inf - (-inf)) is never evaluated;
//   * the accumulations (accumulate): the B operand of MFMA j is the lane's own register j, the A operand is
//     streamed[4 kk + j][16 t + i]; ceil(D / 16) accumulator tiles per output, no rescaling.
// Query-major launch (dq, delta): the lane holds its Q and dout rows (DB float4 each), lse and delta; K and V stream over
//   Band::keys(q0) in 16-key sub-tiles from q0.  S^T = K Q^T (A: K row, B: Q), dP^T = V dout^T (A: V row, B: dout),
//   dQ^T += K^T dS^T (A: K[k0 + 4 kk + j][16 t + i], B: ds[j]).  delta_i = sum_d dout_id out_id from the lane's own float4s,
//   d = 16 t + 4 kk + e in the order t, e, then lanes ^ 16 and ^ 32 (a + b on both partners: the four lanes of a query hold the same
//   bits); the kk == 0 lanes store it to the workspace.  A query with no visible key gets dq = 0 exactly.
// Key-major launch (dk, dv): a wave owns keys j0 .. j0 + 15 with j0 = key_grad_from + 16 tile - the keys in front of key_grad_from
//   are never visited, and row j - key_grad_from of dk / dv [N, Lk - key_grad_from, H, D] is key j's - and the lane holds its K and
//   V rows; Q and dout stream over Band::queries(j0) in 16-query sub-tiles from the span's begin, which need not be a multiple of
//   16.  S = Q K^T (A: Q row, B: K), dP = dout V^T (A: dout row, B: V), dV^T += dout^T P and dK^T += Q^T dS (A: dout / Q
//   [i0 + 4 kk + j][16 t + i], B: p[j] / ds[j]).  The four lse / delta values of queries i0 + 4 kk + reg are four 4-byte loads each
//   (the span's begin is not 16-byte aligned).  A query at or past Lq scores -inf and adds exact zeros; a key no query sees gets
//   dk = dv = 0 exactly.
// Either way lane (m, kk) stores row r0 + m, columns 16 t + 4 kk .. + 3, as one float4 per tile.  D % 16 != 0 is zero-padded inside
// the last d-block in A and in B, in registers.
//
// Work split - the band forward's (attention_mfma_band.hip), not the dense backward's 64-row workgroup, which would walk the union of
// four spans (64 + W streamed rows per wave where 16 + W are needed) and pad Lq = 24 to 64.  The work item is ONE WAVE's 16 owned
// rows: N * H * ceil(Lq / 16) items in the first launch, N * H * ceil((Lk - key_grad_from) / 16) in the second, the tile as the fast
// index; a workgroup is 4 waves on 4 consecutive items, which need not share an (n, h).  Each wave walks its own span with its own
// trip count and the waves never wait for each other: no __syncthreads(), no LDS.  The grid is min(ceil(items / 4), c * CUs)
// workgroups that stride over the items with 64-bit indices.
//
// Streamed rows come straight from global memory in both read patterns: 16 bytes per lane for the score products (the four kk
// lanes of a row on 64 contiguous bytes), 4 bytes per lane with 16 lanes on adjacent columns for the accumulations (one 64-byte
// segment per row).  A streamed row is seen by at most ceil((W + 16) / 16) + 1 owning tiles and L2 serves that overlap.  Rows at or
// past the end are read from clamped addresses and selected to zero.  The next sub-tile's loads are issued into registers in front
// of the current sub-tile's MFMAs, in all eight instantiations.
//
// Determinism: one owning lane per output element, one fixed summation order per element (sub-tile, MFMA), no atomics, no sums
// across waves.  A dq row's bits depend on its own row of q / dout / out / lse, on its keys, values, side-tensor rows, D, W and its
// place in its 16-query tile - not on lane, wave, workgroup, batch position or Lq.  A dk / dv row's bits may ALSO depend on
// key_grad_from: it moves the key's place in its 16-key tile and the start of the query sub-tiles, hence the order of the sum over
// queries.  For one key_grad_from they do not depend on lane, wave, workgroup or batch position.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kSub = 16;  // streamed rows of one MFMA sub-tile = rows a wave owns (kOwn)

// Waves per SIMD of each instantiation by its registers (profiles/sdpa_mfma/resource_usage.txt, VGPRs + AGPRs of 512, no scratch);
// a workgroup puts one wave on each of a CU's four SIMDs, so this is also the workgroups a CU holds at once.
// (query-major 127 / 177 / 225 / 381, key-major 161 / 233 / 289 / 493 for DB = 1 / 2 / 4 / 8)
constexpr int band_bwd_groups_per_cu(int DB, bool key_major) { return DB == 1 ? (key_major ? 3 : 4) : DB == 2 ? 2 : DB == 4 ? (key_major ? 1 : 2) : 1; }

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// A lane's row of an [N, L, H, D] tensor as B operands: float4 t holds columns 16 t + 4 kk .. + 3, zeros at or past D.
template <int DB>
__device__ __forceinline__ void load_own_row(float4 (&b)[DB], const float *row, int kk, int D) {
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        const int d = 16 * t + 4 * kk;
        const float4 x = *reinterpret_cast<const float4 *>(row + (d < D ? d : 0));
        b[t] = d < D ? x : zero4();
    }
}

template <int DB>
__device__ __forceinline__ void store_own_row(float *row, const native_float4 (&acc)[DB], int kk, int D) {
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        const int d = 16 * t + 4 * kk;
        if (d < D) *reinterpret_cast<float4 *>(row + d) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
}

// The A operands of the 16-row sub-tile at r0 of a streamed tensor of L rows (`base`: its (n, h), `sl`: its row stride): rows at
// or past L and columns at or past D are zeros (unpredicated loads from clamped addresses, then a select).
// Score pattern: a[t] = X[r0 + i][16 t + 4 kk .. + 3].
template <int DB>
__device__ __forceinline__ void request_rows(float4 (&a)[DB], const float *base, int64_t sl, int64_t r0, int64_t L, int D, int i, int kk) {
    const int64_t r = r0 + i;
    const float *row = base + min(r, L - 1) * sl;
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        const int d = 16 * t + 4 * kk;
        const float4 x = *reinterpret_cast<const float4 *>(row + (d < D ? d : 0));
        a[t] = (r < L && d < D) ? x : zero4();
    }
}

// Accumulation pattern: a[t][j] = X[r0 + 4 kk + j][16 t + i].
template <int DB>
__device__ __forceinline__ void request_columns(float (&a)[DB][4], const float *base, int64_t sl, int64_t r0, int64_t L, int D, int i, int kk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t r = r0 + 4 * kk + j;
        const float *row = base + min(r, L - 1) * sl;
#pragma unroll
        for (int t = 0; t < DB; ++t) {
            const int d = 16 * t + i;
            const float x = row[d < D ? d : 0];
            a[t][j] = (r < L && d < D) ? x : 0.0f;
        }
    }
}

// sum_d streamed[i][d] own[d] of a sub-tile: the lane ends with its own row against sub-tile rows 4 kk + reg.
template <int DB>
__device__ __forceinline__ native_float4 score_product(const float4 (&a)[DB], const float4 (&own)[DB]) {
    native_float4 acc{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].x, own[t].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].y, own[t].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].z, own[t].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t].w, own[t].w, acc, 0, 0, 0);
    }
    return acc;
}

// acc[t][reg] (column 16 t + 4 kk + reg of the lane's row) += sum_j streamed[4 kk + j][16 t + i] w[j] over the sub-tile.
template <int DB>
__device__ __forceinline__ void accumulate(native_float4 (&acc)[DB], const float (&a)[DB][4], const float (&w)[4]) {
#pragma unroll
    for (int t = 0; t < DB; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], w[j], acc[t], 0, 0, 0);
}

template <int DB>
__device__ __forceinline__ void copy(float4 (&to)[DB], const float4 (&from)[DB]) {
#pragma unroll
    for (int t = 0; t < DB; ++t) to[t] = from[t];
}

template <int DB>
__device__ __forceinline__ void copy(float (&to)[DB][4], const float (&from)[DB][4]) {
#pragma unroll
    for (int t = 0; t < DB; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) to[t][j] = from[t][j];
}

// -------------------------------------------------------------------------------------------- query-major: dq and delta
// DB: 16-wide d-blocks (D <= 16 DB, D % 4 == 0).
template <int DB>
__global__ __launch_bounds__(kBlock) void band_sdpa_bwd_dq_mfma_kernel(Rows q, Rows k, Rows v, Rows o, Rows dout, const float *lse, Band band,
                                                                       float *dq, float *delta, Shape s, int64_t q_tiles, int64_t items) {
    const int D = s.D;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    // (the loop's condition is the wave's: all 64 lanes take every shuffle below)
    for (int64_t item = int64_t(blockIdx.x) * kWavesPerBlock + wave; item < items; item += int64_t(gridDim.x) * kWavesPerBlock) {
        const int64_t tile = item % q_tiles, nh = item / q_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t q0 = tile * kOwn, iq = q0 + i;  // the lane's query
        // the lane's rows, once (queries past the end re-read the last one; nothing is stored for them)
        const int64_t row = min(iq, s.Lq - 1);
        float4 qb[DB], dob[DB];
        load_own_row(qb, q.p + n * q.sn + row * q.sl + h * D, kk, D);
        load_own_row(dob, dout.p + n * dout.sn + row * dout.sl + h * D, kk, D);
        float row_delta = 0.0f;
        {
            float4 ob[DB];
            load_own_row(ob, o.p + n * o.sn + row * o.sl + h * D, kk, D);
#pragma unroll
            for (int t = 0; t < DB; ++t) {
                row_delta = fmaf(dob[t].x, ob[t].x, row_delta);
                row_delta = fmaf(dob[t].y, ob[t].y, row_delta);
                row_delta = fmaf(dob[t].z, ob[t].z, row_delta);
                row_delta = fmaf(dob[t].w, ob[t].w, row_delta);
            }
            row_delta += __shfl_xor(row_delta, 16);  // (a + b on both partners: the four lanes of a query end with the same bits)
            row_delta += __shfl_xor(row_delta, 32);
        }
        const float row_lse = iq < s.Lq ? lse[nh * s.Lq + iq] : -INFINITY;
        if (iq < s.Lq && kk == 0) delta[nh * s.Lq + iq] = row_delta;
        native_float4 acc[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) acc[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};

        const Span keys = band.keys(q0, s);  // this wave's, nobody else's
        const float *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        float4 k_ahead[DB], v_ahead[DB];
        float kc_ahead[DB][4];
        auto request = [&](int64_t k0) {
            request_rows(k_ahead, k_base, k.sl, k0, s.Lk, D, i, kk);
            request_rows(v_ahead, v_base, v.sl, k0, s.Lk, D, i, kk);
            request_columns(kc_ahead, k_base, k.sl, k0, s.Lk, D, i, kk);
        };
        request(keys.begin);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kSub) {
            float4 ka[DB], va[DB];
            float kc[DB][4];
            copy(ka, k_ahead), copy(va, v_ahead), copy(kc, kc_ahead);
            if (k0 + kSub < keys.end) request(k0 + kSub);  // in flight across this sub-tile's MFMAs
            // the lane ends with query iq against keys k0 + 4 kk + reg
            const native_float4 st = score_product(ka, qb);
            const native_float4 dp = score_product(va, dob);
            float ds[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t j = k0 + 4 * kk + reg;
                ds[reg] = 0.0f;
                if (iq < s.Lq && j < s.Lk) {
                    const float p = probability(band.score(st[reg], s.scale, n, h, iq, j, s.Lq), row_lse);
                    if (p != 0.0f) ds[reg] = p * (dp[reg] - row_delta) * s.scale;
                }
            }
            accumulate(acc, kc, ds);  // dQ^T += K^T dS^T: ds is the B operand where it is
        }
        if (iq < s.Lq) store_own_row(dq + ((n * s.Lq + iq) * s.H + h) * D, acc, kk, D);
    }
}

// ------------------------------------------------------------------------------------------------ key-major: dk and dv
template <int DB>
__global__ __launch_bounds__(kBlock) void band_sdpa_bwd_dkv_mfma_kernel(Rows q, Rows k, Rows v, Rows dout, const float *lse, const float *delta,
                                                                        Band band, float *dk, float *dv, Shape s, int64_t key_from,
                                                                        int64_t k_tiles, int64_t items) {
    const int D = s.D;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const int64_t rows_out = s.Lk - key_from;
    for (int64_t item = int64_t(blockIdx.x) * kWavesPerBlock + wave; item < items; item += int64_t(gridDim.x) * kWavesPerBlock) {
        const int64_t tile = item % k_tiles, nh = item / k_tiles, h = nh % s.H, n = nh / s.H;
        const int64_t j0 = key_from + tile * kOwn, jk = j0 + i;  // the lane's key
        // the lane's rows, once (keys past the end re-read the last one; nothing is stored for them)
        const int64_t row = min(jk, s.Lk - 1);
        float4 kb[DB], vb[DB];
        load_own_row(kb, k.p + n * k.sn + row * k.sl + h * D, kk, D);
        load_own_row(vb, v.p + n * v.sn + row * v.sl + h * D, kk, D);
        native_float4 acc_k[DB], acc_v[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) acc_k[t] = acc_v[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};

        const Span queries = band.queries(j0, s);  // this wave's, nobody else's
        const float *q_base = q.p + n * q.sn + h * D, *do_base = dout.p + n * dout.sn + h * D;
        const float *lse_base = lse + nh * s.Lq, *delta_base = delta + nh * s.Lq;
        float4 q_ahead[DB], do_ahead[DB];
        float qc_ahead[DB][4], doc_ahead[DB][4], lse_ahead[4], delta_ahead[4];
        auto request = [&](int64_t i0) {
            request_rows(q_ahead, q_base, q.sl, i0, s.Lq, D, i, kk);
            request_rows(do_ahead, do_base, dout.sl, i0, s.Lq, D, i, kk);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {  // the row statistics of queries i0 + 4 kk + reg
                const int64_t at = i0 + 4 * kk + reg, from = min(at, s.Lq - 1);
                const float a = lse_base[from], b = delta_base[from];
                lse_ahead[reg] = at < s.Lq ? a : -INFINITY;
                delta_ahead[reg] = at < s.Lq ? b : 0.0f;
            }
            request_columns(qc_ahead, q_base, q.sl, i0, s.Lq, D, i, kk);
            request_columns(doc_ahead, do_base, dout.sl, i0, s.Lq, D, i, kk);
        };
        request(queries.begin);
        for (int64_t i0 = queries.begin; i0 < queries.end; i0 += kSub) {
            float4 qa[DB], doa[DB];
            float qc[DB][4], doc[DB][4], row_lse[4], row_delta[4];
            copy(qa, q_ahead), copy(doa, do_ahead), copy(qc, qc_ahead), copy(doc, doc_ahead);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) row_lse[reg] = lse_ahead[reg], row_delta[reg] = delta_ahead[reg];
            if (i0 + kSub < queries.end) request(i0 + kSub);  // in flight across this sub-tile's MFMAs
            // the lane ends with key jk against queries i0 + 4 kk + reg
            const native_float4 st = score_product(qa, kb);
            const native_float4 dp = score_product(doa, vb);
            float p[4], ds[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t iq = i0 + 4 * kk + reg;
                p[reg] = ds[reg] = 0.0f;
                if (iq < s.Lq && jk < s.Lk) {
                    p[reg] = probability(band.score(st[reg], s.scale, n, h, iq, jk, s.Lq), row_lse[reg]);
                    if (p[reg] != 0.0f) ds[reg] = p[reg] * (dp[reg] - row_delta[reg]) * s.scale;
                }
            }
            accumulate(acc_v, doc, p);   // dV^T += dout^T P
            accumulate(acc_k, qc, ds);   // dK^T += Q^T dS
        }
        if (jk < s.Lk) {
            store_own_row(dk + ((n * rows_out + (jk - key_from)) * s.H + h) * D, acc_k, kk, D);
            store_own_row(dv + ((n * rows_out + (jk - key_from)) * s.H + h) * D, acc_v, kk, D);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- host
template <int DB>
int launch_band_bwd_mfma(const Rows &q, const Rows &k, const Rows &v, const Rows &o, const Rows &dout, const float *lse, const Band &band,
                         float *dq, float *dk, float *dv, float *delta, const Shape &s, int64_t key_from, int cus, int64_t q_tiles,
                         int64_t k_tiles, void *stream) {
    const int64_t nh = s.N * s.H;
    const auto grid = [&](int64_t items, bool key_major) {
        const int64_t groups = ceil_div(items, int64_t(kWavesPerBlock)), resident = int64_t(band_bwd_groups_per_cu(DB, key_major)) * cus;
        return dim3{uint32_t(groups < resident ? groups : resident)};
    };
    hipLaunchKernelGGL((band_sdpa_bwd_dq_mfma_kernel<DB>), grid(nh * q_tiles, false), dim3{kBlock}, 0, as_stream(stream), q, k, v, o, dout, lse,
                       band, dq, delta, s, q_tiles, nh * q_tiles);
    if (const int status = launch_status()) return status;
    hipLaunchKernelGGL((band_sdpa_bwd_dkv_mfma_kernel<DB>), grid(nh * k_tiles, true), dim3{kBlock}, 0, as_stream(stream), q, k, v, dout, lse,
                       delta, band, dk, dv, s, key_from, k_tiles, nh * k_tiles);
    return launch_status();
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_band_sdpa_bwd_mfma_supported(int64_t Lq, int64_t W, int64_t D) {
    return Lq >= 2 && W >= 1 && D >= 4 && D <= CUSRL_MAX_SDPA_HEAD_DIM && D % 4 == 0;  // (Lq == 1 stays with the VALU backward)
}

extern "C" int cusrl_band_sdpa_bwd_mfma(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                        int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                                        const int32_t *q_segment, const float *alibi_slopes, float scale, const float *out, const float *lse,
                                        const float *dout, int64_t dout_stride_n, int64_t dout_stride_l, int64_t key_grad_from, float *dq,
                                        float *dk, float *dv, float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D,
                                        void *stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || !valid_band_sizes(N, H, Lq, W, D) || key_grad_from < 0 ||
        key_grad_from > W)
        return CUSRL_E_INVALID;
    if (!band_sizes_fit(N, H, Lq, W, D) || !cusrl_band_sdpa_bwd_mfma_supported(Lq, W, D)) return CUSRL_E_UNSUPPORTED;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Rows ro{out, Lq * H * D, H * D}, rdo{dout, dout_stride_n, dout_stride_l};
    if (!rows_vectorise({rq, rk, rv, ro, rdo}, int(D)) || !aligned(dq, 16) || !aligned(dk, 16) || !aligned(dv, 16)) return CUSRL_E_UNSUPPORTED;
    const int64_t q_tiles = ceil_div(Lq, kOwn), k_tiles = ceil_div(Lq + W - key_grad_from, kOwn);
    if (N * H > INT64_MAX / q_tiles || N * H > INT64_MAX / k_tiles) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!workspace) return CUSRL_E_INVALID;
    const Band band{key_valid, q_segment, alibi_slopes, W};
    const Shape shape{N, H, Lq, Lq + W, int(D), scale};
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
#define CUSRL_BAND_BWD_MFMA(DB) \
    launch_band_bwd_mfma<DB>(rq, rk, rv, ro, rdo, lse, band, dq, dk, dv, workspace, shape, key_grad_from, cus, q_tiles, k_tiles, stream)
    const int status = D <= 16 ? CUSRL_BAND_BWD_MFMA(1) : D <= 32 ? CUSRL_BAND_BWD_MFMA(2) : D <= 64 ? CUSRL_BAND_BWD_MFMA(4) : CUSRL_BAND_BWD_MFMA(8);
#undef CUSRL_BAND_BWD_MFMA
    return status;
}
