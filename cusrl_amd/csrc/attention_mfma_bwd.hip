// Dense scaled dot-product attention, backward, on v_mfma_f32_16x16x4_f32 ("The backward on the matrix cores"): the
// formulas and the visibility of cusrl_sdpa_bwd (include/cusrl_hip.h; `Mask` of attention_common.hpp, passed by value) in the
// formulation of attention_mfma.hip, for the shapes where the VALU passes of attention.hip walk D-long fmaf chains out of LDS lane
// by lane.  Opt-in (ops.sdpa(matrix_core_backward=True)): the sums run in another order, so the bits are not that kernel's.
//
// Formulation (transposed, as in attention_mfma.hip).  Lane (i = m = lane & 15, kk = lane >> 4) supplies A[i][kk] and B[kk][m] and
// holds D[4 kk + reg][m].  A wave owns 16 rows of one (n, h) and a lane is bound to ONE of them, row r0 + m: queries in the first
// launch, keys in the second.  Both launches run the same two steps per 16-row sub-tile of the streamed side:
//   * two score-shaped products (score_product): the A operands of d-block t are one float4 of a streamed row out of LDS
//     (row i, columns 16 t + 4 kk .. + 3), the B operands one float4 of a row the lane holds in registers.  Afterwards the lane has
//     the product of ITS row against streamed rows 4 kk + reg of the sub-tile;
//   * p = probability(s, lse) and ds = p (dp - delta) scale are per-lane arithmetic on those four registers and never leave them;
//   * the accumulations (accumulate) have the forward's P.V shape: the B operand of MFMA j is the lane's own register j, the A
//     operand is streamed[4 kk + j][16 t + i] out of LDS; ceil(D / 16) accumulator tiles per output and no rescaling.
// Query-major launch (dq, delta): the lane holds its Q and dout rows (DB float4 each), lse and delta; K and V stream.
//   S^T = K Q^T (A: K row, B: Q), dP^T = V dout^T (A: V row, B: dout), dQ^T += K^T dS^T (A: K[k0 + 4 kk + j][16 t + i], B: ds[j]).
//   delta_i = sum_d dout_id out_id: the lane's own float4s of dout and out, d = 16 t + 4 kk + e in the order t, e, then lanes ^ 16
//   and ^ 32 (a + b on both partners: the four lanes of a query hold the same bits); the kk == 0 lanes store it to the workspace.
// Key-major launch (dk, dv): the lane holds its K and V rows; Q and dout stream with the tile's 32 lse and delta beside them.
//   S = Q K^T (A: Q row, B: K), dP = dout V^T (A: dout row, B: V), dV^T += dout^T P and dK^T += Q^T dS (A: dout / Q
//   [i0 + 4 kk + j][16 t + i], B: p[j] / ds[j]).  A query at or past Lq scores -inf and adds exact zeros.
// Either way lane (m, kk) stores row r0 + m, columns 16 t + 4 kk .. + 3, as one float4 per tile.  D % 16 != 0 is zero-padded inside
// the last d-block in A and in B, in registers.  p is `probability` as attention.hip writes it: a masked pair or a row with
// lse = -inf gives p = 0 and ds = 0 exactly, exp(-inf - (-inf)) is never evaluated; a key no query sees gets dk = dv = 0 exactly.
//
// Work split.  A workgroup is 4 waves = 64 owned rows; the streamed side goes through LDS in tiles of 32 rows (two sub-tiles),
// staged ONCE per workgroup.  The next tile's global loads are issued into registers in front of the current tile's MFMAs and
// written to LDS behind the next barrier (one buffer, two barriers per tile).  Every wave passes every barrier, so the workgroup
// walks the union of its waves' spans: Mask::keys of its last wave, Mask::queries of its first; a wave whose sub-tile is wholly
// masked adds exact zeros.
//
// Item order.  Work items N * H * ceil(L / 64), the grid G = min(items, c * CUs) workgroups.  Positions are dealt serpentine:
// workgroup b takes position r G + b in even rounds r and r G + (G - 1 - b) in odd ones, and position p is (n, h) = p % (N H) of
// tile slot p / (N H), with the slots ordered longest span first under a causal mask (the last query tile, the first key tile).
// So a round holds tiles of about one length, the lengths fall from round to round, and a workgroup that got the longer end of one
// round gets the shorter end of the next.  The order decides who computes a row, never a bit of it.
//
// LDS rows have a stride of ld = D | 4 floats (ld / 4 odd); both read patterns are the forward's.  (a) score_product reads 16 bytes
// per lane at rows i = 0 .. 15 of one column: i * ld / 4 mod 16 takes 16 different values, so the 16 lanes of a kk group cover the
// 64 banks once.  (b) accumulate reads 4 bytes per lane, 16 lanes along d and the four kk groups 4 rows apart: 4 * ld = 16 * odd
// floats, so the groups start at banks 0, 16, 32, 48 in some order.  The key-major launch reads two tensors per step; each read is
// one such pattern on its own region.  The 32 lse / delta values behind them are read four consecutive floats per kk group, the
// same address across a group's 16 lanes (a broadcast).
//
// Determinism: one owning lane per output element, one fixed summation order per element (tile, sub-tile, MFMA), no atomics and no
// sums across workgroups.  A dq row's bits depend on its own row of q / dout / out / lse / mask, on the keys and on D; a dk / dv
// row's bits depend on its own key row, on the queries and on D - not on lane, wave, workgroup or batch position.
#include "attention_common.hpp"

namespace cusrl {
namespace {

constexpr int kRows = kWavesPerBlock * kOwn;  // rows a workgroup owns: 16 per wave
constexpr int kSub = 16;                       // streamed rows of one MFMA sub-tile (kTile = 32 are staged per step)

// Workgroups a CU holds at once, one wave each on its four SIMDs = the kernel's waves per SIMD by its registers
// (profiles/sdpa_mfma/resource_usage.txt: query-major 129 / 143 / 194 / 294, key-major 157 / 174 / 234 / 338 of 512 for
// DB = 1 / 2 / 4 / 8); LDS (at most 34 KiB of 160) allows four.
constexpr int groups_per_cu(int DB, bool key_major) { return DB == 1 ? 3 : DB == 2 ? (key_major ? 2 : 3) : DB == 4 ? 2 : 1; }

constexpr int loads_per_thread(int DB) { return DB >= 2 ? DB / 2 : 1; }  // float4 per thread, tensor and tile: 32 rows of <= 4 DB float4

__device__ __forceinline__ float4 zero4() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

// The (n, h, tile) of workgroup `b`'s round `r` (file header, "Item order"), or false where the round has no position for it.
__device__ __forceinline__ bool item_of(int64_t r, int64_t items, int64_t nh_count, int64_t &nh, int64_t &slot) {
    const int64_t G = gridDim.x, b = blockIdx.x, at = r * G + ((r & 1) ? G - 1 - b : b);
    if (at >= items) return false;
    slot = at / nh_count, nh = at - slot * nh_count;
    return true;
}

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

// This thread's slots of a staged tile: (row, column) of float4 number threadIdx.x + 256 u; rows at or past kTile do not exist.
template <int kLoads>
struct Slots {
    int row[kLoads], col[kLoads];
    __device__ __forceinline__ Slots(int per_row) {
#pragma unroll
        for (int u = 0; u < kLoads; ++u) {
            const int at = threadIdx.x + u * kBlock;
            row[u] = at / per_row;
            col[u] = (at - row[u] * per_row) * 4;
        }
    }
};

// Rows l0 .. l0 + 31 of two tensors of L rows into registers; rows at or past L are zeros (unpredicated loads from clamped
// addresses, then a select).
template <int kLoads>
__device__ __forceinline__ void request_tiles(float4 (&x)[kLoads], float4 (&y)[kLoads], const float *a, int64_t a_sl, const float *b,
                                              int64_t b_sl, int64_t l0, int64_t L, const Slots<kLoads> &slots) {
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
        const int64_t l = l0 + min(slots.row[u], kTile - 1), from = min(l, L - 1);
        const float4 p = *reinterpret_cast<const float4 *>(a + from * a_sl + slots.col[u]);
        const float4 q = *reinterpret_cast<const float4 *>(b + from * b_sl + slots.col[u]);
        x[u] = l < L ? p : zero4();
        y[u] = l < L ? q : zero4();
    }
}

template <int kLoads>
__device__ __forceinline__ void stage_tiles(float *sa, float *sb, int ld, const float4 (&x)[kLoads], const float4 (&y)[kLoads],
                                            const Slots<kLoads> &slots) {
#pragma unroll
    for (int u = 0; u < kLoads; ++u)
        if (slots.row[u] < kTile) {
            *reinterpret_cast<float4 *>(sa + slots.row[u] * ld + slots.col[u]) = x[u];
            *reinterpret_cast<float4 *>(sb + slots.row[u] * ld + slots.col[u]) = y[u];
        }
}

// sum_d rows[i][d] own[d] of a 16-row sub-tile at `rows`: the lane ends with its own row against sub-tile rows 4 kk + reg.
template <int DB>
__device__ __forceinline__ native_float4 score_product(const float *rows, int ld, int D, int i, int kk, const float4 (&own)[DB]) {
    native_float4 acc{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        const int d = 16 * t + 4 * kk;
        const float4 a = d < D ? *reinterpret_cast<const float4 *>(rows + i * ld + d) : zero4();
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, own[t].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, own[t].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, own[t].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, own[t].w, acc, 0, 0, 0);
    }
    return acc;
}

// acc[t][reg] (column 16 t + 4 kk + reg of the lane's row) += sum_j rows[4 kk + j][16 t + i] w[j] over the 16-row sub-tile at `rows`.
template <int DB>
__device__ __forceinline__ void accumulate(native_float4 (&acc)[DB], const float *rows, int ld, int D, int i, int kk, const float (&w)[4]) {
#pragma unroll
    for (int t = 0; t < DB; ++t) {
        const int d = 16 * t + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = d < D ? rows[(4 * kk + j) * ld + d] : 0.0f;
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w[j], acc[t], 0, 0, 0);
        }
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

// -------------------------------------------------------------------------------------------- query-major: dq and delta
// DB: 16-wide d-blocks (D <= 16 DB, D % 4 == 0).
template <int DB>
__global__ __launch_bounds__(kBlock) void sdpa_bwd_dq_mfma_kernel(Rows q, Rows k, Rows v, Rows o, Rows dout, const float *lse, Mask vis,
                                                                  float *dq, float *delta, Shape s, int64_t q_tiles, int64_t items) {
    extern __shared__ float4 lds[];
    constexpr int kLoads = loads_per_thread(DB);
    const int D = s.D, ld = D | 4;
    float *sk = reinterpret_cast<float *>(lds), *sv = sk + kTile * ld;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const Slots<kLoads> slots(D / 4);
    const int64_t nh_count = s.N * s.H, rounds = (items + gridDim.x - 1) / gridDim.x;

    for (int64_t r = 0; r < rounds; ++r) {
        int64_t nh, slot;
        if (!item_of(r, items, nh_count, nh, slot)) continue;
        const int64_t h = nh % s.H, n = nh / s.H;
        const int64_t q0 = (q_tiles - 1 - slot) * kRows, iq = q0 + wave * kOwn + i;  // the lane's query; the last tile first
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

        const Span keys = vis.keys(q0 + kRows - kOwn, s);  // the span of the workgroup's last wave covers every wave's
        const float *k_base = k.p + n * k.sn + h * D, *v_base = v.p + n * v.sn + h * D;
        float4 k_ahead[kLoads], v_ahead[kLoads];
        request_tiles(k_ahead, v_ahead, k_base, k.sl, v_base, v.sl, keys.begin, s.Lk, slots);
        for (int64_t k0 = keys.begin; k0 < keys.end; k0 += kTile) {
            __syncthreads();  // the previous tile's readers are done
            stage_tiles(sk, sv, ld, k_ahead, v_ahead, slots);
            __syncthreads();
            if (k0 + kTile < keys.end) request_tiles(k_ahead, v_ahead, k_base, k.sl, v_base, v.sl, k0 + kTile, s.Lk, slots);  // in flight across the MFMAs
#pragma unroll
            for (int ks = 0; ks < kTile; ks += kSub) {
                // the lane ends with query iq against keys k0 + ks + 4 kk + reg
                const native_float4 st = score_product(sk + ks * ld, ld, D, i, kk, qb);
                const native_float4 dp = score_product(sv + ks * ld, ld, D, i, kk, dob);
                float ds[4];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int64_t j = k0 + ks + 4 * kk + reg;
                    ds[reg] = 0.0f;
                    if (iq < s.Lq && j < s.Lk) {
                        const float p = probability(vis.score(st[reg], s.scale, n, h, iq, j, s.Lq), row_lse);
                        if (p != 0.0f) ds[reg] = p * (dp[reg] - row_delta) * s.scale;
                    }
                }
                accumulate(acc, sk + ks * ld, ld, D, i, kk, ds);  // dQ^T += K^T dS^T: ds is the B operand where it is
            }
        }
        if (iq < s.Lq) store_own_row(dq + ((n * s.Lq + iq) * s.H + h) * D, acc, kk, D);
    }
}

// ------------------------------------------------------------------------------------------------ key-major: dk and dv
template <int DB>
__global__ __launch_bounds__(kBlock) void sdpa_bwd_dkv_mfma_kernel(Rows q, Rows k, Rows v, Rows dout, const float *lse, const float *delta,
                                                                   Mask vis, float *dk, float *dv, Shape s, int64_t k_tiles, int64_t items) {
    extern __shared__ float4 lds[];
    constexpr int kLoads = loads_per_thread(DB);
    const int D = s.D, ld = D | 4;
    float *sq = reinterpret_cast<float *>(lds), *sdo = sq + kTile * ld, *slse = sdo + kTile * ld, *sdelta = slse + kTile;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const Slots<kLoads> slots(D / 4);
    const int64_t nh_count = s.N * s.H, rounds = (items + gridDim.x - 1) / gridDim.x;

    for (int64_t r = 0; r < rounds; ++r) {
        int64_t nh, slot;
        if (!item_of(r, items, nh_count, nh, slot)) continue;
        const int64_t h = nh % s.H, n = nh / s.H;
        const int64_t j0 = slot * kRows, jk = j0 + wave * kOwn + i;  // the lane's key; the first tile first
        const int64_t row = min(jk, s.Lk - 1);
        float4 kb[DB], vb[DB];
        load_own_row(kb, k.p + n * k.sn + row * k.sl + h * D, kk, D);
        load_own_row(vb, v.p + n * v.sn + row * v.sl + h * D, kk, D);
        native_float4 acc_k[DB], acc_v[DB];
#pragma unroll
        for (int t = 0; t < DB; ++t) acc_k[t] = acc_v[t] = native_float4{0.0f, 0.0f, 0.0f, 0.0f};

        const Span queries = vis.queries(j0, s);  // the span of the workgroup's first wave covers every wave's
        const float *q_base = q.p + n * q.sn + h * D, *do_base = dout.p + n * dout.sn + h * D;
        const float *lse_base = lse + nh * s.Lq, *delta_base = delta + nh * s.Lq;
        float4 q_ahead[kLoads], do_ahead[kLoads];
        float lse_ahead = -INFINITY, delta_ahead = 0.0f;  // threads 0 .. 31: the tile's row statistics
        auto request = [&](int64_t i0) {
            request_tiles(q_ahead, do_ahead, q_base, q.sl, do_base, dout.sl, i0, s.Lq, slots);
            if (threadIdx.x < kTile) {
                const int64_t at = i0 + threadIdx.x;
                lse_ahead = at < s.Lq ? lse_base[at] : -INFINITY;
                delta_ahead = at < s.Lq ? delta_base[at] : 0.0f;
            }
        };
        request(queries.begin);
        for (int64_t i0 = queries.begin; i0 < queries.end; i0 += kTile) {
            __syncthreads();  // the previous tile's readers are done
            stage_tiles(sq, sdo, ld, q_ahead, do_ahead, slots);
            if (threadIdx.x < kTile) slse[threadIdx.x] = lse_ahead, sdelta[threadIdx.x] = delta_ahead;
            __syncthreads();
            if (i0 + kTile < queries.end) request(i0 + kTile);  // in flight across this tile's MFMAs
#pragma unroll
            for (int qs = 0; qs < kTile; qs += kSub) {
                // the lane ends with key jk against queries i0 + qs + 4 kk + reg
                const native_float4 st = score_product(sq + qs * ld, ld, D, i, kk, kb);
                const native_float4 dp = score_product(sdo + qs * ld, ld, D, i, kk, vb);
                float p[4], ds[4];
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int at = qs + 4 * kk + reg;
                    const int64_t iq = i0 + at;
                    p[reg] = ds[reg] = 0.0f;
                    if (iq < s.Lq && jk < s.Lk) {
                        p[reg] = probability(vis.score(st[reg], s.scale, n, h, iq, jk, s.Lq), slse[at]);
                        if (p[reg] != 0.0f) ds[reg] = p[reg] * (dp[reg] - sdelta[at]) * s.scale;
                    }
                }
                accumulate(acc_v, sdo + qs * ld, ld, D, i, kk, p);   // dV^T += dout^T P
                accumulate(acc_k, sq + qs * ld, ld, D, i, kk, ds);   // dK^T += Q^T dS
            }
        }
        if (jk < s.Lk) {
            store_own_row(dk + ((n * s.Lk + jk) * s.H + h) * D, acc_k, kk, D);
            store_own_row(dv + ((n * s.Lk + jk) * s.H + h) * D, acc_v, kk, D);
        }
    }
}

// --------------------------------------------------------------------------------------------------------------- host
template <int DB>
int launch_bwd_mfma(const Rows &q, const Rows &k, const Rows &v, const Rows &o, const Rows &dout, const float *lse, const Mask &mask,
                    float *dq, float *dk, float *dv, float *delta, const Shape &s, int cus, int64_t q_tiles, int64_t k_tiles, void *stream) {
    const int64_t nh = s.N * s.H;
    const auto grid = [&](int64_t items, bool key_major) {
        const int64_t resident = int64_t(groups_per_cu(DB, key_major)) * cus;
        return dim3{uint32_t(items < resident ? items : resident)};
    };
    const size_t tiles = size_t(2) * kTile * (s.D | 4) * sizeof(float);  // two streamed tiles: 33 KiB at D = 128
    hipLaunchKernelGGL((sdpa_bwd_dq_mfma_kernel<DB>), grid(nh * q_tiles, false), dim3{kBlock}, tiles, as_stream(stream), q, k, v, o, dout, lse, mask,
                       dq, delta, s, q_tiles, nh * q_tiles);
    if (const int status = launch_status()) return status;
    hipLaunchKernelGGL((sdpa_bwd_dkv_mfma_kernel<DB>), grid(nh * k_tiles, true), dim3{kBlock}, tiles + 2 * kTile * sizeof(float), as_stream(stream),
                       q, k, v, dout, lse, delta, mask, dk, dv, s, k_tiles, nh * k_tiles);
    return launch_status();
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_sdpa_bwd_mfma_supported(int64_t Lq, int64_t Lk, int64_t D) {
    return Lq >= 1 && Lk >= 1 && D >= 4 && D <= CUSRL_MAX_SDPA_HEAD_DIM && D % 4 == 0;
}

extern "C" int cusrl_sdpa_bwd_mfma(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                                   int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const float *out,
                                   const float *lse, const float *dout, int64_t dout_stride_n, int64_t dout_stride_l,
                                   const uint8_t *keep_mask, const float *bias, int64_t mask_stride_n, int64_t mask_stride_h,
                                   int64_t mask_stride_q, int64_t mask_stride_k, int causal, float scale, float *dq, float *dk, float *dv,
                                   float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D, void *stream) {
    if (!q || !k || !v || !out || !lse || !dout || !dq || !dk || !dv || (keep_mask && bias) || !valid_sizes(N, H, Lq, Lk, D))
        return CUSRL_E_INVALID;
    if (!sizes_fit(N, H, Lq, Lk, D) || !cusrl_sdpa_bwd_mfma_supported(Lq, Lk, D)) return CUSRL_E_UNSUPPORTED;
    const Rows rq{q, q_stride_n, q_stride_l}, rk{k, k_stride_n, k_stride_l}, rv{v, v_stride_n, v_stride_l};
    const Rows ro{out, Lq * H * D, H * D}, rdo{dout, dout_stride_n, dout_stride_l};
    if (!rows_vectorise({rq, rk, rv, ro, rdo}, int(D)) || !aligned(dq, 16) || !aligned(dk, 16) || !aligned(dv, 16)) return CUSRL_E_UNSUPPORTED;
    const int64_t q_tiles = ceil_div(Lq, kRows), k_tiles = ceil_div(Lk, kRows);
    if (N * H > INT64_MAX / q_tiles || N * H > INT64_MAX / k_tiles) return CUSRL_E_UNSUPPORTED;
    if (N == 0) return 0;
    if (!workspace) return CUSRL_E_INVALID;
    const Mask mask{keep_mask, bias, mask_stride_n, mask_stride_h, mask_stride_q, mask_stride_k, causal != 0};
    const Shape shape{N, H, Lq, Lk, int(D), scale};
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
#define CUSRL_BWD_MFMA(DB) launch_bwd_mfma<DB>(rq, rk, rv, ro, rdo, lse, mask, dq, dk, dv, workspace, shape, cus, q_tiles, k_tiles, stream)
    const int status = D <= 16 ? CUSRL_BWD_MFMA(1) : D <= 32 ? CUSRL_BWD_MFMA(2) : D <= 64 ? CUSRL_BWD_MFMA(4) : CUSRL_BWD_MFMA(8);
#undef CUSRL_BWD_MFMA
    return status;
}
