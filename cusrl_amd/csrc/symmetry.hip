// Mirror symmetry (cusrl/hook/auxiliary/symmetry.py, cusrl/hook/mdp/observation.py:213-217) as single launches:
//   cusrl_mirror_rows          MirrorDef.__call__ over several fields at once, into strided / offset destinations: the
//                              [R, 2, C] rows of SymmetricDataAugmentation (original half copied, mirrored half through the
//                              table) and the repeated narrow leaves in ONE launch
//   cusrl_mirror_rows_bwd      its gradient, through the inverse table (fixed-order sums per input column)
//   cusrl_mirror_mse_fwd_bwd   MirrorSymmetryLoss: both weighted terms and the gradients wrt both actor outputs in one pass
//   cusrl_symmetrize_mean_var  the symmetric running-statistics update of ObservationNormalization, in place
//   cusrl_symmetric_head_fwd / _bwd / _sample   the head of SymmetricActor over the stacked [2B, A] rows of ONE wrapped pass
// Table (int32, built once on the host, cusrl_amd/hook/auxiliary/symmetry.py): [C_out] forward codes, [C_in + 1] offsets,
// [C_out] inverse codes.  A code is a column index with bit 31 set when the value is negated.  A negation is a sign flip
// (exact, signed zeros included), which is what `x * -1` is for every non-NaN x.
#include "common.hpp"
#include "loss_reduce.hpp"

namespace cusrl {

constexpr uint32_t kFlipBit = 0x80000000u;
constexpr int kMirrorTile = 4096;  // elements per block of the row kernels (whole rows; a wider row takes a block alone)

__device__ __forceinline__ float apply_code(float v, uint32_t code) { return (code & kFlipBit) ? -v : v; }
__device__ __forceinline__ int code_column(uint32_t code) { return int(code & ~kFlipBit); }

struct MirrorTable {
    cusrl_mirror_field_t f[CUSRL_MAX_MIRROR_FIELDS];
};

__host__ __device__ inline int64_t mirror_rows_per_block(int64_t width) { return width >= kMirrorTile ? 1 : kMirrorTile / width; }

// blockIdx.y = field, blockIdx.x = a tile of whole rows.  Thread t of the tile writes element t (coalesced stores); its load
// is a gather inside the same row, which the row's cache lines serve.
__global__ __launch_bounds__(kBlock) void mirror_rows_kernel(MirrorTable table, int64_t rows) {
    const cusrl_mirror_field_t &f = table.f[blockIdx.y];
    const int64_t width = f.width, rpb = mirror_rows_per_block(width);
    const int64_t row0 = int64_t(blockIdx.x) * rpb;
    if (row0 >= rows) return;
    const int64_t nrows = rows - row0 < rpb ? rows - row0 : rpb;
    const uint32_t n = uint32_t(nrows * width), w = uint32_t(width);
    const uint32_t *codes = reinterpret_cast<const uint32_t *>(f.table);
    for (uint32_t e = threadIdx.x; e < n; e += kBlock) {
        const uint32_t r = e / w, c = e - r * w;
        const int64_t row = row0 + r;
        const float *src = f.src + row * f.src_stride;
        float v;
        if (codes) {
            const uint32_t code = codes[c];
            v = apply_code(src[code_column(code)], code);
        } else {
            v = src[c];
        }
        f.dst[row * f.dst_stride + f.dst_offset + c] = v;
    }
}

// grad_in[r, i] = sum over the output columns j that read column i, in increasing j, of sign_j * grad_out[r, j]
__global__ __launch_bounds__(kBlock) void mirror_rows_bwd_kernel(const float *__restrict__ grad_out, int64_t go_stride,
                                                                 float *__restrict__ grad_in, int64_t gi_stride,
                                                                 const uint32_t *__restrict__ table, int c_in, int c_out,
                                                                 int64_t rows) {
    const int64_t rpb = mirror_rows_per_block(c_in), row0 = int64_t(blockIdx.x) * rpb;
    if (row0 >= rows) return;
    const int64_t nrows = rows - row0 < rpb ? rows - row0 : rpb;
    const uint32_t n = uint32_t(nrows * c_in), w = uint32_t(c_in);
    const uint32_t *offsets = table + c_out, *inverse = table + c_out + c_in + 1;
    for (uint32_t e = threadIdx.x; e < n; e += kBlock) {
        const uint32_t r = e / w, i = e - r * w;
        const int64_t row = row0 + r;
        const float *g = grad_out + row * go_stride;
        float acc = 0.0f;
        for (uint32_t k = offsets[i]; k < offsets[i + 1]; ++k) {
            const uint32_t code = inverse[k];
            acc += apply_code(g[code_column(code)], code);
        }
        grad_in[row * gi_stride + i] = acc;
    }
}

// torch.sign: the gradient of abs (0 at 0, NaN stays NaN)
__device__ __forceinline__ float sign_of(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : x); }

// One pass over [B, A]: element (b, j) adds its squared differences to the fp64 partials and writes d mu[b, j] and
// d sigma[b, j]; as (b, i) it writes d mu~[b, i] and d sigma~[b, i], re-deriving the differences of the output columns that
// read column i (from the same row, in cache) in increasing j.  A std vector ([A], repeat_std) is one row, done by block 0.
__global__ __launch_bounds__(kBlock) void mirror_mse_kernel(const float *__restrict__ mu, const float *__restrict__ mu_m,
                                                            const float *__restrict__ sigma, const float *__restrict__ sigma_m,
                                                            int std_vector, const uint32_t *__restrict__ table, int64_t B,
                                                            int A, float g_mean, float g_std, float *__restrict__ d_mu,
                                                            float *__restrict__ d_mu_m, float *__restrict__ d_sigma,
                                                            float *__restrict__ d_sigma_m, double *__restrict__ partials,
                                                            ScaledLoss<2> scales, float *__restrict__ loss_out) {
    __shared__ double scratch[kWavesPerBlock];
    const uint32_t *offsets = table + A, *inverse = table + 2 * A + 1;
    const int64_t n = B * A, stride = int64_t(gridDim.x) * kBlock;
    const bool std_matrix = sigma != nullptr && !std_vector;
    double acc_mean = 0.0, acc_std = 0.0;
    for (int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
        const int64_t b = e / A;
        const int j = int(e - b * A);
        const float *m = mu + b * A, *mm = mu_m + b * A;
        const uint32_t code = table[j];
        const float d = m[j] - apply_code(mm[code_column(code)], code);
        acc_mean += double(d * d);
        d_mu[e] = g_mean * d;
        float acc = 0.0f;
        for (uint32_t k = offsets[j]; k < offsets[j + 1]; ++k) {
            const uint32_t c = inverse[k];
            const int jj = code_column(c);
            const float dd = m[jj] - apply_code(mm[j], c);
            acc += apply_code(-(g_mean * dd), c);
        }
        d_mu_m[e] = acc;
        if (std_matrix) {
            const float *s = sigma + b * A, *sm = sigma_m + b * A;
            const float t = s[j] - fabsf(sm[code_column(code)]);
            acc_std += double(t * t);
            d_sigma[e] = g_std * t;
            float a2 = 0.0f;
            for (uint32_t k = offsets[j]; k < offsets[j + 1]; ++k) {
                const int jj = code_column(inverse[k]);
                a2 += -(g_std * (s[jj] - fabsf(sm[j])));
            }
            d_sigma_m[e] = a2 * sign_of(sm[j]);
        }
    }
    if (sigma != nullptr && std_vector && blockIdx.x == 0) {
        for (int j = threadIdx.x; j < A; j += kBlock) {
            const uint32_t code = table[j];
            const float t = sigma[j] - fabsf(sigma_m[code_column(code)]);
            acc_std += double(t * t);
            d_sigma[j] = g_std * t;
            float a2 = 0.0f;
            for (uint32_t k = offsets[j]; k < offsets[j + 1]; ++k) {
                const int jj = code_column(inverse[k]);
                a2 += -(g_std * (sigma[jj] - fabsf(sigma_m[j])));
            }
            d_sigma_m[j] = a2 * sign_of(sigma_m[j]);
        }
    }
    publish_loss_sums<2>({acc_mean, acc_std}, scratch, partials, loss_out, scales);
}

// observation.py:213-217 in fp32, one rounding per operation and in the reference's order:
//   mm = M(mean); mv = |M(var)|; var = (var + mv) / 2 + (mean - mm)^2 / 4; mean = (mean + mm) / 2
// Every new value reads other columns of the old ones: all of them are staged in LDS before any is stored.
__global__ __launch_bounds__(kBlock) void symmetrize_mean_var_kernel(float *__restrict__ mean, float *__restrict__ var,
                                                                     const uint32_t *__restrict__ table, int C) {
    extern __shared__ float staged[];  // [2 C]: new mean, new var
    for (int j = threadIdx.x; j < C; j += kBlock) {
        const uint32_t code = table[j];
        const int i = code_column(code);
        const float m = mean[j], v = var[j];
        const float mm = apply_code(mean[i], code), mv = fabsf(apply_code(var[i], code));
        const float diff = __fsub_rn(m, mm);
        staged[j + C] = __fadd_rn(__fmul_rn(__fadd_rn(v, mv), 0.5f), __fmul_rn(__fmul_rn(diff, diff), 0.25f));
        staged[j] = __fmul_rn(__fadd_rn(m, mm), 0.5f);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < C; j += kBlock) {
        mean[j] = staged[j];
        var[j] = staged[j + C];
    }
}

// ---- the head of a symmetric actor (SymmetricActor, symmetry.py:396-456): the wrapped actor ran ONCE over the stacked rows
// [2B, A] (original rows first, mirrored rows second); these combine the two halves.  A std vector ([A], NormalDist) is one
// row that is both halves.  Every operation is one fp32 rounding in torch's order: (o + M(m)) / 2 as add, then * 0.5 (exact).
__device__ __forceinline__ float head_mean(const float *o, const float *m, int j, uint32_t code) {
    return __fmul_rn(__fadd_rn(o[j], apply_code(m[code_column(code)], code)), 0.5f);
}
__device__ __forceinline__ float head_std(const float *o, const float *m, int j, uint32_t code) {
    return __fmul_rn(__fadd_rn(o[j], fabsf(m[code_column(code)])), 0.5f);  // |M(x)| = |x|: the flip does not matter
}

// Element (b, j) per thread, grid-strided: coalesced stores, the gather stays inside the mirrored row.
__global__ __launch_bounds__(kBlock) void symmetric_head_fwd_kernel(const float *__restrict__ mean2, const float *__restrict__ std2,
                                                                    int std_vector, const uint32_t *__restrict__ table, int64_t B,
                                                                    int A, float *__restrict__ mean_out,
                                                                    float *__restrict__ std_out) {
    const uint32_t n = uint32_t(B * A), w = uint32_t(A), stride = gridDim.x * kBlock;
    for (uint32_t e = blockIdx.x * kBlock + threadIdx.x; e < n; e += stride) {
        const uint32_t b = e / w, j = e - b * w;
        const uint32_t code = table[j];
        const float *mo = mean2 + size_t(b) * w;
        mean_out[e] = head_mean(mo, mo + n, int(j), code);
        const float *so = std_vector ? std2 : std2 + size_t(b) * w;
        std_out[e] = head_std(so, std_vector ? so : so + n, int(j), code);
    }
}

// The combine + Normal.rsample with the caller's eps + Normal.log_prob summed over A.  One lane per row (rollout.hip's shape:
// rows are short and the batch is one env step); the row's log-prob accumulates in fp64, nothing else stays live across columns.
__global__ __launch_bounds__(kBlock) void symmetric_head_sample_kernel(const float *__restrict__ mean2, const float *__restrict__ std2,
                                                                       int std_vector, const float *__restrict__ eps,
                                                                       const uint32_t *__restrict__ table, int64_t B, int A,
                                                                       float *__restrict__ action, float *__restrict__ logp,
                                                                       float *__restrict__ mean_out, float *__restrict__ std_out) {
    const int64_t b = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (b >= B) return;
    const int64_t row = b * A, half = B * A;
    const float *mo = mean2 + row, *so = std_vector ? std2 : std2 + row;
    const float *mm = mo + half, *sm = std_vector ? so : so + half;
    double acc = 0.0;
    for (int j = 0; j < A; ++j) {
        const uint32_t code = table[j];
        const float m = head_mean(mo, mm, j, code), s = head_std(so, sm, j, code);
        const float a = __fadd_rn(m, __fmul_rn(s, eps[row + j]));
        const double d = double(a) - double(m), sd = double(s);
        acc += -(d * d) / (2.0 * sd * sd) - log(sd) - 0.918938533204672741780329736406;
        mean_out[row + j] = m;
        std_out[row + j] = s;
        action[row + j] = a;
    }
    logp[b] = float(acc);
}

// One term of d std_m[i]: output column (code) read input column i whose value is s.  torch's order: g / 2, times sign(M(s)), times
// the mirror's multiplier; the sign as torch evaluates it, (0 < x) - (x < 0): +0 for either zero.
__device__ __forceinline__ float head_std_term(float g, float s, uint32_t code) {
    const float m = apply_code(s, code), sgn = float(0.0f < m) - float(m < 0.0f);
    return apply_code(__fmul_rn(__fmul_rn(g, 0.5f), sgn), code);
}

// blockIdx.y < elementwise_planes: element (b, i) per thread over those planes' blocks — d_o[b, i] = g / 2 and d_m[b, i], the
// inverse list's terms in increasing output column (the order of mirror_rows_bwd_kernel).  The planes behind them take one
// column sum each — the head's bias gradient (d_bias != NULL: A planes), then a std vector's gradient (A planes): a column's
// blocks add d_o + d_m ROW BY ROW in fp64 and publish like a loss pass (loss_reduce.hpp).  Pairing the halves per row is what
// makes the bias gradient of a column that mirrors onto itself with a flip exactly 0 (g / 2 - g / 2 in every row), as the
// reference's two passes have it; one fp32 column sum over the 2B stacked rows leaves a rounding residue there.
__global__ __launch_bounds__(kBlock) void symmetric_head_bwd_kernel(const float *__restrict__ g_mean, const float *__restrict__ g_std,
                                                                    const float *__restrict__ std2, int std_vector,
                                                                    const uint32_t *__restrict__ table, int64_t B, int A,
                                                                    int elementwise_planes, float *__restrict__ d_mean2,
                                                                    float *__restrict__ d_std2, float *__restrict__ d_bias,
                                                                    double *__restrict__ partials) {
    __shared__ double scratch[kWavesPerBlock];
    const uint32_t *offsets = table + A, *inverse = table + 2 * A + 1;
    const uint32_t w = uint32_t(A);
    if (int(blockIdx.y) < elementwise_planes) {
        const uint32_t n = uint32_t(B * A), stride = uint32_t(elementwise_planes) * gridDim.x * kBlock;
        const bool std_matrix = g_std != nullptr && !std_vector;
        for (uint32_t e = (blockIdx.y * gridDim.x + blockIdx.x) * kBlock + threadIdx.x; e < n; e += stride) {
            const uint32_t b = e / w, i = e - b * w;
            const uint32_t first = offsets[i], last = offsets[i + 1];
            if (g_mean != nullptr) {
                const float *g = g_mean + size_t(b) * w;
                d_mean2[e] = __fmul_rn(g[i], 0.5f);
                float acc = 0.0f;
                for (uint32_t k = first; k < last; ++k) {
                    const uint32_t c = inverse[k];
                    acc += apply_code(__fmul_rn(g[code_column(c)], 0.5f), c);
                }
                d_mean2[n + e] = acc;
            }
            if (std_matrix) {
                const float *g = g_std + size_t(b) * w;
                const float s = std2[n + e];
                d_std2[e] = __fmul_rn(g[i], 0.5f);
                float acc = 0.0f;
                for (uint32_t k = first; k < last; ++k) {
                    const uint32_t c = inverse[k];
                    acc += head_std_term(g[code_column(c)], s, c);
                }
                d_std2[n + e] = acc;
            }
        }
        return;
    }
    const int column = int(blockIdx.y) - elementwise_planes;
    const bool of_bias = d_bias != nullptr && column < A;
    const int i = of_bias || d_bias == nullptr ? column : column - A;
    const uint32_t first = offsets[i], last = offsets[i + 1];
    const float *g0 = of_bias ? g_mean : g_std;
    const float s = of_bias ? 0.0f : std2[i];
    double acc[1] = {0.0};
    for (int64_t b = int64_t(blockIdx.x) * kBlock + threadIdx.x; b < B; b += int64_t(gridDim.x) * kBlock) {
        const float *g = g0 + b * A;
        double row = double(__fmul_rn(g[i], 0.5f));
        for (uint32_t k = first; k < last; ++k) {
            const uint32_t c = inverse[k];
            const int jj = code_column(c);
            row += double(of_bias ? apply_code(__fmul_rn(g[jj], 0.5f), c) : head_std_term(g[jj], s, c));
        }
        acc[0] += row;
    }
    publish_loss_sums<1>(acc, scratch, partials + size_t(column) * gridDim.x, of_bias ? d_bias + i : d_std2 + i,
                         ScaledLoss<1>{{1.0}});
}

// One block per column over the `blocks` partial sums its column's blocks left.
__global__ __launch_bounds__(kBlock) void symmetric_head_columns_finalize_kernel(const double *__restrict__ partials, int blocks,
                                                                                 float *__restrict__ d_bias, int bias_columns,
                                                                                 float *__restrict__ d_std) {
    __shared__ double scratch[kWavesPerBlock];
    const int column = int(blockIdx.x);
    float *out = column < bias_columns ? d_bias + column : d_std + (column - bias_columns);
    finalize_loss_sums<1>(partials + size_t(column) * blocks, blocks, scratch, out, ScaledLoss<1>{{1.0}});
}

// The shape limits of the three entries (include/cusrl_hip.h): 0 invalid, 1 unsupported, 2 fine.
inline int symmetric_head_shape(int64_t B, int64_t A) {
    if (B < 0 || A <= 0) return 0;
    if (A > CUSRL_MAX_SYMMETRIC_HEAD_ACTIONS || B > (int64_t(INT32_MAX) / 2) / A) return 1;
    return 2;
}

inline int64_t elementwise_blocks(int64_t n) {
    const int64_t want = ceil_div(n, kBlock);
    return want > 4096 ? 4096 : want;
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_mirror_rows(const cusrl_mirror_field_t *fields, int n_fields, int64_t rows, void *stream) {
    if (!fields || n_fields <= 0 || rows < 0) return CUSRL_E_INVALID;
    if (n_fields > CUSRL_MAX_MIRROR_FIELDS) return CUSRL_E_TOO_MANY;
    MirrorTable table{};
    int64_t blocks = 0;
    for (int i = 0; i < n_fields; ++i) {
        const cusrl_mirror_field_t &f = fields[i];
        if (f.width <= 0 || f.src_width <= 0) return CUSRL_E_INVALID;
        if (rows > 0 && (!f.src || !f.dst)) return CUSRL_E_INVALID;  // (an empty tensor may have no storage)
        if (f.src_stride < f.src_width || f.dst_offset < 0 || f.dst_stride < f.dst_offset + f.width) return CUSRL_E_INVALID;
        if (!f.table && f.width != f.src_width) return CUSRL_E_INVALID;  // a copy keeps the width
        if (rows > 1 && f.src_stride > (int64_t(1) << 40)) return CUSRL_E_UNSUPPORTED;
        table.f[i] = f;
        const int64_t need = ceil_div(rows, mirror_rows_per_block(f.width));
        if (need > blocks) blocks = need;
    }
    if (rows == 0) return 0;
    if (blocks > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    hipLaunchKernelGGL(mirror_rows_kernel, dim3(uint32_t(blocks), uint32_t(n_fields)), dim3(kBlock), 0, as_stream(stream),
                       table, rows);
    return launch_status();
}

extern "C" int cusrl_mirror_rows_bwd(const float *grad_out, int64_t go_stride, float *grad_in, int64_t gi_stride,
                                     const int32_t *table, int64_t c_in, int64_t c_out, int64_t rows, void *stream) {
    if (!table || c_in <= 0 || c_out <= 0 || rows < 0) return CUSRL_E_INVALID;
    if (rows > 0 && (!grad_out || !grad_in)) return CUSRL_E_INVALID;  // (an empty tensor may have no storage)
    if (go_stride < c_out || gi_stride < c_in) return CUSRL_E_INVALID;
    if (c_in > INT32_MAX / 2 || c_out > INT32_MAX / 2) return CUSRL_E_UNSUPPORTED;
    if (rows == 0) return 0;
    const int64_t blocks = ceil_div(rows, mirror_rows_per_block(c_in));
    if (blocks > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    hipLaunchKernelGGL(mirror_rows_bwd_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), grad_out, go_stride,
                       grad_in, gi_stride, reinterpret_cast<const uint32_t *>(table), int(c_in), int(c_out), rows);
    return launch_status();
}

extern "C" int64_t cusrl_mirror_mse_num_partials(int64_t n) { return loss_blocks(n); }

extern "C" int cusrl_mirror_mse_fwd_bwd(const float *mu, const float *mu_m, const float *sigma, const float *sigma_m,
                                        int std_vector, const int32_t *table, int64_t B, int64_t A, double weight,
                                        float *loss_out, float *d_mu, float *d_mu_m, float *d_sigma, float *d_sigma_m,
                                        double *partials, void *stream) {
    if (B <= 0 || A <= 0 || weight < 0.0) return CUSRL_E_INVALID;
    if (!mu || !mu_m || !table || !loss_out || !d_mu || !d_mu_m || !partials) return CUSRL_E_INVALID;
    if ((sigma == nullptr) != (sigma_m == nullptr)) return CUSRL_E_INVALID;
    if (sigma && (!d_sigma || !d_sigma_m)) return CUSRL_E_INVALID;
    if (A > 65536 || B > (int64_t(1) << 40) / A) return CUSRL_E_UNSUPPORTED;
    const int64_t n = B * A, blocks = loss_blocks(n);
    const double std_count = sigma ? double(std_vector ? A : n) : 1.0;
    const float g_mean = float(2.0 * weight / double(n)), g_std = float(2.0 * weight / std_count);
    const ScaledLoss<2> scales{{weight / double(n), weight / std_count}};
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(mirror_mse_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, s, mu, mu_m, sigma, sigma_m, std_vector,
                       reinterpret_cast<const uint32_t *>(table), B, int(A), g_mean, g_std, d_mu, d_mu_m, d_sigma, d_sigma_m,
                       partials, scales, loss_out);
    return finish_scaled_loss<2>(blocks, partials, scales, loss_out, s);
}

extern "C" int cusrl_symmetrize_mean_var(float *mean, float *var, const int32_t *table, int64_t C, void *stream) {
    if (!mean || !var || !table || C <= 0) return CUSRL_E_INVALID;
    if (C > CUSRL_MAX_SYMMETRIZE_CHANNELS) return CUSRL_E_UNSUPPORTED;
    hipLaunchKernelGGL(symmetrize_mean_var_kernel, dim3(1), dim3(kBlock), size_t(2 * C) * sizeof(float), as_stream(stream),
                       mean, var, reinterpret_cast<const uint32_t *>(table), int(C));
    return launch_status();
}

extern "C" int cusrl_symmetric_head_fwd(const float *mean2, const float *std2, int std_vector, const int32_t *table, int64_t B,
                                        int64_t A, float *mean_out, float *std_out, void *stream) {
    const int shape = symmetric_head_shape(B, A);
    if (shape == 0 || !table) return CUSRL_E_INVALID;
    if (shape == 1) return CUSRL_E_UNSUPPORTED;
    if (B == 0) return 0;
    if (!mean2 || !std2 || !mean_out || !std_out) return CUSRL_E_INVALID;
    hipLaunchKernelGGL(symmetric_head_fwd_kernel, dim3(uint32_t(elementwise_blocks(B * A))), dim3(kBlock), 0, as_stream(stream),
                       mean2, std2, std_vector, reinterpret_cast<const uint32_t *>(table), B, int(A), mean_out, std_out);
    return launch_status();
}

extern "C" int cusrl_symmetric_head_sample(const float *mean2, const float *std2, int std_vector, const float *eps,
                                           const int32_t *table, int64_t B, int64_t A, float *action, float *logp,
                                           float *mean_out, float *std_out, void *stream) {
    const int shape = symmetric_head_shape(B, A);
    if (shape == 0 || !table) return CUSRL_E_INVALID;
    if (shape == 1) return CUSRL_E_UNSUPPORTED;
    if (B == 0) return 0;
    if (!mean2 || !std2 || !eps || !action || !logp || !mean_out || !std_out) return CUSRL_E_INVALID;
    hipLaunchKernelGGL(symmetric_head_sample_kernel, dim3(uint32_t(ceil_div(B, kBlock))), dim3(kBlock), 0, as_stream(stream),
                       mean2, std2, std_vector, eps, reinterpret_cast<const uint32_t *>(table), B, int(A), action, logp,
                       mean_out, std_out);
    return launch_status();
}

extern "C" int64_t cusrl_symmetric_head_num_partials(int64_t B, int64_t A) {
    return symmetric_head_shape(B, A) == 2 ? 2 * A * loss_blocks(B) : 0;  // (the bias columns and a std vector's)
}

extern "C" int cusrl_symmetric_head_bwd(const float *g_mean, const float *g_std, const float *std2, int std_vector,
                                        const int32_t *table, int64_t B, int64_t A, float *d_mean2, float *d_std2, float *d_bias,
                                        double *partials, void *stream) {
    const int shape = symmetric_head_shape(B, A);
    if (shape == 0 || !table) return CUSRL_E_INVALID;
    if (shape == 1) return CUSRL_E_UNSUPPORTED;
    if (B == 0) return 0;  // (an empty tensor may have no storage)
    if ((!g_mean && !g_std) || (g_mean && !d_mean2) || (g_std && (!std2 || !d_std2)) || (d_bias && !g_mean)) return CUSRL_E_INVALID;
    const bool std_columns = g_std && std_vector;
    const int64_t columns = (d_bias ? A : 0) + (std_columns ? A : 0);
    if (columns && !partials) return CUSRL_E_INVALID;
    // with column sums the grid's x extent is their block count; the element-wise part gets as many planes of it as its own
    // block count asks for
    const int64_t want = elementwise_blocks(B * A), blocks = columns ? loss_blocks(B) : want;
    const int64_t planes = g_mean || (g_std && !std_vector) ? ceil_div(want, blocks) : 0;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(symmetric_head_bwd_kernel, dim3(uint32_t(blocks), uint32_t(planes + columns)), dim3(kBlock), 0, s, g_mean,
                       g_std, std2, std_vector, reinterpret_cast<const uint32_t *>(table), B, int(A), int(planes), d_mean2, d_std2,
                       d_bias, partials);
    if (int rc = launch_status()) return rc;
    if (!columns || blocks == 1) return 0;  // each column's one block finalised itself
    hipLaunchKernelGGL(symmetric_head_columns_finalize_kernel, dim3(uint32_t(columns)), dim3(kBlock), 0, s, partials, int(blocks),
                       d_bias, int(d_bias ? A : 0), d_std2);
    return launch_status();
}
