// Running observation statistics for gfx950: masked column mean / variance of one env step,
// Chan merge into the running statistics, and the normalise-and-clamp pass — three launches, no host round trip
// (the reference: ~15 torch launches and a boolean-mask select that synchronises, twice per env step).  Over the same pivots,
// partial rows and merge, AMP's transition preparation for C <= 128 (amp.py:112-128): cusrl_amp_prepare, TWO
// launches instead of cat + index + 2 x (stats, finalize, merge) + 2 x normalise.
//
// One body per computation — what several kernels must agree on bit for bit is a function they all call (running_stats.hpp):
//   shifted_mean_var  float64 shifted sums -> mean, population variance  masked_stats_finalize_kernel, amp_normalize_kernel, merge_and_scale
//   chan_merge<T>     a batch into the running mean / variance           rms_merge_kernel, amp_normalize_kernel (float), merge_and_scale (double)
//   capped_count      the max_count cap of the running count             rms_merge_kernel, amp_normalize_kernel
//   normalize_clamp   (x - mean) / std, then +-clamp                     rms_normalize_kernel, amp_normalize_kernel, prologue_apply, affine
// (merge_and_scale: reward_norm.hip; prologue_apply: deploy.hip, its own switch around the division; affine: column_affine.hip, the
// division alone.)  The SUMMATION ORDERS are not shared: each kernel's folds decide the last bits of its float64 sums.
#include "common.hpp"
#include "running_stats.hpp"

namespace cusrl {

constexpr int kRmsMaxBlocks = 256;

// partials[block][c][{sum, sumsq}] for c < C, partials[block][C][0] = number of selected rows in this block's rows.
// The sums are of x - x[0][c] (row 0's value of the channel, selected or not, the pivot every block reads: shifted_mean_var).
// C < kBlock: lanes keep one channel each (below); C >= kBlock: masked_col_stats_wide_kernel.
__global__ __launch_bounds__(kBlock) void masked_col_stats_kernel(const float *__restrict__ x,
                                                                  const uint8_t *__restrict__ mask, int64_t rows, int C,
                                                                  double *__restrict__ partials) {
    // a lane keeps one channel: its stride over the flat [rows * C] array is a multiple of C
    const int64_t threads = int64_t(gridDim.x) * kBlock;
    const int64_t stride = threads / C * C;
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t E = rows * C;
    const double pivot = double(x[tid % C]);  // rows >= 1 when this kernel runs
    double sum = 0.0, sumsq = 0.0, count = 0.0;
    for (int64_t i = tid < stride ? tid : E; i < E; i += stride) {
        const int64_t row = i / C;
        if (!mask || mask[row]) {
            const double v = double(x[i]) - pivot;  // exact: the difference of two floats fits a double
            sum += v;
            sumsq += v * v;
            count += 1.0;
        }
    }
    __shared__ double red[kBlock][3];
    red[threadIdx.x][0] = sum;
    red[threadIdx.x][1] = sumsq;
    red[threadIdx.x][2] = count;
    __syncthreads();
    // Fold the kBlock / C lanes of every channel in two levels (with 2 .. 12 channels a single loop per channel is a
    // chain of 20 .. 128 dependent LDS reads: 9 us for the toy config's 2-channel observation): `groups` lanes per
    // column take every groups-th lane of that channel, then one lane per column folds the groups.
    const int64_t base = int64_t(blockIdx.x) * kBlock;
    const int columns = C + 1;
    const int groups = kBlock / columns < 16 ? kBlock / columns : 16;  // >= 1 because C < kBlock
    const int column = threadIdx.x % columns, group = threadIdx.x / columns;
    // column c < C folds the lanes of channel c; column C folds the row counts of channel 0's lanes
    const int channel = column < C ? column : 0;
    const int first = int((int64_t(channel) - base % C + C) % C);
    double s = 0.0, q = 0.0, n = 0.0;
    if (group < groups) {
        for (int k = first + group * C; k < kBlock; k += groups * C) {
            s += red[k][0];
            q += red[k][1];
            n += red[k][2];
        }
    }
    __syncthreads();
    if (group < groups) {
        red[threadIdx.x][0] = s;
        red[threadIdx.x][1] = q;
        red[threadIdx.x][2] = n;
    }
    __syncthreads();
    if (threadIdx.x <= C) {
        s = q = n = 0.0;
        for (int g = 0; g < groups; ++g) {
            s += red[g * columns + threadIdx.x][0];
            q += red[g * columns + threadIdx.x][1];
            n += red[g * columns + threadIdx.x][2];
        }
        double *out = partials + (int64_t(blockIdx.x) * (C + 1) + threadIdx.x) * 2;
        if (threadIdx.x < C) {
            out[0] = s;
            out[1] = q;
        } else {
            out[0] = n;
            out[1] = 0.0;
        }
    }
}

// C >= kBlock: block b takes rows b, b + P, ... and its lanes walk the row in windows of kBlock adjacent channels
// (coalesced), each lane summing one channel of the window over the block's rows; same partials layout and pivot.
__global__ __launch_bounds__(kBlock) void masked_col_stats_wide_kernel(const float *__restrict__ x,
                                                                       const uint8_t *__restrict__ mask, int64_t rows,
                                                                       int C, double *__restrict__ partials) {
    double *out = partials + int64_t(blockIdx.x) * (C + 1) * 2;
    for (int c = threadIdx.x; c < C; c += kBlock) {
        const double pivot = double(x[c]);
        double sum = 0.0, sumsq = 0.0, count = 0.0;
        for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
            if (!mask || mask[row]) {
                const double v = double(x[row * C + c]) - pivot;
                sum += v;
                sumsq += v * v;
                count += 1.0;
            }
        }
        out[c * 2] = sum;
        out[c * 2 + 1] = sumsq;
        if (c == 0) {
            out[C * 2] = count;
            out[C * 2 + 1] = 0.0;
        }
    }
}

// One block folds the P block partials: the C + 1 columns (C channels + the row count) are spread over the whole block,
// kBlock / (C + 1) lanes per column each taking every G-th partial, so the serial chain is P / G fp64 loads long instead
// of P (P = 24 .. 256; as a single loop per channel this launch was 15 us inside every captured env step).  C >= kBlock:
// windows of kBlock - 1 channels, each with the count column (re-folded in the same order, so the same n every window).
__global__ __launch_bounds__(kBlock) void masked_stats_finalize_kernel(const double *__restrict__ partials, int P, int C,
                                                                       const float *__restrict__ x,
                                                                       float *__restrict__ mean, float *__restrict__ var,
                                                                       double *__restrict__ count) {
    __shared__ double folded[kBlock][2];
    const int width = C < kBlock ? C : kBlock - 1;  // channels per window
    const int columns = width + 1;                  // + the count column
    const int groups = kBlock / columns;            // >= 1
    const int column = threadIdx.x % columns, group = threadIdx.x / columns;
    for (int c0 = 0; c0 < C; c0 += width) {
        const int w = C - c0 < width ? C - c0 : width;
        const int source = column < width ? c0 + column : C;  // partial column this lane folds
        double s = 0.0, q = 0.0;
        if (group < groups && (column < w || column == width)) {
            for (int p = group; p < P; p += groups) {
                const double2 v = reinterpret_cast<const double2 *>(partials)[int64_t(p) * (C + 1) + source];
                s += v.x;
                q += v.y;
            }
        }
        __syncthreads();  // the previous window's lanes have read `folded`
        folded[threadIdx.x][0] = s;
        folded[threadIdx.x][1] = q;
        __syncthreads();
        if (int(threadIdx.x) < w) {
            const int c = c0 + threadIdx.x;
            double n = 0.0;
            s = q = 0.0;
            for (int g = 0; g < groups; ++g) {
                s += folded[g * columns + threadIdx.x][0];
                q += folded[g * columns + threadIdx.x][1];
                n += folded[g * columns + width][0];
            }
            if (n > 0.0) {
                const MeanVar batch = shifted_mean_var(s, q, n, double(x[c]));
                mean[c] = float(batch.mean);
                var[c] = float(batch.var);
            } else {
                mean[c] = 0.0f;
                var[c] = 1.0f;
            }
            if (c == 0) *count = n;
        }
    }
}

__global__ __launch_bounds__(kBlock) void rms_merge_kernel(float *__restrict__ mean, float *__restrict__ var,
                                                           float *__restrict__ std, double *__restrict__ count,
                                                           const float *__restrict__ batch_mean,
                                                           const float *__restrict__ batch_var,
                                                           const double *__restrict__ batch_count, float eps,
                                                           double max_count, int C) {
    const double w_old_count = *count, w_new_count = *batch_count;
    __syncthreads();  // every lane has read the counts before lane 0 updates them
    if (w_new_count <= 0.0) return;
    for (int c = threadIdx.x; c < C; c += kBlock) {
        chan_merge(mean[c], var[c], w_old_count, batch_mean[c], batch_var[c], w_new_count);
        std[c] = sqrtf(var[c] + eps);
    }
    if (threadIdx.x == 0) *count = capped_count(w_old_count + w_new_count, max_count);
}

__global__ __launch_bounds__(kBlock) void rms_normalize_kernel(const float *__restrict__ x, const float *__restrict__ mean,
                                                               const float *__restrict__ std, float clamp,
                                                               float *__restrict__ out, int64_t E, int C, int vec4) {
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    if (vec4) {  // C % 4 == 0: the 4 elements of a chunk are 4 adjacent channels of one row
        const int64_t n4 = E / 4;
        for (int64_t i = tid; i < n4; i += stride) {
            const int c = int((i * 4) % C);
            const float4 v = reinterpret_cast<const float4 *>(x)[i];
            const float4 m = *reinterpret_cast<const float4 *>(mean + c);
            const float4 s = *reinterpret_cast<const float4 *>(std + c);
            reinterpret_cast<float4 *>(out)[i] =
                make_float4(normalize_clamp(v.x, m.x, s.x, clamp), normalize_clamp(v.y, m.y, s.y, clamp),
                            normalize_clamp(v.z, m.z, s.z, clamp), normalize_clamp(v.w, m.w, s.w, clamp));
        }
    } else {
        for (int64_t i = tid; i < E; i += stride) {
            const int c = int(i % C);
            out[i] = normalize_clamp(x[i], mean[c], std[c], clamp);
        }
    }
}

// --------------------------------------------------------------------------------------------- AMP transition preparation
// Two launches: (A) every block assembles its slice of the agent rows and fetches its slice of the expert rows (raw, into the
// output buffers) and leaves fp64 {sum, sumsq} per channel of both; block 0 also snapshots the running statistics.
// (B) every block folds the <= 64 partial rows itself (L2-resident, fixed order), replays the two Chan merges from the
// snapshot — so no block depends on another block's result — normalises its slice in place; block 0 publishes the new
// running statistics.  (A single-workgroup form of the whole step measured 118 us: one CU's latency chain.)
constexpr int kPrepMaxC = 128;
constexpr int kPrepMaxBlocks = 64;
constexpr int kPrepItems = 8;  // elements per thread and tensor

// workspace layout (doubles): [P][2 tensors][C][2] partial sums, then the snapshot: mean[C], var[C], count, then the
// pivots: agent[C], expert[C].  The sums are of x - pivot (row 0's agent / expert value of the channel, as in masked_col_stats_kernel).
__device__ __forceinline__ int64_t prep_snapshot_offset(int P, int C) { return int64_t(P) * 2 * C * 2; }

// row 0's value of channel c of the agent rows and of the expert rows
__device__ __forceinline__ void prep_pivots(const float *__restrict__ state, const float *__restrict__ next_state,
                                            const int32_t *__restrict__ columns, int K, const float *__restrict__ agent_raw,
                                            const float *__restrict__ dataset, const int64_t *__restrict__ indices,
                                            const float *__restrict__ expert_raw, int C, int c, double &pa, double &pe) {
    const int k = c < K ? c : c - K;
    pa = double(agent_raw ? agent_raw[c] : (c < K ? state : next_state)[columns ? columns[k] : k]);
    pe = double(expert_raw ? expert_raw[c] : dataset[indices[0] * C + c]);
}

__global__ __launch_bounds__(kBlock) void amp_assemble_kernel(
    const float *__restrict__ state, const float *__restrict__ next_state, int state_pitch,
    const int32_t *__restrict__ columns, int K, const float *__restrict__ agent_raw, const float *__restrict__ dataset,
    const int64_t *__restrict__ indices, const float *__restrict__ expert_raw, int E, int C,
    const float *__restrict__ mean, const float *__restrict__ var, const double *__restrict__ count,
    float *__restrict__ agent_out, float *__restrict__ expert_out, double *__restrict__ work) {
    __shared__ double red[kBlock][4];
    const int threads = int(gridDim.x) * kBlock;
    const int stride = threads / C * C;  // a lane stays on one channel (threads >= kBlock > C)
    const int tid = int(blockIdx.x) * kBlock + threadIdx.x;
    double sa = 0.0, qa = 0.0, se = 0.0, qe = 0.0;
    if (tid < stride) {
        const int c = tid % C;
        const int k = c < K ? c : c - K;
        const int col = agent_raw ? 0 : (columns ? columns[k] : k);
        const float *__restrict__ side = c < K ? state : next_state;
        double pa, pe;
        prep_pivots(state, next_state, columns, K, agent_raw, dataset, indices, expert_raw, C, c, pa, pe);
        // rounds of kPrepItems elements: every index, then every row element is requested before the first store (the
        // launch is a chain of dependent memory round trips: index -> dataset row -> store); out-of-range items are clamped
        for (int i0 = tid; i0 < E; i0 += stride * kPrepItems) {
            int idx[kPrepItems], row[kPrepItems];
            int64_t pick[kPrepItems];
            float a[kPrepItems], e[kPrepItems];
#pragma unroll
            for (int j = 0; j < kPrepItems; ++j) {
                idx[j] = min(i0 + j * stride, E - 1);
                row[j] = idx[j] / C;  // 32-bit: E <= 2^20
                if (!expert_raw) pick[j] = indices[row[j]];
            }
#pragma unroll
            for (int j = 0; j < kPrepItems; ++j) {
                // torch.cat([state[..., idx], next_state[..., idx]], -1)  amp.py:116-120;  dataset[randint]  amp.py:160-163
                const int i = row[j] * C + c;  // the clamped item re-reads this lane's channel of the last row
                a[j] = agent_raw ? agent_raw[i] : side[int64_t(row[j]) * state_pitch + col];
                e[j] = expert_raw ? expert_raw[i] : dataset[pick[j] * C + c];
            }
#pragma unroll
            for (int j = 0; j < kPrepItems; ++j) {
                const int i = i0 + j * stride;
                if (i < E) {
                    agent_out[i] = a[j];
                    expert_out[i] = e[j];
                    const double da = double(a[j]) - pa, de = double(e[j]) - pe;
                    sa += da, qa += da * da;
                    se += de, qe += de * de;
                }
            }
        }
    }
    red[threadIdx.x][0] = sa, red[threadIdx.x][1] = qa, red[threadIdx.x][2] = se, red[threadIdx.x][3] = qe;
    __syncthreads();
    // channel c of this block = lanes whose global id is congruent to c mod C
    if (int(threadIdx.x) < C) {
        const int base = int(blockIdx.x) * kBlock;
        const int first = (int(threadIdx.x) - base % C + C) % C;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int l = first; l < kBlock; l += C)
            for (int j = 0; j < 4; ++j) t[j] += red[l][j];
        double *out = work + (int64_t(blockIdx.x) * 2 * C + threadIdx.x) * 2;
        out[0] = t[0], out[1] = t[1];
        out[int64_t(C) * 2] = t[2], out[int64_t(C) * 2 + 1] = t[3];
    }
    if (blockIdx.x == 0) {  // the statistics every block of launch B merges into (nothing in THIS launch writes them)
        double *snap = work + prep_snapshot_offset(int(gridDim.x), C);
        for (int c = threadIdx.x; c < C; c += kBlock) {
            snap[c] = double(mean[c]), snap[C + c] = double(var[c]);
            prep_pivots(state, next_state, columns, K, agent_raw, dataset, indices, expert_raw, C, c, snap[2 * C + 1 + c],
                        snap[3 * C + 1 + c]);
        }
        if (threadIdx.x == 0) snap[2 * C] = *count;
    }
}

__global__ __launch_bounds__(kBlock) void amp_normalize_kernel(const double *__restrict__ work, int P, int E, int C, int rows,
                                                               float eps, double max_count, float clamp,
                                                               float *__restrict__ mean, float *__restrict__ var,
                                                               float *__restrict__ std, double *__restrict__ count,
                                                               float *__restrict__ agent_out, float *__restrict__ expert_out) {
    __shared__ float s_mean[kPrepMaxC], s_std[kPrepMaxC];
    __shared__ double fold[kBlock][4];
    {
        // partial rows spread over the block: lane (group, c) folds rows group, group + G, ...; then one lane per channel
        // folds the G groups — both in fixed order
        const int groups = kBlock / C, c = threadIdx.x % C, group = threadIdx.x / C;
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        if (group < groups)
            for (int p = group; p < P; p += groups) {
                const double *row = work + (int64_t(p) * 2 * C + c) * 2;
                t[0] += row[0], t[1] += row[1];
                t[2] += row[int64_t(C) * 2], t[3] += row[int64_t(C) * 2 + 1];
            }
        for (int j = 0; j < 4; ++j) fold[threadIdx.x][j] = t[j];
    }
    __syncthreads();
    if (int(threadIdx.x) < C) {
        const int c = threadIdx.x, groups = kBlock / C;
        const double *snap = work + prep_snapshot_offset(P, C);
        float m = float(snap[c]), v = float(snap[C + c]);
        double running = snap[2 * C];
        // transition_rms.update(agent); transition_rms.update(expert)   amp.py:122-124 — what masked_stats_finalize_kernel and
        // rms_merge_kernel do per update (population variance; Chan merge, weights count : rows, fp32)
        for (int which = 0; which < 2; ++which) {
            double s = 0.0, q = 0.0;
            for (int g = 0; g < groups; ++g) s += fold[g * C + c][2 * which], q += fold[g * C + c][2 * which + 1];
            const double n = double(rows);
            const MeanVar batch = shifted_mean_var(s, q, n, snap[2 * C + 1 + which * C + c]);
            running = capped_count(chan_merge(m, v, running, float(batch.mean), float(batch.var), n), max_count);
        }
        const float sd = sqrtf(v + eps);
        s_mean[c] = m, s_std[c] = sd;
        if (blockIdx.x == 0) {
            mean[c] = m, var[c] = v, std[c] = sd;
            if (c == 0) *count = running;
        }
    }
    __syncthreads();
    // normalise both with the statistics after BOTH updates   amp.py:125-128, rms.py:198-203
    const int threads = int(gridDim.x) * kBlock;
    const int stride = threads / C * C;
    const int tid = int(blockIdx.x) * kBlock + threadIdx.x;
    if (tid < stride) {
        const float m = s_mean[tid % C], sd = s_std[tid % C];
        for (int i = tid; i < E; i += stride) {
            const float a = normalize_clamp(agent_out[i], m, sd, clamp), e = normalize_clamp(expert_out[i], m, sd, clamp);
            agent_out[i] = a;
            expert_out[i] = e;
        }
    }
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int64_t cusrl_masked_stats_num_partials(int64_t rows, int64_t C) {
    if (rows <= 0 || C <= 0) return 0;
    const int64_t want = ceil_div(rows * C, int64_t(kBlock) * 8);
    return want < 1 ? 1 : (want > kRmsMaxBlocks ? kRmsMaxBlocks : want);
}

extern "C" int cusrl_masked_col_stats(const float *x, const uint8_t *mask, int64_t rows, int64_t C, double *partials,
                                      float *batch_mean, float *batch_var, double *batch_count, void *stream) {
    if (rows < 0 || C <= 0) return CUSRL_E_INVALID;
    if (!partials || !batch_mean || !batch_var || !batch_count || (rows > 0 && !x)) return CUSRL_E_INVALID;
    if (C >= (int64_t(1) << 30)) return CUSRL_E_UNSUPPORTED;  // int channel offsets in the partials
    hipStream_t s = as_stream(stream);
    const int64_t P = rows == 0 ? 0 : cusrl_masked_stats_num_partials(rows, C);
    if (P > 0) {
        if (C < kBlock)
            hipLaunchKernelGGL(masked_col_stats_kernel, dim3(uint32_t(P)), dim3(kBlock), 0, s, x, mask, rows, int(C),
                               partials);
        else
            hipLaunchKernelGGL(masked_col_stats_wide_kernel, dim3(uint32_t(P)), dim3(kBlock), 0, s, x, mask, rows,
                               int(C), partials);
        if (int rc = launch_status()) return rc;
    }
    hipLaunchKernelGGL(masked_stats_finalize_kernel, dim3(1), dim3(kBlock), 0, s, partials, int(P), int(C), x,
                       batch_mean, batch_var, batch_count);
    return launch_status();
}

extern "C" int cusrl_rms_merge(float *mean, float *var, float *std, double *count, const float *batch_mean,
                               const float *batch_var, const double *batch_count, float eps, double max_count,
                               int64_t C, void *stream) {
    if (C <= 0 || !mean || !var || !std || !count || !batch_mean || !batch_var || !batch_count) return CUSRL_E_INVALID;
    if (C > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    hipLaunchKernelGGL(rms_merge_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), mean, var, std, count, batch_mean,
                       batch_var, batch_count, eps, max_count, int(C));
    return launch_status();
}

extern "C" int cusrl_rms_normalize(const float *x, const float *mean, const float *std, float clamp, float *out,
                                   int64_t rows, int64_t C, void *stream) {
    if (rows < 0 || C <= 0) return CUSRL_E_INVALID;
    if (rows == 0) return 0;
    if (!x || !mean || !std || !out) return CUSRL_E_INVALID;
    if (C > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    const int64_t E = rows * C;
    const int vec4 = C % 4 == 0 && aligned(x, 16) && aligned(out, 16) && aligned(mean, 16) && aligned(std, 16);
    int64_t blocks = ceil_div(vec4 ? E / 4 : E, kBlock);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rms_normalize_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), x, mean, std,
                       clamp, out, E, int(C), vec4);
    return launch_status();
}

extern "C" int64_t cusrl_amp_prepare_max_elements(void) { return int64_t(1) << 20; }

static int prep_blocks(int64_t elements) {
    const int64_t want = ceil_div(elements, int64_t(kBlock) * kPrepItems);
    return int(want < 1 ? 1 : (want > kPrepMaxBlocks ? kPrepMaxBlocks : want));
}

extern "C" int64_t cusrl_amp_prepare_workspace(int64_t N, int64_t C) {
    if (N <= 0 || C <= 0) return 0;
    return int64_t(prep_blocks(N * C)) * 2 * C * 2 + 4 * C + 1;  // doubles
}

extern "C" int cusrl_amp_prepare(const float *state, const float *next_state, int64_t state_pitch, const int32_t *columns,
                                 int64_t K, const float *agent_raw, const float *dataset, const int64_t *indices,
                                 const float *expert_raw, int64_t N, int64_t C, float *mean, float *var, float *std,
                                 double *count, float eps, double max_count, float clamp, float *agent_out,
                                 float *expert_out, double *workspace, void *stream) {
    if (N <= 0 || C <= 0) return CUSRL_E_INVALID;
    if (!mean || !var || !std || !count || !agent_out || !expert_out || !workspace) return CUSRL_E_INVALID;
    if (!agent_raw && (!state || !next_state || 2 * K != C || state_pitch < K || state_pitch > INT32_MAX)) return CUSRL_E_INVALID;
    if (!expert_raw && (!dataset || !indices)) return CUSRL_E_INVALID;
    if (C > kPrepMaxC || N * C > cusrl_amp_prepare_max_elements()) return CUSRL_E_UNSUPPORTED;
    const int P = prep_blocks(N * C);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(amp_assemble_kernel, dim3(P), dim3(kBlock), 0, s, state, next_state, int(state_pitch), columns, int(K),
                       agent_raw, dataset, indices, expert_raw, int(N * C), int(C), mean, var, count, agent_out, expert_out,
                       workspace);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(amp_normalize_kernel, dim3(P), dim3(kBlock), 0, s, workspace, P, int(N * C), int(C), int(N), eps,
                       max_count, clamp, mean, var, std, count, agent_out, expert_out);
    return launch_status();
}
