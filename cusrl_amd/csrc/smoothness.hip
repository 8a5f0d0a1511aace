// ActionSmoothnessLoss (cusrl/hook/auxiliary/smoothness.py:59-102): the first- and second-order differences of the action mean
// along time, cut at episode ends, as weighted mean absolute values — both losses and their gradients from ONE C-ABI call.
//
//   cusrl_action_smoothness_fwd_bwd   count launch -> walk launch (-> one-block finalize beyond one block)
//
// The reference pads the minibatch into per-episode sequences (split_and_pad_sequences), convolves them with [-1, 1] and
// [-1, 2, -1], gathers the valid positions through a boolean mask, and lets autograd run the chain backwards.  In closed form,
// for mean [T, B, A] and done [T, B]:
//   pair (t-1, t) of env b is valid iff !done[t-1, b];                 d1 = mean[t] - mean[t-1]
//   triple (t-2, t-1, t) is valid iff !done[t-2, b] && !done[t-1, b];  d2 = -mean[t-2] + 2 mean[t-1] - mean[t]
//   loss_k = sum_valid sum_a w_k[a] |d_k| / (n_k A),  n_k = number of valid pairs / triples (done[T-1] never matters)
//   d loss_k / d mean: +-w_1[a] sign(d1) / (n_1 A) on rows t, t-1;  (-1, +2, -1) w_2[a] sign(d2) / (n_2 A) on rows t-2, t-1, t
// with sign(0) = 0 (torch's abs backward).  n_k = 0: the loss is 0 / 0 = NaN (the mean of an empty selection) and no pair or
// triple exists that could add to the gradient, which is then all zeros — what the reference's autograd gives.
#include "common.hpp"
#include "loss_reduce.hpp"

namespace cusrl {

constexpr int kSmoothCountBlocks = 64;   // blocks of the count launch at most (their partials are re-summed by every walk block)
constexpr int kSmoothMaxBlocks = 1024;   // blocks of the walk at most (grid-stride over the columns beyond that)

// n_1 and n_2 per block of envs: exact integer counts of `done` flags.  Thread = env b, walking t; the lanes of a wave read
// consecutive bytes of each done row.  count_partials[block] = {n_1, n_2} of the envs that block owns.
__global__ __launch_bounds__(kBlock) void smoothness_count_kernel(const uint8_t *__restrict__ done, int T, int B,
                                                                  long long *__restrict__ count_partials) {
    __shared__ long long scratch[kWavesPerBlock];
    long long n1 = 0, n2 = 0;
    for (int b = blockIdx.x * kBlock + threadIdx.x; b < B; b += gridDim.x * kBlock) {
        bool open_before = false;  // !done[t-1, b]
        for (int t = 0; t + 1 < T; ++t) {
            const bool open = done[int64_t(t) * B + b] == 0;
            n1 += open;
            n2 += open && open_before;
            open_before = open;
        }
    }
    const long long total1 = block_sum(n1, scratch), total2 = block_sum(n2, scratch);
    if (threadIdx.x == 0) {
        count_partials[2 * blockIdx.x] = total1;
        count_partials[2 * blockIdx.x + 1] = total2;
    }
}

__device__ __forceinline__ float sign_of(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }

__device__ __forceinline__ float mean_loss(double total, long long n, int A) { return float(total / (double(n) * double(A))); }

// Thread = one flattened (b, a) column of the [B * A] rows, walking t = 0 .. T-1: consecutive lanes read and write
// consecutive addresses of every row.  The last two means, the last two done flags and the gradient still pending for the
// last row (first order) / the last two rows (second order) live in registers; a gradient element is stored once, by its
// owner, when no later pair or triple can reach it.  g1 / g2: the [T, B * A] gradient planes of the two terms (NULL with its
// weight: that term is not evaluated).  Every block first re-sums the count launch's partials in one fixed order.
__global__ __launch_bounds__(kBlock) void smoothness_walk_kernel(
    const float *__restrict__ mean, const uint8_t *__restrict__ done, const float *__restrict__ w1, const float *__restrict__ w2,
    int T, int B, int A, const long long *__restrict__ count_partials, int count_blocks, float *__restrict__ g1,
    float *__restrict__ g2, double *__restrict__ loss_partials, float *__restrict__ losses_out,
    long long *__restrict__ counts_out) {
    __shared__ long long count_scratch[kWavesPerBlock];
    __shared__ double scratch[kWavesPerBlock];
    __shared__ long long counts[2];
    const long long part1 = int(threadIdx.x) < count_blocks ? count_partials[2 * threadIdx.x] : 0;
    const long long part2 = int(threadIdx.x) < count_blocks ? count_partials[2 * threadIdx.x + 1] : 0;
    const long long total1 = block_sum(part1, count_scratch), total2 = block_sum(part2, count_scratch);
    if (threadIdx.x == 0) {
        counts[0] = total1;
        counts[1] = total2;
        if (blockIdx.x == 0) counts_out[0] = total1, counts_out[1] = total2;
    }
    __syncthreads();
    const long long n1 = counts[0], n2 = counts[1];
    // (what the mean's backward hands every selected element: 1 / (n_k A), rounded to fp32 as torch's division is)
    const float share1 = float(1.0 / (double(n1) * double(A))), share2 = float(1.0 / (double(n2) * double(A)));

    const int64_t BA = int64_t(B) * A;
    double acc1 = 0.0, acc2 = 0.0;
    for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < BA; j += int64_t(gridDim.x) * kBlock) {
        const int b = int(j / A), a = int(j - int64_t(b) * A);
        const float weight1 = w1 ? w1[a] : 0.0f, weight2 = w2 ? w2[a] : 0.0f;
        const float c1 = weight1 * share1, c2 = weight2 * share2;
        float m2 = 0.0f, m1 = mean[j];          // mean[t-2], mean[t-1]
        bool open2 = false, open1 = done[b] == 0;  // !done[t-2], !done[t-1]
        float p1 = 0.0f;                        // first order: pending gradient of row t-1
        float q2 = 0.0f, q1 = 0.0f;             // second order: pending gradients of rows t-2 and t-1
        for (int t = 1; t < T; ++t) {
            const int64_t at = int64_t(t) * BA + j;
            const float m = mean[at];
            if (g1) {
                float here = 0.0f;
                if (open1) {
                    const float d = m - m1;
                    acc1 += double(weight1 * fabsf(d));
                    here = c1 * sign_of(d);
                    p1 -= here;
                }
                g1[at - BA] = p1;
                p1 = here;
            }
            if (g2) {
                float here = 0.0f;
                if (t >= 2) {
                    if (open2 && open1) {
                        const float d = (2.0f * m1 - m2) - m;
                        acc2 += double(weight2 * fabsf(d));
                        const float s = c2 * sign_of(d);
                        q2 -= s;
                        q1 += 2.0f * s;
                        here = -s;
                    }
                    g2[at - 2 * BA] = q2;
                }
                q2 = q1;
                q1 = here;
            }
            m2 = m1;
            m1 = m;
            open2 = open1;
            open1 = done[int64_t(t) * B + b] == 0;
        }
        const int64_t last = int64_t(T - 1) * BA + j;
        if (g1) g1[last] = p1;
        if (g2) g2[last - BA] = q2, g2[last] = q1;
    }
    publish_loss_sums<2>({acc1, acc2}, scratch, loss_partials, losses_out,
                         [&](int k, double sum) { return (k ? g2 : g1) ? mean_loss(sum, k ? n2 : n1, A) : 0.0f; });
}

__global__ __launch_bounds__(kBlock) void smoothness_finalize_kernel(const double *__restrict__ loss_partials, int blocks,
                                                                     const long long *__restrict__ counts, int A, int has1,
                                                                     int has2, float *__restrict__ losses_out) {
    __shared__ double scratch[kWavesPerBlock];
    finalize_loss_sums<2>(loss_partials, blocks, scratch, losses_out,
                          [&](int k, double sum) { return (k ? has2 : has1) ? mean_loss(sum, counts[k], A) : 0.0f; });
}

static int64_t count_blocks_of(int64_t B) {
    const int64_t want = ceil_div(B, kBlock);
    return want > kSmoothCountBlocks ? kSmoothCountBlocks : want;
}

static int64_t walk_blocks_of(int64_t B, int64_t A) {
    const int64_t want = ceil_div(B * A, kBlock);
    return want > kSmoothMaxBlocks ? kSmoothMaxBlocks : want;
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int64_t cusrl_action_smoothness_workspace(int64_t T, int64_t B, int64_t A) {
    if (T < 3 || B <= 0 || A <= 0 || B > INT32_MAX / A || T > INT32_MAX / (B * A)) return 0;
    return 2 * (count_blocks_of(B) + walk_blocks_of(B, A));  // 8-byte words: {n_1, n_2} per count block, two sums per walk block
}

extern "C" int cusrl_action_smoothness_fwd_bwd(const float *mean, const uint8_t *done, const float *w1, const float *w2,
                                               int64_t T, int64_t B, int64_t A, float *losses_out, int64_t *counts_out,
                                               float *d_mean, void *workspace, void *stream) {
    if (T < 3 || B <= 0 || A <= 0) return CUSRL_E_INVALID;
    if (!mean || !done || (!w1 && !w2) || !losses_out || !counts_out || !d_mean || !workspace) return CUSRL_E_INVALID;
    if (B > INT32_MAX / A || T > INT32_MAX / (B * A)) return CUSRL_E_UNSUPPORTED;  // 32-bit row and column indices
    const int64_t plane = T * B * A, count_blocks = count_blocks_of(B), walk_blocks = walk_blocks_of(B, A);
    long long *count_partials = static_cast<long long *>(workspace);
    double *loss_partials = reinterpret_cast<double *>(count_partials + 2 * count_blocks);
    float *g1 = w1 ? d_mean : nullptr, *g2 = w2 ? d_mean + (w1 ? plane : 0) : nullptr;
    long long *counts = reinterpret_cast<long long *>(counts_out);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(smoothness_count_kernel, dim3(uint32_t(count_blocks)), dim3(kBlock), 0, s, done, int(T), int(B),
                       count_partials);
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(smoothness_walk_kernel, dim3(uint32_t(walk_blocks)), dim3(kBlock), 0, s, mean, done, w1, w2, int(T), int(B),
                       int(A), count_partials, int(count_blocks), g1, g2, loss_partials, losses_out, counts);
    if (int rc = launch_status()) return rc;
    if (walk_blocks == 1) return 0;  // the one block finalised itself
    hipLaunchKernelGGL(smoothness_finalize_kernel, dim3(1), dim3(kBlock), 0, s, loss_partials, int(walk_blocks), counts, int(A),
                       int(w1 != nullptr), int(w2 != nullptr), losses_out);
    return launch_status();
}
