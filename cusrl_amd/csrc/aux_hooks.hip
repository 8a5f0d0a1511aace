// Reward-side hooks of a captured env step and the auxiliary objectives of a minibatch step as
// single launches:
//   cusrl_reward_shaping        RewardShaping.post_step         cusrl/hook/mdp/reward.py:43-47   (mul_, add_, clamp_)
//   cusrl_amp_style_reward_mean the style reward (amp.py:130-134) + the mean the metric records, one launch
//   cusrl_mse_loss_fwd_bwd      nn.MSELoss(predictor(x), target(x)) of RandomNetworkDistillation.objective (rnd.py:78-81):
//                               loss and d loss / d prediction in one pass
//   cusrl_column_mse_fwd_bwd    weight * nn.MSELoss(prediction, leaf[..., columns]) of the privileged-information hooks
//                               (estimation.py, representation.py, distillation.py): the same, the target read in place
//   cusrl_normal_nll_fwd_bwd    nn.NormalNllLoss (cusrl/nn/layer/loss.py:62-141): the loss and both gradients in one pass
//   cusrl_nan_to_num2           ObservationNanToNum.pre_act / post_step  cusrl/hook/mdp/observation.py:42-56: nan_to_num_ of
//                               the observation AND the state in one launch, storing only what it replaced
// All of these are a few hundred KB per launch at 4096 envs: latency-bound chains of tiny kernels in the reference's form,
// so what counts is the NUMBER of dependent launches inside the captured step (>= 1.5 us each + their own latency).
// (AMP's transition preparation, cusrl_amp_prepare, is a running-statistics update: csrc/normalization.hip.)
#include "common.hpp"
#include "loss_reduce.hpp"
#include "philox.hpp"

namespace cusrl {

// --------------------------------------------------------------------------------------------- reward shaping
// reward.mul_(scale).add_(shift) [two roundings, like the two torch ops], then clamp_(min, max) in torch's order:
// min(max(x, lo), hi), NaN propagates
__global__ __launch_bounds__(kBlock) void reward_shaping_kernel(float *__restrict__ reward, float scale, float shift,
                                                                float lower, float upper, int has_lower, int has_upper,
                                                                int64_t n) {
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    float r = __fadd_rn(__fmul_rn(reward[i], scale), shift);
    if (has_lower) r = (r != r) ? r : (r < lower ? lower : r);
    if (has_upper) r = (r != r) ? r : (r > upper ? upper : r);
    reward[i] = r;
}

// --------------------------------------------------------------------------------------------- observation sanitiser
// tensor.nan_to_num_(nan, posinf, neginf) of up to TWO fp32 arrays in one launch, classified on the bit pattern by
// nan_to_num_word (common.hpp): a finite pattern is never rewritten.  STORE ON CHANGE: a lane writes its 16
// bytes (or its scalar) back only when a value in it was replaced by a different pattern — on clean input, the common case, the
// launch is a pure read stream of 4 B per element.  No element is touched by two threads: nothing to order.
// Per array: a scalar head up to the first 16-byte boundary (<= 3 elements; observation tensors can be offset views, only
// 4-byte alignment is guaranteed), a 16-byte body, a scalar tail (<= 3); the <= 6 scalars go to the first threads of the grid.
// The body is a grid-stride loop over a capped grid with TWO independent 16-byte loads per lane in flight before the first
// conditional store (the compiler cannot hoist a load of the same array over such a store by itself).
constexpr int kSanitizeMaxBlocks = 2048;                      // 8 blocks per CU
constexpr int64_t kSanitizeSpan = int64_t(kBlock) * 2 * 4;    // elements of one array one block covers per pass

__device__ __forceinline__ bool sanitize_word(uint32_t &bits, uint32_t nan, uint32_t posinf, uint32_t neginf) {
    const uint32_t to = nan_to_num_word(bits, nan, posinf, neginf);
    const bool changed = to != bits;  // (posinf = +Inf leaves an infinity alone: nothing to store)
    bits = to;
    return changed;
}

__device__ __forceinline__ bool sanitize_quad(uint4 &v, uint32_t nan, uint32_t posinf, uint32_t neginf) {
    bool changed = sanitize_word(v.x, nan, posinf, neginf);
    changed |= sanitize_word(v.y, nan, posinf, neginf);
    changed |= sanitize_word(v.z, nan, posinf, neginf);
    changed |= sanitize_word(v.w, nan, posinf, neginf);
    return changed;
}

template <bool NT>
__device__ __forceinline__ void sanitize_array(uint32_t *__restrict__ words, int64_t n, int64_t tid, int64_t stride, uint32_t nan,
                                               uint32_t posinf, uint32_t neginf) {
    int64_t head = int64_t((16 - (reinterpret_cast<uintptr_t>(words) & 15)) & 15) / 4;
    if (head > n) head = n;
    const int64_t quads = (n - head) / 4, tail = head + quads * 4;
    if (tid < head + (n - tail)) {  // the <= 6 scalars in front of and behind the body
        const int64_t i = tid < head ? tid : tail + (tid - head);
        uint32_t w = words[i];
        if (sanitize_word(w, nan, posinf, neginf)) words[i] = w;
    }
    uint4 *__restrict__ body = reinterpret_cast<uint4 *>(words + head);
    for (int64_t q0 = tid; q0 < quads; q0 += 2 * stride) {
        const int64_t q1 = q0 + stride;
        const bool second = q1 < quads;
        uint4 v0 = stream_load16<NT>(reinterpret_cast<const char *>(body + q0)), v1 = make_uint4(0u, 0u, 0u, 0u);
        if (second) v1 = stream_load16<NT>(reinterpret_cast<const char *>(body + q1));
        if (sanitize_quad(v0, nan, posinf, neginf)) body[q0] = v0;
        if (second && sanitize_quad(v1, nan, posinf, neginf)) body[q1] = v1;
    }
}

// NT: non-temporal loads (chosen by the launch's footprint, cusrl_nan_to_num2).  The rare stores are plain: whoever reads the
// tensor next (the actor's forward, the buffer append) wants them in L2.
template <bool NT>
__global__ __launch_bounds__(kBlock) void nan_to_num2_kernel(uint32_t *__restrict__ a, int64_t na, uint32_t *__restrict__ b,
                                                             int64_t nb, uint32_t nan, uint32_t posinf, uint32_t neginf) {
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x, stride = int64_t(gridDim.x) * kBlock;
    if (na > 0) sanitize_array<NT>(a, na, tid, stride, nan, posinf, neginf);
    if (nb > 0) sanitize_array<NT>(b, nb, tid, stride, nan, posinf, neginf);
}

// --------------------------------------------------------------------------------------------- AMP style reward + its mean
constexpr int kPrepThreads = 1024;  // one workgroup: rows of ONE env step, a single pass

__global__ __launch_bounds__(kPrepThreads) void amp_style_reward_mean_kernel(const float *__restrict__ logit,
                                                                             float *__restrict__ reward,
                                                                             float *__restrict__ bonus_out, float scale,
                                                                             int64_t rows, float *__restrict__ mean_out) {
    __shared__ double scratch[kPrepThreads / kWave];
    double total = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += kPrepThreads) {
        // reward_scale * -log(clamp(1 - 1 / (1 + exp(-logit)), min=1e-4)), evaluated in the reference's order
        const float p = 1.0f - 1.0f / (1.0f + expf(-logit[i]));
        const float bonus = scale * -logf(fmaxf(p, 1e-4f));
        reward[i] += bonus;
        if (bonus_out) bonus_out[i] = bonus;
        total += double(bonus);
    }
    total = block_sum<double, kPrepThreads / kWave>(total, scratch);
    if (threadIdx.x == 0) *mean_out = float(total / double(rows));
}

// --------------------------------------------------------------------------------------------- MSE loss, forward + backward
// target == nullptr: zeros (a plain scaled sum of squares).  The sum leaves through publish_loss_sums (loss_reduce.hpp).
__global__ __launch_bounds__(kBlock) void mse_fwd_bwd_kernel(const float *__restrict__ prediction,
                                                             const float *__restrict__ target, int64_t n, float grad_scale,
                                                             float *__restrict__ d_prediction,
                                                             double *__restrict__ partials, double loss_scale,
                                                             float *__restrict__ loss_out) {
    __shared__ double scratch[kWavesPerBlock];
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x, stride = int64_t(gridDim.x) * kBlock;
    double acc = 0.0;
    if ((n & 3) == 0 && aligned_ptr16(prediction) && (!target || aligned_ptr16(target)) && aligned_ptr16(d_prediction)) {
        for (int64_t i = tid; i < n / 4; i += stride) {
            const float4 p = reinterpret_cast<const float4 *>(prediction)[i];
            const float4 t = target ? reinterpret_cast<const float4 *>(target)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float d[4] = {p.x - t.x, p.y - t.y, p.z - t.z, p.w - t.w};
            acc += double(d[0] * d[0]) + double(d[1] * d[1]) + double(d[2] * d[2]) + double(d[3] * d[3]);
            reinterpret_cast<float4 *>(d_prediction)[i] =
                make_float4(grad_scale * d[0], grad_scale * d[1], grad_scale * d[2], grad_scale * d[3]);
        }
    } else {
        for (int64_t i = tid; i < n; i += stride) {
            const float d = prediction[i] - (target ? target[i] : 0.0f);
            acc += double(d * d);
            d_prediction[i] = grad_scale * d;  // d mean((p - t)^2) / d p = 2 (p - t) / n
        }
    }
    publish_loss_sums<1>({acc}, scratch, partials, loss_out, ScaledLoss<1>{{loss_scale}});
}

// --------------------------------------------------------------------------------------------- column MSE, forward + backward
// weight * mean((prediction - target[..., columns])^2) and its gradient wrt the prediction, the target read IN PLACE: row r of
// the target starts at target + r * pitch (a buffer leaf, or a row view of one), column k of the prediction is compared with
// target column columns[k] (NULL: k).  What StateEstimation / the *Prediction hooks / PolicyDistillationLoss compute per
// minibatch step (estimation.py:126-131, representation.py:40-45,108-113,167-173, distillation.py:44-47) as index + sub +
// pow + mean + mul forward and fill + mse_backward + mul backward.
// Threads walk the dense [rows * K] index space of the prediction: its loads and the gradient's stores are coalesced; the
// target's reads are K-wide runs pitch apart (K is small and the rows of one wave share cache lines).  n < 2^31: 32-bit
// index arithmetic (one unsigned division per element).
__global__ __launch_bounds__(kBlock) void column_mse_fwd_bwd_kernel(const float *__restrict__ prediction,
                                                                    const float *__restrict__ target, int64_t pitch,
                                                                    const int32_t *__restrict__ columns, uint32_t n, uint32_t K,
                                                                    int vector, float grad_scale,
                                                                    float *__restrict__ d_prediction,
                                                                    double *__restrict__ partials, double loss_scale,
                                                                    float *__restrict__ loss_out) {
    __shared__ double scratch[kWavesPerBlock];
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    double acc = 0.0;
    if (vector) {  // columns == NULL, K % 4 == 0, pitch % 4 == 0, every pointer 16-byte aligned (checked by the host)
        const uint32_t quads = n / 4, row_quads = K / 4;
        for (uint32_t q = tid; q < quads; q += stride) {
            const uint32_t r = q / row_quads, kq = q - r * row_quads;
            const float4 p = reinterpret_cast<const float4 *>(prediction)[q];
            const float4 t = *reinterpret_cast<const float4 *>(target + int64_t(r) * pitch + 4 * kq);
            const float d[4] = {p.x - t.x, p.y - t.y, p.z - t.z, p.w - t.w};
            acc += double(d[0] * d[0]) + double(d[1] * d[1]) + double(d[2] * d[2]) + double(d[3] * d[3]);
            reinterpret_cast<float4 *>(d_prediction)[q] =
                make_float4(grad_scale * d[0], grad_scale * d[1], grad_scale * d[2], grad_scale * d[3]);
        }
    } else {
        for (uint32_t i = tid; i < n; i += stride) {
            const uint32_t r = i / K, k = i - r * K;
            const int64_t column = columns ? int64_t(columns[k]) : int64_t(k);
            const float d = prediction[i] - target[int64_t(r) * pitch + column];
            acc += double(d * d);
            d_prediction[i] = grad_scale * d;  // d (w mean((p - t)^2)) / d p = 2 w (p - t) / n
        }
    }
    publish_loss_sums<1>({acc}, scratch, partials, loss_out, ScaledLoss<1>{{loss_scale}});
}

// --------------------------------------------------------------------------------------------- Normal NLL, forward + backward
// NormalNllLoss (cusrl/nn/layer/loss.py:110-141): nll = 0.5 (log_var + (target - mean)^2 / var) [+ log sqrt(2 pi)], reduced by
// mean or sum, and its gradients wrt the mean and the variance parameter `dist` from the same pass.  `mode` says what `dist`
// holds (0 log_var, 1 log_std, 2 var, 3 std); it is clamped from below at `bound`, given in its own domain.  Per element in
// fp32 in the reference's order; with w = (incoming gradient of the reduction) / 2 and e = 1 - (target - mean)^2 / var:
//   d nll / d mean = -2 w (target - mean) / var        d nll / d dist = w e * d log_var / d dist  (1, 2, 1 / var, 2 / std)
// and zero where dist < bound (torch's clamp_min backward).  The clamp is a comparison, not fmaxf: a NaN stays a NaN.
// mean, dist and target are rows of K elements one pitch apart (the halves of a chunked [rows, 2K] input: pitch 2K); both
// gradients share one pitch, so the chunked form's gradient is written as ONE [rows, 2K] tensor.  Threads walk the dense
// [rows * K] index space like column_mse_fwd_bwd_kernel (n < 2^31, one unsigned division per element).
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;

__device__ __forceinline__ float normal_nll_element(float m, float d, float t, int mode, int full, float bound, float half_g,
                                                    float &d_mean, float &d_dist) {
    const bool below = d < bound;
    const float c = below ? bound : d;
    float log_var, var, slope;  // slope = d log_var / d dist
    switch (mode) {
        case 0: log_var = c, var = expf(log_var), slope = 1.0f; break;
        case 1: log_var = c * 2.0f, var = expf(log_var), slope = 2.0f; break;
        case 2: var = c, log_var = logf(var), slope = 1.0f / var; break;
        default: var = c * c, log_var = logf(c) * 2.0f, slope = 2.0f / c; break;
    }
    const float diff = t - m, ratio = diff * diff / var;
    float nll = 0.5f * (log_var + ratio);
    if (full) nll = nll + kLogSqrt2Pi;
    d_mean = -(2.0f * half_g * diff / var);
    d_dist = below ? 0.0f : half_g * (1.0f - ratio) * slope;
    return nll;
}

__global__ __launch_bounds__(kBlock) void normal_nll_fwd_bwd_kernel(
    const float *__restrict__ mean, int64_t mean_pitch, const float *__restrict__ dist, int64_t dist_pitch,
    const float *__restrict__ target, int64_t target_pitch, uint32_t n, uint32_t K, int vector, int mode, int full, float bound,
    float half_g, float *__restrict__ d_mean, float *__restrict__ d_dist, int64_t grad_pitch, double *__restrict__ partials,
    double loss_scale, float *__restrict__ loss_out) {
    __shared__ double scratch[kWavesPerBlock];
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, stride = gridDim.x * kBlock;
    double acc = 0.0;
    if (vector) {  // K % 4 == 0, every pitch % 4 == 0, every pointer 16-byte aligned (checked by the host)
        const uint32_t quads = n / 4, row_quads = K / 4;
        for (uint32_t q = tid; q < quads; q += stride) {
            const uint32_t r = q / row_quads;
            const int64_t k = 4 * int64_t(q - r * row_quads);
            const float4 m = *reinterpret_cast<const float4 *>(mean + int64_t(r) * mean_pitch + k);
            const float4 d = *reinterpret_cast<const float4 *>(dist + int64_t(r) * dist_pitch + k);
            const float4 t = *reinterpret_cast<const float4 *>(target + int64_t(r) * target_pitch + k);
            float4 gm, gd;
            acc += double(normal_nll_element(m.x, d.x, t.x, mode, full, bound, half_g, gm.x, gd.x));
            acc += double(normal_nll_element(m.y, d.y, t.y, mode, full, bound, half_g, gm.y, gd.y));
            acc += double(normal_nll_element(m.z, d.z, t.z, mode, full, bound, half_g, gm.z, gd.z));
            acc += double(normal_nll_element(m.w, d.w, t.w, mode, full, bound, half_g, gm.w, gd.w));
            *reinterpret_cast<float4 *>(d_mean + int64_t(r) * grad_pitch + k) = gm;
            *reinterpret_cast<float4 *>(d_dist + int64_t(r) * grad_pitch + k) = gd;
        }
    } else {
        for (uint32_t i = tid; i < n; i += stride) {
            const uint32_t r = i / K;
            const int64_t k = int64_t(i - r * K);
            float gm, gd;
            acc += double(normal_nll_element(mean[int64_t(r) * mean_pitch + k], dist[int64_t(r) * dist_pitch + k],
                                             target[int64_t(r) * target_pitch + k], mode, full, bound, half_g, gm, gd));
            d_mean[int64_t(r) * grad_pitch + k] = gm;
            d_dist[int64_t(r) * grad_pitch + k] = gd;
        }
    }
    publish_loss_sums<1>({acc}, scratch, partials, loss_out, ScaledLoss<1>{{loss_scale}});
}

// --------------------------------------------------------------------------------------------- BCE-with-logits of a joint batch
// logit [2 * rows]: the first `rows` are agent transitions (target 0), the rest expert transitions (target 1).
//   loss = mean_i ((1 - t_i) x_i - log_sigmoid(x_i))     torch.nn.functional.binary_cross_entropy_with_logits
//   d loss / d x_i = (sigmoid(x_i) - t_i) / (2 rows)
// scaled by `weight` — (BCE(D(agent), 0) + BCE(D(expert), 1)) / 2 * loss_weight of amp.py:143-147 is exactly the mean over
// the joint batch times loss_weight.  One workgroup (a discriminator batch is 2 x 512 rows).
__global__ __launch_bounds__(kPrepThreads) void bce_pair_fwd_bwd_kernel(const float *__restrict__ logit, int64_t rows,
                                                                        float weight, float *__restrict__ loss_out,
                                                                        float *__restrict__ d_logit) {
    __shared__ double scratch[kPrepThreads / kWave];
    const int64_t n = 2 * rows;
    const float grad_scale = weight / float(n);
    double total = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kPrepThreads) {
        const float x = logit[i], t = i < rows ? 0.0f : 1.0f;
        const float log_sigmoid = fminf(x, 0.0f) - log1pf(expf(-fabsf(x)));
        total += double((1.0f - t) * x - log_sigmoid);
        d_logit[i] = (1.0f / (1.0f + expf(-x)) - t) * grad_scale;
    }
    total = block_sum<double, kPrepThreads / kWave>(total, scratch);
    if (threadIdx.x == 0) *loss_out = float(total / double(n) * double(weight));
}

// --------------------------------------------------------------------------------------------- synthetic benchmark env
// One step of the i.i.d. benchmark task of BASELINE.json config 2 (cusrl_amd/testing/environment.py): next observation
// ~ N(0, 1) [N, obs], reward ~ N(0, 1) [N, R], terminated ~ Bernoulli(p_term), truncated ~ Bernoulli(p_trunc), and one fresh
// N(0, 1) row per env for the resets — ONE launch instead of five generator launches (rand, compare, 3 x randn).
// Counter-based Philox4x32-10 keyed on (seed, step counter, stream, element): the step counter lives in device memory and is
// advanced by the kernel itself, so a hipGraph replay draws fresh numbers like an eager call does.  (The generator: philox.hpp.)
__device__ __forceinline__ float4 philox_normal4(const Philox &r) {  // two Box-Muller pairs
    const float r0 = sqrtf(-2.0f * logf(philox_uniform(r.c[0]))), r1 = sqrtf(-2.0f * logf(philox_uniform(r.c[2])));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * philox_uniform(r.c[1]), &s0, &c0);
    sincosf(6.283185307179586f * philox_uniform(r.c[3]), &s1, &c1);
    return make_float4(r0 * c0, r0 * s0, r1 * c1, r1 * s1);
}

__global__ __launch_bounds__(kBlock) void synthetic_env_step_kernel(uint64_t seed, unsigned long long *__restrict__ counter,
                                                                    int64_t N, int obs, int R, float p_term, float p_trunc,
                                                                    float *__restrict__ next_obs, float *__restrict__ reward,
                                                                    uint8_t *__restrict__ terminated,
                                                                    uint8_t *__restrict__ truncated,
                                                                    float *__restrict__ reset_rows, int64_t obs_quads,
                                                                    int64_t reward_quads) {
    // counter[0] = step number, counter[1] = arrival ticket.  Every block reads the step number first; the LAST block to
    // arrive at the ticket (all others have read by then) advances it — so a hipGraph replay draws fresh numbers like an
    // eager call, with no second launch and no host-side parity.  (Control flow only: no value depends on arrival order.)
    const unsigned long long step = __hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t k0 = uint32_t(seed), k1 = uint32_t(seed >> 32);
    const uint32_t s0 = uint32_t(step), s1 = uint32_t(step >> 32);
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t obs_total = N * obs, reward_total = N * R;
    auto store4 = [](float *dst, int64_t base, int64_t total, const float4 &v) {
        if (base + 3 < total && (reinterpret_cast<uintptr_t>(dst + base) & 15) == 0) {
            *reinterpret_cast<float4 *>(dst + base) = v;
        } else {
            const float e[4] = {v.x, v.y, v.z, v.w};
            for (int j = 0; j < 4 && base + j < total; ++j) dst[base + j] = e[j];
        }
    };
    if (i < obs_quads) {  // stream 0: next observation, stream 1: reset rows
        store4(next_obs, i * 4, obs_total, philox_normal4(philox4x32_10(uint32_t(i), uint32_t(i >> 32) | 0x00000000u, s0, s1, k0, k1)));
        store4(reset_rows, i * 4, obs_total, philox_normal4(philox4x32_10(uint32_t(i), uint32_t(i >> 32) | 0x40000000u, s0, s1, k0, k1)));
    }
    if (i < reward_quads)  // stream 2
        store4(reward, i * 4, reward_total, philox_normal4(philox4x32_10(uint32_t(i), uint32_t(i >> 32) | 0x80000000u, s0, s1, k0, k1)));
    if (i < N) {  // stream 3: the two flags of env i
        const Philox r = philox4x32_10(uint32_t(i), uint32_t(i >> 32) | 0xC0000000u, s0, s1, k0, k1);
        terminated[i] = philox_uniform(r.c[0]) < p_term ? 1 : 0;
        truncated[i] = philox_uniform(r.c[1]) < p_trunc ? 1 : 0;
    }
    __syncthreads();  // the whole block has read `step`
    if (threadIdx.x == 0) {
        const unsigned long long arrived = atomicAdd(counter + 1, 1ull);
        if (arrived == gridDim.x - 1) {
            __hip_atomic_store(counter + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(counter, step + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// --------------------------------------------------------------------------------------------- metric taps of a captured step
// accumulator[i] += *value[i] for up to 32 scalars whose addresses travel by value in the kernarg segment: what a captured
// step does with the 0-d metrics its hooks record (torch: stack + add_, two launches per step).
constexpr int kMaxTapScalars = 32;
struct ScalarTable {
    const float *value[kMaxTapScalars];
};

__global__ void accumulate_scalars_kernel(const ScalarTable table, int n, float *__restrict__ accumulator) {
    const int i = threadIdx.x;
    if (i < n) accumulator[i] += *table.value[i];
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_accumulate_scalars(const float *const *values, int n, float *accumulator, void *stream) {
    if (n < 0 || n > kMaxTapScalars) return n < 0 ? CUSRL_E_INVALID : CUSRL_E_TOO_MANY;
    if (n == 0) return 0;
    if (!values || !accumulator) return CUSRL_E_INVALID;
    ScalarTable table;
    for (int i = 0; i < kMaxTapScalars; ++i) table.value[i] = i < n ? values[i] : nullptr;
    for (int i = 0; i < n; ++i)
        if (!table.value[i]) return CUSRL_E_INVALID;
    hipLaunchKernelGGL(accumulate_scalars_kernel, dim3(1), dim3(kWave), 0, as_stream(stream), table, n, accumulator);
    return launch_status();
}

extern "C" int cusrl_reward_shaping(float *reward, float scale, float shift, float lower, float upper, int has_lower,
                                    int has_upper, int64_t n, void *stream) {
    if (n < 0) return CUSRL_E_INVALID;
    if (n == 0) return 0;
    if (!reward) return CUSRL_E_INVALID;
    hipLaunchKernelGGL(reward_shaping_kernel, dim3(uint32_t(ceil_div(n, kBlock))), dim3(kBlock), 0, as_stream(stream),
                       reward, scale, shift, lower, upper, has_lower, has_upper, n);
    return launch_status();
}

extern "C" int cusrl_nan_to_num2(float *a, int64_t na, float *b, int64_t nb, float nan, float posinf, float neginf,
                                 void *stream) {
    if (na < 0 || nb < 0) return CUSRL_E_INVALID;
    if ((na > 0 && !a) || (nb > 0 && !b)) return CUSRL_E_INVALID;
    if (na + nb == 0) return 0;
    if ((na > 0 && !aligned(a, 4)) || (nb > 0 && !aligned(b, 4))) return CUSRL_E_INVALID;
    // the longer array decides the grid (every thread walks both); + 6: the head / tail scalars of an array too short for a body
    const int64_t longest = na > nb ? na : nb;
    int64_t blocks = ceil_div(longest + 6, kSanitizeSpan);
    if (blocks > kSanitizeMaxBlocks) blocks = kSanitizeMaxBlocks;
    // cache policy by footprint, like the push (push_body.hpp): a clean pass only READS its 4 B per element; once that does not
    // fit the 256 MB Infinity Cache nobody finds the lines again, so they stream past the caches
    const bool streaming = 4 * (na + nb) >= (int64_t(256) << 20);
    uint32_t *wa = reinterpret_cast<uint32_t *>(a), *wb = reinterpret_cast<uint32_t *>(nb > 0 ? b : nullptr);
    if (streaming)
        hipLaunchKernelGGL(nan_to_num2_kernel<true>, dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), wa, na, wb, nb,
                           float_as_word(nan), float_as_word(posinf), float_as_word(neginf));
    else
        hipLaunchKernelGGL(nan_to_num2_kernel<false>, dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), wa, na, wb, nb,
                           float_as_word(nan), float_as_word(posinf), float_as_word(neginf));
    return launch_status();
}

extern "C" int cusrl_amp_style_reward_mean(const float *logit, float *reward, float *bonus_out, float scale, int64_t rows,
                                           float *mean_out, void *stream) {
    if (rows <= 0) return CUSRL_E_INVALID;
    if (!logit || !reward || !mean_out) return CUSRL_E_INVALID;
    if (rows > (int64_t(1) << 20)) return CUSRL_E_UNSUPPORTED;  // one workgroup: beyond this use cusrl_amp_style_reward
    hipLaunchKernelGGL(amp_style_reward_mean_kernel, dim3(1), dim3(kPrepThreads), 0, as_stream(stream), logit, reward,
                       bonus_out, scale, rows, mean_out);
    return launch_status();
}

extern "C" int64_t cusrl_mse_loss_num_partials(int64_t n) { return loss_blocks(n); }

static int launch_sumsq(const float *x, const float *target, int64_t n, double loss_scale, float grad_scale, float *loss_out,
                        float *grad_out, double *partials, hipStream_t s) {
    const int64_t blocks = loss_blocks(n);
    hipLaunchKernelGGL(mse_fwd_bwd_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, s, x, target, n, grad_scale, grad_out,
                       partials, loss_scale, loss_out);
    return finish_scaled_loss<1>(blocks, partials, {{loss_scale}}, loss_out, s);
}

extern "C" int cusrl_mse_loss_fwd_bwd(const float *prediction, const float *target, int64_t n, float *loss_out,
                                      float *d_prediction, double *partials, void *stream) {
    if (n <= 0) return CUSRL_E_INVALID;
    if (!prediction || !target || !loss_out || !d_prediction || !partials) return CUSRL_E_INVALID;
    return launch_sumsq(prediction, target, n, 1.0 / double(n), float(2.0 / double(n)), loss_out, d_prediction, partials,
                        as_stream(stream));
}

extern "C" int cusrl_sumsq_fwd_bwd(const float *x, int64_t n, double loss_scale, double grad_scale, float *loss_out,
                                   float *grad_out, double *partials, void *stream) {
    if (n <= 0) return CUSRL_E_INVALID;
    if (!x || !loss_out || !grad_out || !partials) return CUSRL_E_INVALID;
    return launch_sumsq(x, nullptr, n, loss_scale, float(grad_scale), loss_out, grad_out, partials, as_stream(stream));
}

extern "C" int64_t cusrl_column_mse_num_partials(int64_t rows, int64_t K) {
    if (rows <= 0 || K <= 0 || rows > INT32_MAX / K) return 0;
    return loss_blocks(rows * K);  // the launch rule of the contiguous loss
}

extern "C" int cusrl_column_mse_fwd_bwd(const float *prediction, const float *target, int64_t target_pitch,
                                        const int32_t *columns, int64_t rows, int64_t K, float weight, float *loss_out,
                                        float *d_prediction, double *partials, void *stream) {
    if (rows <= 0 || K <= 0) return CUSRL_E_INVALID;
    if (!prediction || !target || !loss_out || !d_prediction || !partials) return CUSRL_E_INVALID;
    if (target_pitch <= 0 || (!columns && target_pitch < K)) return CUSRL_E_INVALID;
    if (rows > INT32_MAX / K) return CUSRL_E_UNSUPPORTED;  // 32-bit element index
    const int64_t n = rows * K, blocks = cusrl_column_mse_num_partials(rows, K);
    const int vector = !columns && K % 4 == 0 && target_pitch % 4 == 0 && aligned(prediction, 16) && aligned(target, 16) &&
                       aligned(d_prediction, 16);
    const double loss_scale = double(weight) / double(n);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(column_mse_fwd_bwd_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, s, prediction, target, target_pitch,
                       columns, uint32_t(n), uint32_t(K), vector, float(2.0 * loss_scale), d_prediction, partials, loss_scale,
                       loss_out);
    return finish_scaled_loss<1>(blocks, partials, {{loss_scale}}, loss_out, s);
}

extern "C" int64_t cusrl_normal_nll_num_partials(int64_t rows, int64_t K) { return cusrl_column_mse_num_partials(rows, K); }

extern "C" int cusrl_normal_nll_fwd_bwd(const float *mean, int64_t mean_pitch, const float *dist, int64_t dist_pitch,
                                        const float *target, int64_t target_pitch, int64_t rows, int64_t K, int mode, int full,
                                        float bound, int reduction, float *loss_out, float *d_mean, float *d_dist,
                                        int64_t grad_pitch, double *partials, void *stream) {
    if (rows <= 0 || K <= 0) return CUSRL_E_INVALID;
    if (!mean || !dist || !target || !loss_out || !d_mean || !d_dist || !partials) return CUSRL_E_INVALID;
    if (mean_pitch < K || dist_pitch < K || target_pitch < K || grad_pitch < K) return CUSRL_E_INVALID;
    if (mode < 0 || mode > 3 || full < 0 || full > 1 || reduction < 1 || reduction > 2) return CUSRL_E_INVALID;
    if (rows > INT32_MAX / K) return CUSRL_E_UNSUPPORTED;  // 32-bit element index
    const int64_t n = rows * K, blocks = cusrl_normal_nll_num_partials(rows, K);
    const int vector = K % 4 == 0 && mean_pitch % 4 == 0 && dist_pitch % 4 == 0 && target_pitch % 4 == 0 &&
                       grad_pitch % 4 == 0 && aligned(mean, 16) && aligned(dist, 16) && aligned(target, 16) &&
                       aligned(d_mean, 16) && aligned(d_dist, 16);
    // reduction 1: mean, 2: sum.  What arrives at every element from the reduction's backward, halved (nll = 0.5 (...))
    const double loss_scale = reduction == 1 ? 1.0 / double(n) : 1.0;
    const float half_g = 0.5f * float(loss_scale);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(normal_nll_fwd_bwd_kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, s, mean, mean_pitch, dist, dist_pitch,
                       target, target_pitch, uint32_t(n), uint32_t(K), vector, mode, full, bound, half_g, d_mean, d_dist,
                       grad_pitch, partials, loss_scale, loss_out);
    return finish_scaled_loss<1>(blocks, partials, {{loss_scale}}, loss_out, s);
}

extern "C" int cusrl_bce_pair_fwd_bwd(const float *logit, int64_t rows, float weight, float *loss_out, float *d_logit,
                                      void *stream) {
    if (rows <= 0) return CUSRL_E_INVALID;
    if (!logit || !loss_out || !d_logit) return CUSRL_E_INVALID;
    if (rows > (int64_t(1) << 19)) return CUSRL_E_UNSUPPORTED;  // one workgroup
    hipLaunchKernelGGL(bce_pair_fwd_bwd_kernel, dim3(1), dim3(kPrepThreads), 0, as_stream(stream), logit, rows, weight,
                       loss_out, d_logit);
    return launch_status();
}

extern "C" int cusrl_synthetic_env_step(uint64_t seed, uint64_t *counter, int64_t N, int64_t obs_dim, int64_t reward_dim,
                                        float p_terminate, float p_truncate, float *next_observation, float *reward,
                                        uint8_t *terminated, uint8_t *truncated, float *reset_rows, void *stream) {
    if (N <= 0 || obs_dim <= 0 || reward_dim <= 0) return CUSRL_E_INVALID;
    if (!counter || !next_observation || !reward || !terminated || !truncated || !reset_rows) return CUSRL_E_INVALID;
    if (obs_dim > INT32_MAX || reward_dim > INT32_MAX || N * obs_dim > (int64_t(1) << 40)) return CUSRL_E_UNSUPPORTED;
    const int64_t obs_quads = ceil_div(N * obs_dim, 4), reward_quads = ceil_div(N * reward_dim, 4);
    int64_t threads = obs_quads > reward_quads ? obs_quads : reward_quads;
    if (N > threads) threads = N;
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(synthetic_env_step_kernel, dim3(uint32_t(ceil_div(threads, kBlock))), dim3(kBlock), 0, s, seed,
                       reinterpret_cast<unsigned long long *>(counter), N, int(obs_dim), int(reward_dim), p_terminate,
                       p_truncate, next_observation, reward, terminated, truncated, reset_rows, obs_quads, reward_quads);
    return launch_status();
}
