// The arithmetic the running-statistics kernels share, one body per computation (the callers: the table in normalization.hip).
// Every step is one rounded IEEE operation in the order written (the library is built with -ffp-contract=off), so the host
// twins of reward_norm.hip and deploy.hip give the device's bits wherever float64 division and square root agree.
#pragma once

#include "common.hpp"

namespace cusrl {

struct MeanVar { double mean, var; };

// Mean and POPULATION variance (clamped at 0) of n values from the float64 sums s, q of x - pivot and (x - pivot)^2: shifted sums
// keep q / n - (s / n)^2 free of the cancellation of E[x^2] - E[x]^2 when |mean| >> std, and a constant channel exact.
__host__ __device__ __forceinline__ MeanVar shifted_mean_var(double s, double q, double n, double pivot) {
    const double d = s / n;  // mean - pivot
    const double v = q / n - d * d;
    return {pivot + d, v < 0.0 ? 0.0 : v};
}

// Chan merge of a batch of n values into the running (mean, var) of `count` values, in T; returns the uncapped new count.
template <typename T>
__host__ __device__ __forceinline__ double chan_merge(T &mean, T &var, double count, T batch_mean, T batch_var, double n) {
    const double w_sum = count + n;
    const T w_new = T(n / w_sum), w_cross = T((count / w_sum) * (n / w_sum));
    const T delta = batch_mean - mean;
    mean = mean + delta * w_new;
    var = var + ((batch_var - var) * w_new + (delta * delta) * w_cross);
    return w_sum;
}

__host__ __device__ __forceinline__ double capped_count(double total, double max_count) {
    return max_count > 0.0 && total > max_count ? max_count : total;
}

// (x - mean) / std: a subtraction, then a DIVISION (no reciprocal), torch's bits; clamp <= 0: no clamp
__host__ __device__ __forceinline__ float normalized(float x, float m, float s) { return (x - m) / s; }
__host__ __device__ __forceinline__ float symmetric_clamp(float v, float clamp) {
    return clamp > 0.0f ? fminf(fmaxf(v, -clamp), clamp) : v;
}
__host__ __device__ __forceinline__ float normalize_clamp(float x, float m, float s, float clamp) {
    return symmetric_clamp(normalized(x, m, s), clamp);
}

}  // namespace cusrl
