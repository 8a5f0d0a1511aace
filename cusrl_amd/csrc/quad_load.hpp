// The two read paths of a lane's four k values of a [*, K] row-major matrix at ANY width K (mlp2_wave_forward.hip: x and W1;
// recurrent_step.hip: x and W_ih): one clamped 16-byte load when the caller says `wide` (K % 4 == 0 and the matrix 16-byte aligned),
// four clamped 4-byte loads otherwise.  Both leave the same values in the same registers.
#pragma once

#include "common.hpp"

namespace cusrl {

// columns k .. k + 3 of row `row` of a [*, K] matrix, UNSELECTED: every address is clamped into the row (column 0 for k >= K),
// so that the load can stay in flight; quad_select zeroes what lies at k >= K when the value is used
__device__ __forceinline__ float4 quad_load(const float *base, int64_t row, int K, int k, bool wide) {
    const float *at = base + row * K;
    if (wide) return *reinterpret_cast<const float4 *>(at + (k < K ? k : 0));  // (K % 4 == 0: the quad is live or dead as a whole)
    return make_float4(at[k < K ? k : 0], at[k + 1 < K ? k + 1 : 0], at[k + 2 < K ? k + 2 : 0], at[k + 3 < K ? k + 3 : 0]);
}

__device__ __forceinline__ float4 quad_select(const float4 &v, int K, int k) {
    return make_float4(k < K ? v.x : 0.f, k + 1 < K ? v.y : 0.f, k + 2 < K ? v.z : 0.f, k + 3 < K ? v.w : 0.f);
}

}  // namespace cusrl
