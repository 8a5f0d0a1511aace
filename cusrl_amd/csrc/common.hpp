// Shared device/host helpers for libcusrl_hip.so (gfx950 / CDNA4 only — wave64, no CUDA paths).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cusrl_hip.h"

namespace cusrl {

constexpr int kWave = 64;      // CDNA wavefront
constexpr int kBlock = 256;    // 4 waves = one wave per SIMD of a CU
constexpr int kWavesPerBlock = kBlock / kWave;

// Launch-shape / cache-policy overrides (cusrl_set_option, include/cusrl_hip.h): 0 everywhere = every kernel chooses by its
// own measured rule.  Set by the host through the C ABI — never read from the process environment inside a launch entry point.
enum Option {
    kOptGaePolicy,    // gae_policy    1 + {0, 5, 7}: force that cache policy of the scan (0: by footprint)
    kOptGaeBlock,     // gae_block     128 | 256 threads per block (0: by column count)
    kOptLossPolicy,   // loss_policy   1: default cache policy, 2: non-temporal [B, A] streams (0: by footprint)
    kOptPushPolicy,   // push_policy   1: default cache policy, 2: streaming (0: by footprint)
    kOptColsumRows,   // colsum_rows   rows per block of the mask + column-sum pass (0: 64)
    kOptHeadRows,     // head_rows     rows per block of the narrow-head backward (0: 96)
    kOptGruBiasRows,  // gru_bias_rows rows per partial row of the GRU bias gradients, 4 | 8 | 16 | 32 (0: 16)
    kNumOptions
};
int64_t option(Option which);  // api.hip

inline int launch_status() {
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : static_cast<int>(err);
}

inline hipStream_t as_stream(void *stream) { return static_cast<hipStream_t>(stream); }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ bool aligned_ptr16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// tensor.nan_to_num of one fp32 word, classified on the bit pattern: exponent all ones and a mantissa -> `nan` (any sign, any
// payload), +Inf -> `posinf`, -Inf -> `neginf`; every other pattern (-0.0, denormals, +-FLT_MAX) comes back as it is, so no
// floating-point mode can touch it.  The sanitiser's (aux_hooks.hip) and the deploy prologue's (deploy.hip) one classification.
__host__ __device__ __forceinline__ uint32_t float_as_word(float value) { return __builtin_bit_cast(uint32_t, value); }
__host__ __device__ __forceinline__ float word_as_float(uint32_t bits) { return __builtin_bit_cast(float, bits); }
__host__ __device__ __forceinline__ uint32_t nan_to_num_word(uint32_t bits, uint32_t nan, uint32_t posinf, uint32_t neginf) {
    if ((bits & 0x7f800000u) != 0x7f800000u) return bits;  // finite
    return (bits & 0x007fffffu) ? nan : ((bits >> 31) ? neginf : posinf);
}

// ---- 16-byte accesses with the non-temporal hint (streams nobody reads again soon); clang's builtins take native vectors ----
typedef float native_float4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float4 nt_load16(const float4 *p) {
    const native_float4 v = __builtin_nontemporal_load(reinterpret_cast<const native_float4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

__device__ __forceinline__ void nt_store16(float4 *p, const float4 &v) {
    const native_float4 n = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(n, reinterpret_cast<native_float4 *>(p));
}

// 16 opaque bytes, streamed (NT) or not: the non-temporal pair moves them as a float4, the bits pass through untouched
template <bool NT>
__device__ __forceinline__ uint4 stream_load16(const char *p) {
    if constexpr (NT) {
        const float4 v = nt_load16(reinterpret_cast<const float4 *>(p));
        return make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
    } else {
        return *reinterpret_cast<const uint4 *>(p);
    }
}
template <bool NT>
__device__ __forceinline__ void stream_store16(char *p, const uint4 &v) {
    if constexpr (NT) {
        nt_store16(reinterpret_cast<float4 *>(p),
                   make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)));
    } else {
        *reinterpret_cast<uint4 *>(p) = v;
    }
}

// ---- wave / block reductions (wave64 shuffles; LDS only across the 4 waves of a block) ----
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;  // valid in lane 0
}

// Sum over a block of kWaves waves; result valid in thread 0.  `scratch` holds kWaves entries, which thread 0 adds in index
// order.
template <typename T, int kWaves = kWavesPerBlock>
__device__ __forceinline__ T block_sum(T v, T *scratch) {
    v = wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    if (lane == 0) scratch[wave] = v;
    __syncthreads();
    T total = T(0);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kWaves; ++w) total += scratch[w];
    }
    __syncthreads();
    return total;
}

// Wave-wide sum of a double by DPP moves of its two halves (quad swaps, row rotations, row broadcasts): six steps of
// 2 v_mov_dpp + 1 v_add_f64 instead of six ds_bpermute round trips per half; fixed order; the total lands in lane 63.
// NOT wave_sum's order (neighbours first here, halves first there): the two give different last bits, so a sum whose
// bits are pinned stays with the one it was written with.
template <int kCtrl>
__device__ __forceinline__ double dpp_move(double v) {
    const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), kCtrl, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), kCtrl, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum_to_last_lane(double v) {
    v += dpp_move<0xb1>(v);   // quad_perm:[1,0,3,2]
    v += dpp_move<0x4e>(v);   // quad_perm:[2,3,0,1]
    v += dpp_move<0x124>(v);  // row_ror:4
    v += dpp_move<0x128>(v);  // row_ror:8   -> every lane holds its row's (16 lanes) sum
    v += dpp_move<0x142>(v);  // row_bcast:15 -> rows 1 and 3 add the row in front of them
    v += dpp_move<0x143>(v);  // row_bcast:31 -> the upper half adds lane 31: lane 63 holds the wave's sum
    return v;
}

// Exclusive prefix sum of one int per thread over the block; also returns the block total.
__device__ __forceinline__ int block_exclusive_scan(int v, int *scratch, int &total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        int up = __shfl_up(incl, off, kWave);
        if (lane >= off) incl += up;
    }
    if (lane == kWave - 1) scratch[wave] = incl;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        int s = scratch[w];
        if (w < wave) base += s;
        total += s;
    }
    __syncthreads();
    return base + incl - v;
}

}  // namespace cusrl
