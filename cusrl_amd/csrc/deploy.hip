// The two elementwise ends of a deployed policy's step (cusrl_amd/nn/deployed.py; DESIGN.md, "Deployment"; contracts:
// include/cusrl_hip.h).  A deployed policy at batch 1 .. 4096 is launch latency, so what stands in front of the first GEMM is
// ONE launch and what stands behind the last one is ONE launch:
//   prologue   x = clamp((nan_to_num(obs) - mean) / std, -c, c)       the sanitiser's bit classification (csrc/common.hpp)
//                                                                     and the normaliser's element (csrc/running_stats.hpp),
//                                                                     in their order, each an optional part
//   epilogue   a = clip((y + bias) * scale + shift, lo, hi), in place  + the memory rows of finished envs zeroed
// Every step is one rounded fp32 operation (the library is built with -ffp-contract=off), the division is the correctly
// rounded one, so a 16-byte lane and a scalar lane give the same bits and the host restatements (`*_cpu`, below) give them too.
// A lane loads its operands before it stores, so the prologue's out may be obs itself.  Plain vector stores only.
#include "common.hpp"
#include "running_stats.hpp"

namespace cusrl {
namespace {

constexpr int kDeployMaxBlocks = 2048;  // 8 blocks per CU; the grid-stride loops cover what is left

struct Replace {
    uint32_t nan, posinf, neginf;
    int on;
};

// one element of the prologue: the sanitiser's word, then normalize_clamp — its division behind the prologue's own switch
__host__ __device__ __forceinline__ float prologue_apply(float v, float m, float s, const Replace &r, int normalize, float clamp) {
    if (r.on) v = word_as_float(nan_to_num_word(float_as_word(v), r.nan, r.posinf, r.neginf));
    if (normalize) v = normalized(v, m, s);
    return symmetric_clamp(v, clamp);
}

// kWidth 4: K % 4 == 0, the 4 elements of a lane are 4 adjacent channels of one row; kWidth 1: one element per lane
template <int kWidth>
__global__ __launch_bounds__(kBlock) void deploy_prologue_kernel(const float *obs, const float *__restrict__ mean,
                                                                 const float *__restrict__ std, Replace replace, float clamp,
                                                                 float *out, int64_t lanes, int K) {
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    const int normalize = mean != nullptr;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < lanes; i += stride) {
        if constexpr (kWidth == 4) {
            const int c = int((i * 4) % K);
            const float4 v = reinterpret_cast<const float4 *>(obs)[i];
            float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f), s = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
            if (normalize) {
                m = *reinterpret_cast<const float4 *>(mean + c);
                s = *reinterpret_cast<const float4 *>(std + c);
            }
            reinterpret_cast<float4 *>(out)[i] =
                make_float4(prologue_apply(v.x, m.x, s.x, replace, normalize, clamp), prologue_apply(v.y, m.y, s.y, replace, normalize, clamp),
                            prologue_apply(v.z, m.z, s.z, replace, normalize, clamp), prologue_apply(v.w, m.w, s.w, replace, normalize, clamp));
        } else {
            const int c = int(i % K);
            out[i] = prologue_apply(obs[i], normalize ? mean[c] : 0.0f, normalize ? std[c] : 1.0f, replace, normalize, clamp);
        }
    }
}

// one element of the epilogue: one add, one multiply and one add (two roundings), two compares.  The compares leave a NaN a
// NaN, as torch.clamp does.
__host__ __device__ __forceinline__ float epilogue_apply(float v, float b, float scale, float shift, float lo, float hi, int biased,
                                                         int affine, int clip) {
    if (biased) v = v + b;
    if (affine) {
        v = v * scale;
        v = v + shift;
    }
    if (clip) {
        v = v < lo ? lo : v;
        v = v > hi ? hi : v;
    }
    return v;
}

// The action part walks the E = B * A elements of y (one per lane: A is narrow and rarely a multiple of 4), the memory part the
// B * M / kMemWidth lanes of the memory, both by grid-stride over the same grid.  A finished env's row is written as zeros, any
// other row is not touched.
template <int kMemWidth>
__global__ __launch_bounds__(kBlock) void deploy_epilogue_kernel(float *y, const float *__restrict__ bias, const float *__restrict__ scale,
                                                                 const float *__restrict__ shift, const float *__restrict__ lo,
                                                                 const float *__restrict__ hi, int64_t E, int A,
                                                                 const uint8_t *__restrict__ done, float *__restrict__ memory,
                                                                 int64_t memory_lanes, int64_t lanes_per_row) {
    const int64_t tid = int64_t(blockIdx.x) * kBlock + threadIdx.x, stride = int64_t(gridDim.x) * kBlock;
    const int biased = bias != nullptr, affine = scale != nullptr, clip = lo != nullptr;
    if (biased || affine || clip) {
        for (int64_t i = tid; i < E; i += stride) {
            const int a = int(i % A);
            y[i] = epilogue_apply(y[i], biased ? bias[a] : 0.0f, affine ? scale[a] : 1.0f, affine ? shift[a] : 0.0f, clip ? lo[a] : 0.0f,
                                  clip ? hi[a] : 0.0f, biased, affine, clip);
        }
    }
    for (int64_t i = tid; i < memory_lanes; i += stride) {
        if (done[i / lanes_per_row]) {
            if constexpr (kMemWidth == 4)
                reinterpret_cast<float4 *>(memory)[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            else
                memory[i] = 0.0f;
        }
    }
}

int grid_blocks(int64_t lanes) {
    const int64_t blocks = ceil_div(lanes, kBlock);
    return int(blocks < 1 ? 1 : (blocks > kDeployMaxBlocks ? kDeployMaxBlocks : blocks));
}

Replace make_replace(const float *triple) {
    Replace r{0u, 0u, 0u, 0};
    if (triple) r = Replace{float_as_word(triple[0]), float_as_word(triple[1]), float_as_word(triple[2]), 1};
    return r;
}

int check_prologue(const void *obs, const void *mean, const void *std, const void *out, int64_t B, int64_t K) {
    if (B < 0 || K <= 0) return CUSRL_E_INVALID;
    if ((mean == nullptr) != (std == nullptr)) return CUSRL_E_INVALID;
    if (B > 0 && (!obs || !out)) return CUSRL_E_INVALID;
    if (K > INT32_MAX || B > INT64_MAX / K) return CUSRL_E_UNSUPPORTED;
    return 0;
}

int check_epilogue(const void *y, const void *scale, const void *shift, const void *lo, const void *hi, int64_t B, int64_t A,
                   const void *done, const void *memory, int64_t M) {
    if (B < 0 || A <= 0 || M < 0) return CUSRL_E_INVALID;
    if ((scale == nullptr) != (shift == nullptr) || (lo == nullptr) != (hi == nullptr)) return CUSRL_E_INVALID;
    if (done && (!memory || M <= 0)) return CUSRL_E_INVALID;
    if (B > 0 && !y) return CUSRL_E_INVALID;
    if (A > INT32_MAX || B > INT64_MAX / A || (M > 0 && B > INT64_MAX / M)) return CUSRL_E_UNSUPPORTED;
    return 0;
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_deploy_prologue(const float *obs, const float *replace, const float *mean, const float *std, float clamp,
                                     float *out, int64_t B, int64_t K, void *stream) {
    if (int rc = check_prologue(obs, mean, std, out, B, K)) return rc;
    if (B == 0) return 0;
    if (!aligned(obs, 4) || !aligned(out, 4)) return CUSRL_E_INVALID;
    const int64_t E = B * K;
    const bool vec = K % 4 == 0 && aligned(obs, 16) && aligned(out, 16) && (!mean || (aligned(mean, 16) && aligned(std, 16)));
    const int64_t lanes = vec ? E / 4 : E;
    const Replace r = make_replace(replace);
    if (!(clamp > 0.0f)) clamp = 0.0f;  // (a NaN included: no clamp)
    if (vec)
        hipLaunchKernelGGL(deploy_prologue_kernel<4>, dim3(grid_blocks(lanes)), dim3(kBlock), 0, as_stream(stream), obs, mean, std, r,
                           clamp, out, lanes, int(K));
    else
        hipLaunchKernelGGL(deploy_prologue_kernel<1>, dim3(grid_blocks(lanes)), dim3(kBlock), 0, as_stream(stream), obs, mean, std, r,
                           clamp, out, lanes, int(K));
    return launch_status();
}

extern "C" int cusrl_deploy_prologue_cpu(const float *obs, const float *replace, const float *mean, const float *std, float clamp,
                                         float *out, int64_t B, int64_t K) {
    if (int rc = check_prologue(obs, mean, std, out, B, K)) return rc;
    const Replace r = make_replace(replace);
    if (!(clamp > 0.0f)) clamp = 0.0f;
    const int normalize = mean != nullptr;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t k = 0; k < K; ++k)
            out[b * K + k] = prologue_apply(obs[b * K + k], normalize ? mean[k] : 0.0f, normalize ? std[k] : 1.0f, r, normalize, clamp);
    return 0;
}

extern "C" int cusrl_deploy_epilogue(float *y, const float *bias, const float *scale, const float *shift, const float *lo,
                                     const float *hi, int64_t B, int64_t A, const uint8_t *done, float *memory, int64_t M,
                                     void *stream) {
    if (int rc = check_epilogue(y, scale, shift, lo, hi, B, A, done, memory, M)) return rc;
    if (B == 0) return 0;
    const bool arithmetic = bias || scale || lo;
    if (!arithmetic && !done) return 0;  // nothing to do: nothing launched
    const int64_t E = arithmetic ? B * A : 0;
    const bool vec = done && M % 4 == 0 && aligned(memory, 16);
    const int64_t lanes_per_row = done ? (vec ? M / 4 : M) : 1;
    const int64_t memory_lanes = done ? B * lanes_per_row : 0;
    const int blocks = grid_blocks(E > memory_lanes ? E : memory_lanes);
    if (vec)
        hipLaunchKernelGGL(deploy_epilogue_kernel<4>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), y, bias, scale, shift, lo, hi, E,
                           int(A), done, memory, memory_lanes, lanes_per_row);
    else
        hipLaunchKernelGGL(deploy_epilogue_kernel<1>, dim3(blocks), dim3(kBlock), 0, as_stream(stream), y, bias, scale, shift, lo, hi, E,
                           int(A), done, memory, memory_lanes, lanes_per_row);
    return launch_status();
}

extern "C" int cusrl_deploy_epilogue_cpu(float *y, const float *bias, const float *scale, const float *shift, const float *lo,
                                         const float *hi, int64_t B, int64_t A, const uint8_t *done, float *memory, int64_t M) {
    if (int rc = check_epilogue(y, scale, shift, lo, hi, B, A, done, memory, M)) return rc;
    const int biased = bias != nullptr, affine = scale != nullptr, clip = lo != nullptr;
    for (int64_t b = 0; b < B; ++b) {
        if (biased || affine || clip)
            for (int64_t a = 0; a < A; ++a)
                y[b * A + a] = epilogue_apply(y[b * A + a], biased ? bias[a] : 0.0f, affine ? scale[a] : 1.0f, affine ? shift[a] : 0.0f,
                                              clip ? lo[a] : 0.0f, clip ? hi[a] : 0.0f, biased, affine, clip);
        if (done && done[b])
            for (int64_t m = 0; m < M; ++m) memory[b * M + m] = 0.0f;
    }
    return 0;
}
