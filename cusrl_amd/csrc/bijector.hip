// The std bijectors of cusrl/nn/layer/bijector.py:76-126 over a contiguous fp32 [n], forward and backward ("Std
// bijectors"): the bounded sigmoid `min + range * sigmoid(x)` and the bounded softplus `softplus(clamp(x) * scale) / scale`, each
// as ONE launch per direction instead of torch's chain of element-wise launches.  The formulas, the parameters of each kind
// and the error codes are in include/cusrl_hip.h.  The launch shape is csrc/column_affine.hip's: a lane moves 16 bytes when
// n % 4 == 0 and every pointer is 16-byte aligned, 4 bytes otherwise (the same arithmetic per element, so the same bits), the
// grid is capped and strides over the rest, element indices are 64-bit.  Every step is one rounded fp32 operation in the order
// torch's expression performs them (the library is built with -ffp-contract=off: no fma), with the accurate expf / log1pf.  The
// backward recomputes from the saved x; no output is saved.  Each lane loads its operands before it stores, so y may be x and
// dx may be dy (which is why the pointers carry no __restrict__).
#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kBijectorMaxBlocks = 2048;  // 8 blocks per CU; the grid strides over what is left
constexpr float kSoftplusThreshold = 20.0f;  // torch's: softplus(z) = z beyond it

// SIGMOID: a = min, b = range.  SOFTPLUS: a = scale, b = min_input, c = max_input.
struct BijectorParams {
    float a, b, c;
};

__device__ __forceinline__ float bijector_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }  // (gate.hip's gate_sigmoid)

// a NaN passes through (both comparisons are false), as torch's clamp does
__device__ __forceinline__ float bijector_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int kKind>
__device__ __forceinline__ float bijector_forward(float x, const BijectorParams &p) {
    if (kKind == CUSRL_BIJECTOR_SIGMOID) return p.a + p.b * bijector_sigmoid(x);  // (two roundings)
    const float z = bijector_clamp(x, p.b, p.c) * p.a;
    return (z > kSoftplusThreshold ? z : log1pf(expf(z))) / p.a;
}

template <int kKind>
__device__ __forceinline__ float bijector_backward(float x, float dy, const BijectorParams &p) {
    if (kKind == CUSRL_BIJECTOR_SIGMOID) {
        const float s = bijector_sigmoid(x);
        return dy * p.b * (1.0f - s) * s;  // torch's order: the mul's gradient, then sigmoid_backward's grad * (1 - s) * s
    }
    if (!(x >= p.b && x <= p.c)) return 0.0f;  // outside the bounds, a NaN included: exactly zero whatever dy holds
    const float z = x * p.a;                   // (inside the bounds the clamp is the identity)
    return dy * (z > kSoftplusThreshold ? 1.0f : bijector_sigmoid(z));
}

// `lanes` lanes of kWidth floats (4: n % 4 == 0).  Forward: out = f(x).  Backward: out = dy * f'(x).
template <int kKind, bool kBackward, int kWidth>
__global__ __launch_bounds__(kBlock) void bijector_kernel(const float *x, const float *dy, float *out, int64_t lanes,
                                                          BijectorParams p) {
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < lanes; i += stride) {
        if constexpr (kWidth == 4) {
            const float4 v = reinterpret_cast<const float4 *>(x)[i];
            if constexpr (kBackward) {
                const float4 d = reinterpret_cast<const float4 *>(dy)[i];
                reinterpret_cast<float4 *>(out)[i] =
                    make_float4(bijector_backward<kKind>(v.x, d.x, p), bijector_backward<kKind>(v.y, d.y, p),
                                bijector_backward<kKind>(v.z, d.z, p), bijector_backward<kKind>(v.w, d.w, p));
            } else {
                reinterpret_cast<float4 *>(out)[i] = make_float4(bijector_forward<kKind>(v.x, p), bijector_forward<kKind>(v.y, p),
                                                                 bijector_forward<kKind>(v.z, p), bijector_forward<kKind>(v.w, p));
            }
        } else {
            if constexpr (kBackward)
                out[i] = bijector_backward<kKind>(x[i], dy[i], p);
            else
                out[i] = bijector_forward<kKind>(x[i], p);
        }
    }
}

template <int kKind, bool kBackward>
int launch_bijector(const float *x, const float *dy, float *out, int64_t n, const BijectorParams &p, void *stream) {
    const bool vec = n % 4 == 0 && aligned(x, 16) && aligned(dy, 16) && aligned(out, 16);  // (NULL is aligned)
    const int64_t lanes = vec ? n / 4 : n;
    int64_t blocks = ceil_div(lanes, kBlock);
    if (blocks > INT32_MAX) return CUSRL_E_UNSUPPORTED;  // more lanes than a grid of 32-bit extent has threads
    if (blocks > kBijectorMaxBlocks) blocks = kBijectorMaxBlocks;
    const dim3 grid{uint32_t(blocks)}, block{kBlock};
    if (vec)
        hipLaunchKernelGGL((bijector_kernel<kKind, kBackward, 4>), grid, block, 0, as_stream(stream), x, dy, out, lanes, p);
    else
        hipLaunchKernelGGL((bijector_kernel<kKind, kBackward, 1>), grid, block, 0, as_stream(stream), x, dy, out, lanes, p);
    return launch_status();
}

template <bool kBackward>
int dispatch_bijector(int kind, const float *x, const float *dy, float *out, int64_t n, float p0, float p1, float p2,
                      void *stream) {
    if (!x || !out || (kBackward && !dy) || n < 0) return CUSRL_E_INVALID;
    if (kind == CUSRL_BIJECTOR_SIGMOID) {
        if (n == 0) return 0;
        return launch_bijector<CUSRL_BIJECTOR_SIGMOID, kBackward>(x, dy, out, n, {p0, p1, 0.0f}, stream);
    }
    if (kind == CUSRL_BIJECTOR_SOFTPLUS) {
        if (!(p0 > 0.0f) || !(p1 <= p2)) return CUSRL_E_INVALID;  // (a NaN parameter fails either test)
        if (n == 0) return 0;
        return launch_bijector<CUSRL_BIJECTOR_SOFTPLUS, kBackward>(x, dy, out, n, {p0, p1, p2}, stream);
    }
    return CUSRL_E_INVALID;
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_bijector_fwd(int kind, const float *x, float *y, int64_t n, float p0, float p1, float p2, void *stream) {
    return dispatch_bijector<false>(kind, x, nullptr, y, n, p0, p1, p2, stream);
}

extern "C" int cusrl_bijector_bwd(int kind, const float *x, const float *dy, float *dx, int64_t n, float p0, float p1, float p2,
                                  void *stream) {
    return dispatch_bijector<true>(kind, x, dy, dx, n, p0, p1, p2, stream);
}
