// Per-column affine map over [rows, C] with fixed statistics, forward and backward ("Column affine"): the arithmetic
// of cusrl/nn/module/normalization.py:52 (`(input - mean) / std`) and :89 (`input * std + mean`) and of what torch's autograd
// gives for them (`dy / std`, `dy * std`; mean and std are not trainable, so there is no column reduction).  Every result is
// the correctly rounded IEEE operation torch's own expression performs — a subtraction then a DIVISION (no reciprocal), a
// multiplication then an addition (the library is built with -ffp-contract=off: no fma) — so both directions give torch's
// bits.  One launch; a lane moves 16 bytes (4 adjacent columns of one row) when C % 4 == 0 and every pointer is 16-byte
// aligned, one element otherwise.  Each lane loads its operands before it stores, so `out` may be `x` and `dx` may be `dy`
// (which is why those two carry no __restrict__).
#include "common.hpp"
#include "running_stats.hpp"

namespace cusrl {
namespace {

enum AffineOp { kNormalize, kDenormalize, kDivide, kScale };

constexpr int kAffineMaxBlocks = 2048;  // 8 blocks per CU; the grid strides over what is left

template <int kOp>
__device__ __forceinline__ float affine(float v, float m, float s) {
    if (kOp == kNormalize) return normalized(v, m, s);
    if (kOp == kDenormalize) return v * s + m;  // (two roundings: -ffp-contract=off)
    if (kOp == kDivide) return v / s;
    return v * s;
}

// `E` elements in lanes of kWidth (4: E % 4 == 0 and C % 4 == 0, so a lane's columns belong to one row).  A thread's column is
// carried along instead of being divided out of its 64-bit index every time: it advances by `step` = (stride * kWidth) % C.
template <int kOp, int kWidth>
__global__ __launch_bounds__(kBlock) void column_affine_kernel(const float *x, const float *__restrict__ mean,
                                                               const float *__restrict__ std, float *out, int64_t E, int64_t C,
                                                               int64_t step) {
    constexpr bool kHasMean = kOp == kNormalize || kOp == kDenormalize;
    const int64_t lanes = E / kWidth;
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    int64_t c = (i * kWidth) % C;
    for (; i < lanes; i += stride) {
        if (kWidth == 4) {
            const float4 v = reinterpret_cast<const float4 *>(x)[i];
            const float4 s = *reinterpret_cast<const float4 *>(std + c);
            const float4 m = kHasMean ? *reinterpret_cast<const float4 *>(mean + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4 *>(out)[i] = make_float4(affine<kOp>(v.x, m.x, s.x), affine<kOp>(v.y, m.y, s.y),
                                                             affine<kOp>(v.z, m.z, s.z), affine<kOp>(v.w, m.w, s.w));
        } else {
            out[i] = affine<kOp>(x[i], kHasMean ? mean[c] : 0.f, std[c]);
        }
        c += step;
        if (c >= C) c -= C;
    }
}

template <int kOp>
int launch_column_affine(const float *x, const float *mean, const float *std, float *out, int64_t rows, int64_t C, void *stream) {
    if (C > INT32_MAX || rows > INT64_MAX / C) return CUSRL_E_UNSUPPORTED;
    if (rows == 0) return 0;
    const int64_t E = rows * C;
    const bool vec = C % 4 == 0 && aligned(x, 16) && aligned(out, 16) && aligned(std, 16) && aligned(mean, 16);  // (NULL is aligned)
    const int64_t lanes = vec ? E / 4 : E;
    int64_t blocks = ceil_div(lanes, kBlock);
    if (blocks > kAffineMaxBlocks) blocks = kAffineMaxBlocks;
    const int64_t stride = blocks * kBlock;
    if (vec)
        hipLaunchKernelGGL((column_affine_kernel<kOp, 4>), dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), x, mean, std,
                           out, E, C, (stride * 4) % C);
    else
        hipLaunchKernelGGL((column_affine_kernel<kOp, 1>), dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), x, mean, std,
                           out, E, C, stride % C);
    return launch_status();
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_column_affine_fwd(const float *x, const float *mean, const float *std, float *out, int64_t rows, int64_t C,
                                       int inverse, void *stream) {
    if (!x || !mean || !std || !out || rows < 0 || C < 1 || (inverse != 0 && inverse != 1)) return CUSRL_E_INVALID;
    return inverse ? launch_column_affine<kDenormalize>(x, mean, std, out, rows, C, stream)
                   : launch_column_affine<kNormalize>(x, mean, std, out, rows, C, stream);
}

extern "C" int cusrl_column_affine_bwd(const float *dy, const float *std, float *dx, int64_t rows, int64_t C, int inverse,
                                       void *stream) {
    if (!dy || !std || !dx || rows < 0 || C < 1 || (inverse != 0 && inverse != 1)) return CUSRL_E_INVALID;
    return inverse ? launch_column_affine<kScale>(dy, nullptr, std, dx, rows, C, stream)
                   : launch_column_affine<kDivide>(dy, nullptr, std, dx, rows, C, stream);
}
