// Gates and GLU activations, forward and backward ("Gates and GLU"): everything between the GEMMs of
// cusrl/nn/layer/gate.py:36-136 and cusrl/nn/layer/activation.py:7-26 as one launch per direction.  The formulas, the operands
// each kind uses and the error codes are in include/cusrl_hip.h.  The launch shape is csrc/column_affine.hip's: a lane moves
// 16 bytes when the width is a multiple of 4 and every pointer is 16-byte aligned, 4 bytes otherwise (the same arithmetic per
// element, so the same bits), the grid is capped and strides over the rest, element indices are 64-bit.  The backward
// recomputes sigmoid and tanh from the saved pre-activations.  Outputs alias nothing.
#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kGateMaxBlocks = 2048;  // 8 blocks per CU; the grid strides over what is left

__device__ __forceinline__ float gate_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }  // (gru.hip's gru_sigmoid)

// ---- a lane's elements: 4 adjacent floats of one row, or one float
template <int kWidth>
struct Lane {
    float v[kWidth];
};

template <int kWidth>
__device__ __forceinline__ Lane<kWidth> load_lane(const float *p, int64_t i) {
    Lane<kWidth> lane;
    if constexpr (kWidth == 4) {
        const float4 t = reinterpret_cast<const float4 *>(p)[i];
        lane.v[0] = t.x, lane.v[1] = t.y, lane.v[2] = t.z, lane.v[3] = t.w;
    } else {
        lane.v[0] = p[i];
    }
    return lane;
}

template <int kWidth>
__device__ __forceinline__ void store_lane(float *p, int64_t i, const Lane<kWidth> &lane) {
    if constexpr (kWidth == 4)
        reinterpret_cast<float4 *>(p)[i] = make_float4(lane.v[0], lane.v[1], lane.v[2], lane.v[3]);
    else
        p[i] = lane.v[0];
}

// pre-activation with its optional second addend, `first + second` in the reference's order
template <int kWidth>
__device__ __forceinline__ Lane<kWidth> load_pre(const float *first, const float *second, int64_t i) {
    Lane<kWidth> lane = load_lane<kWidth>(first, i);
    if (second) {
        const Lane<kWidth> more = load_lane<kWidth>(second, i);
#pragma unroll
        for (int k = 0; k < kWidth; ++k) lane.v[k] = lane.v[k] + more.v[k];
    }
    return lane;
}

// ---- which operands a kind touches (include/cusrl_hip.h's table)
constexpr bool fwd_uses_y(int kind) { return kind == CUSRL_GATE_INPUT || kind == CUSRL_GATE_OUTPUT || kind == CUSRL_GATE_HIGHWAY; }
constexpr bool uses_q(int kind) { return kind == CUSRL_GATE_SIGMOID_TANH || kind == CUSRL_GATE_GRU_OUT; }
constexpr bool bwd_uses_x(int kind) { return kind != CUSRL_GATE_OUTPUT && kind != CUSRL_GATE_SIGMOID_TANH; }  // reads x, writes dx
constexpr bool bwd_uses_y(int kind) { return kind == CUSRL_GATE_OUTPUT || kind == CUSRL_GATE_HIGHWAY; }      // reads y, writes dy

struct GateOperands {
    const float *x, *y, *p, *p2, *q, *q2, *dout;
    float *out, *dx, *dy, *dp, *dq;
};

template <int kKind>
__device__ __forceinline__ float gate_forward(float x, float y, float p, float q) {
    const float g = gate_sigmoid(p);
    if (kKind == CUSRL_GATE_INPUT) return g * x + y;
    if (kKind == CUSRL_GATE_OUTPUT) return x + g * y;
    if (kKind == CUSRL_GATE_HIGHWAY) return g * x + (1.0f - g) * y;
    if (kKind == CUSRL_GATE_SIGMOID_TANH) return x + g * tanhf(q);
    if (kKind == CUSRL_GATE_GRU_RESET) return g * x;
    return (1.0f - g) * x + g * tanhf(q);  // GRU_OUT
}

// What the backward needs of a sigmoid at pre-activation v: g = s(v) as the forward computes it, and its complement 1 - g and
// slope g (1 - g) WITHOUT the cancellation of `1 - g` near g = 1 (at v = 8 the rounded difference is off by 2e-4 of itself):
// with e = exp(-|v|), s(|v|) = 1 / (1 + e) and s(-|v|) = e / (1 + e), so the slope is their product.  Where the forward's g has
// rounded to exactly 0 or 1 the forward is constant in fp32 and the slope is exactly 0.
struct SigmoidTerms {
    float g, complement, slope;
};

__device__ __forceinline__ SigmoidTerms sigmoid_terms(float v) {
    const float e = expf(-fabsf(v));
    const float large = 1.0f / (1.0f + e), small = e * large;
    const float g = gate_sigmoid(v);
    return {g, v >= 0.0f ? small : large, (g == 0.0f || g == 1.0f) ? 0.0f : large * small};
}

// 1 - h h for h = tanh(v), by the same route: 4 u / (1 + u)^2 with u = exp(-2 |v|) (at v = 4 the rounded `1 - h h` is off by
// 5e-5 of itself); exactly 0 where the forward's h has rounded to +-1.
__device__ __forceinline__ float tanh_slope(float v, float h) {
    const float u = expf(-2.0f * fabsf(v));
    const float w = 1.0f / (1.0f + u);
    return fabsf(h) == 1.0f ? 0.0f : 4.0f * u * w * w;
}

// d = dout, p and q the summed pre-activations.
template <int kKind>
__device__ __forceinline__ void gate_backward(float x, float y, float p, float q, float d, float &dx, float &dy, float &dp, float &dq) {
    const SigmoidTerms s = sigmoid_terms(p);
    dx = dy = dq = 0.0f;  // (what a kind does not produce is not stored)
    if (kKind == CUSRL_GATE_INPUT || kKind == CUSRL_GATE_GRU_RESET) {
        dx = d * s.g;
        dp = d * x * s.slope;
    } else if (kKind == CUSRL_GATE_OUTPUT) {
        dy = d * s.g;
        dp = d * y * s.slope;
    } else if (kKind == CUSRL_GATE_HIGHWAY) {
        dx = d * s.g;
        dy = d * s.complement;
        dp = d * (x - y) * s.slope;
    } else {
        const float h = tanhf(q);
        dq = d * s.g * tanh_slope(q, h);
        if (kKind == CUSRL_GATE_SIGMOID_TANH) {
            dp = d * h * s.slope;
        } else {  // GRU_OUT
            dx = d * s.complement;
            dp = d * (h - x) * s.slope;
        }
    }
}

template <int kKind, int kWidth>
__global__ __launch_bounds__(kBlock) void gate_fwd_kernel(GateOperands a, int64_t lanes) {
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < lanes; i += stride) {
        const Lane<kWidth> x = load_lane<kWidth>(a.x, i);
        const Lane<kWidth> p = load_pre<kWidth>(a.p, a.p2, i);
        Lane<kWidth> y = {}, q = {}, out;
        if constexpr (fwd_uses_y(kKind)) y = load_lane<kWidth>(a.y, i);
        if constexpr (uses_q(kKind)) q = load_pre<kWidth>(a.q, a.q2, i);
#pragma unroll
        for (int k = 0; k < kWidth; ++k) out.v[k] = gate_forward<kKind>(x.v[k], y.v[k], p.v[k], q.v[k]);
        store_lane<kWidth>(a.out, i, out);
    }
}

template <int kKind, int kWidth>
__global__ __launch_bounds__(kBlock) void gate_bwd_kernel(GateOperands a, int64_t lanes) {
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < lanes; i += stride) {
        const Lane<kWidth> d = load_lane<kWidth>(a.dout, i);
        const Lane<kWidth> p = load_pre<kWidth>(a.p, a.p2, i);
        Lane<kWidth> x = {}, y = {}, q = {}, dx, dy, dp, dq;
        if constexpr (bwd_uses_x(kKind)) x = load_lane<kWidth>(a.x, i);
        if constexpr (bwd_uses_y(kKind)) y = load_lane<kWidth>(a.y, i);
        if constexpr (uses_q(kKind)) q = load_pre<kWidth>(a.q, a.q2, i);
#pragma unroll
        for (int k = 0; k < kWidth; ++k) gate_backward<kKind>(x.v[k], y.v[k], p.v[k], q.v[k], d.v[k], dx.v[k], dy.v[k], dp.v[k], dq.v[k]);
        store_lane<kWidth>(a.dp, i, dp);
        if constexpr (bwd_uses_x(kKind)) store_lane<kWidth>(a.dx, i, dx);
        if constexpr (bwd_uses_y(kKind)) store_lane<kWidth>(a.dy, i, dy);
        if constexpr (uses_q(kKind)) store_lane<kWidth>(a.dq, i, dq);
    }
}

bool all_aligned16(const GateOperands &a) {  // (NULL is aligned)
    return aligned(a.x, 16) && aligned(a.y, 16) && aligned(a.p, 16) && aligned(a.p2, 16) && aligned(a.q, 16) && aligned(a.q2, 16) &&
           aligned(a.dout, 16) && aligned(a.out, 16) && aligned(a.dx, 16) && aligned(a.dy, 16) && aligned(a.dp, 16) && aligned(a.dq, 16);
}

template <int kKind, bool kBackward>
int launch_gate(const GateOperands &a, int64_t rows, int64_t C, void *stream) {
    if (C > INT32_MAX || rows > INT64_MAX / C) return CUSRL_E_UNSUPPORTED;
    if (rows == 0) return 0;
    const bool vec = C % 4 == 0 && all_aligned16(a);
    const int64_t lanes = vec ? rows * C / 4 : rows * C;
    int64_t blocks = ceil_div(lanes, kBlock);
    if (blocks > kGateMaxBlocks) blocks = kGateMaxBlocks;
    const dim3 grid{uint32_t(blocks)}, block{kBlock};
    if (kBackward) {
        if (vec)
            hipLaunchKernelGGL((gate_bwd_kernel<kKind, 4>), grid, block, 0, as_stream(stream), a, lanes);
        else
            hipLaunchKernelGGL((gate_bwd_kernel<kKind, 1>), grid, block, 0, as_stream(stream), a, lanes);
    } else {
        if (vec)
            hipLaunchKernelGGL((gate_fwd_kernel<kKind, 4>), grid, block, 0, as_stream(stream), a, lanes);
        else
            hipLaunchKernelGGL((gate_fwd_kernel<kKind, 1>), grid, block, 0, as_stream(stream), a, lanes);
    }
    return launch_status();
}

template <bool kBackward>
int dispatch_gate(int kind, const GateOperands &a, int64_t rows, int64_t C, void *stream) {
    switch (kind) {
        case CUSRL_GATE_INPUT: return launch_gate<CUSRL_GATE_INPUT, kBackward>(a, rows, C, stream);
        case CUSRL_GATE_OUTPUT: return launch_gate<CUSRL_GATE_OUTPUT, kBackward>(a, rows, C, stream);
        case CUSRL_GATE_HIGHWAY: return launch_gate<CUSRL_GATE_HIGHWAY, kBackward>(a, rows, C, stream);
        case CUSRL_GATE_SIGMOID_TANH: return launch_gate<CUSRL_GATE_SIGMOID_TANH, kBackward>(a, rows, C, stream);
        case CUSRL_GATE_GRU_RESET: return launch_gate<CUSRL_GATE_GRU_RESET, kBackward>(a, rows, C, stream);
        case CUSRL_GATE_GRU_OUT: return launch_gate<CUSRL_GATE_GRU_OUT, kBackward>(a, rows, C, stream);
    }
    return CUSRL_E_INVALID;
}

bool known_gate(int kind) { return kind >= CUSRL_GATE_INPUT && kind <= CUSRL_GATE_GRU_OUT; }

// ---------------------------------------------------------------------------------------------------------------- GLU
constexpr float kInvSqrt2 = 0.70710678118654752440f;
constexpr float kInvSqrt2Pi = 0.39894228040143267794f;

// act(b) and act'(b).  Phi through erfcf: no cancellation in the left tail, where 1 + erff(.) has lost every digit.
template <int kKind>
__device__ __forceinline__ void glu_activation(float b, float &act, float &slope) {
    if (kKind == CUSRL_GLU_GEGLU) {
        const float cdf = 0.5f * erfcf(-b * kInvSqrt2);
        const float pdf = expf(-0.5f * b * b) * kInvSqrt2Pi;
        act = b * cdf;
        slope = cdf + b * pdf;
    } else {
        const float s = gate_sigmoid(b);
        act = b * s;
        slope = s + b * s * (1.0f - s);
    }
}

// `lanes` lanes of kWidth over out [rows, H]; lane i covers out elements [i * kWidth, ...) of row r at column c (kWidth == 4:
// H % 4 == 0, so a lane stays in one row), i.e. a = input[r * 2H + c] = input[e + r * H] and b = H further on.  Row and column
// are carried along, advanced by (row_step, col_step) = divmod(stride * kWidth, H) per grid stride.
template <int kKind, int kWidth, bool kBackward>
__global__ __launch_bounds__(kBlock) void glu_kernel(const float *input, const float *dout, float *out, int64_t lanes, int64_t H,
                                                     int64_t row_step, int64_t col_step) {
    const int64_t stride = int64_t(gridDim.x) * kBlock;
    int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    int64_t r = i * kWidth / H, c = i * kWidth % H;
    for (; i < lanes; i += stride) {
        const int64_t at = (i * kWidth + r * H) / kWidth;  // lane index of a within input; b is H / kWidth lanes on
        const Lane<kWidth> a = load_lane<kWidth>(input, at), b = load_lane<kWidth>(input, at + H / kWidth);
        Lane<kWidth> first, second;
        if constexpr (kBackward) {
            const Lane<kWidth> d = load_lane<kWidth>(dout, i);
#pragma unroll
            for (int k = 0; k < kWidth; ++k) {
                float act, slope;
                glu_activation<kKind>(b.v[k], act, slope);
                first.v[k] = d.v[k] * act;
                second.v[k] = d.v[k] * a.v[k] * slope;
            }
            store_lane<kWidth>(out, at, first);
            store_lane<kWidth>(out, at + H / kWidth, second);
        } else {
#pragma unroll
            for (int k = 0; k < kWidth; ++k) {
                float act, slope;
                glu_activation<kKind>(b.v[k], act, slope);
                first.v[k] = a.v[k] * act;
            }
            store_lane<kWidth>(out, i, first);
        }
        r += row_step;
        c += col_step;
        if (c >= H) c -= H, ++r;
    }
}

template <int kKind, bool kBackward>
int launch_glu(const float *input, const float *dout, float *out, int64_t rows, int64_t H, void *stream) {
    if (H > INT32_MAX / 2 || rows > INT64_MAX / (2 * H)) return CUSRL_E_UNSUPPORTED;
    if (rows == 0) return 0;
    const bool vec = H % 4 == 0 && aligned(input, 16) && aligned(dout, 16) && aligned(out, 16);
    const int width = vec ? 4 : 1;
    const int64_t lanes = rows * H / width;
    int64_t blocks = ceil_div(lanes, kBlock);
    if (blocks > kGateMaxBlocks) blocks = kGateMaxBlocks;
    const int64_t step = blocks * kBlock * width;
    const dim3 grid{uint32_t(blocks)}, block{kBlock};
    if (vec)
        hipLaunchKernelGGL((glu_kernel<kKind, 4, kBackward>), grid, block, 0, as_stream(stream), input, dout, out, lanes, H, step / H,
                           step % H);
    else
        hipLaunchKernelGGL((glu_kernel<kKind, 1, kBackward>), grid, block, 0, as_stream(stream), input, dout, out, lanes, H, step / H,
                           step % H);
    return launch_status();
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_gate_fwd(int kind, const float *x, const float *y, const float *p, const float *p2, const float *q,
                              const float *q2, float *out, int64_t rows, int64_t C, void *stream) {
    if (!known_gate(kind) || !x || !p || !out || rows < 0 || C < 1) return CUSRL_E_INVALID;
    if ((fwd_uses_y(kind) && !y) || (uses_q(kind) && !q)) return CUSRL_E_INVALID;
    GateOperands a = {};
    a.x = x, a.p = p, a.p2 = p2, a.out = out;
    if (fwd_uses_y(kind)) a.y = y;
    if (uses_q(kind)) a.q = q, a.q2 = q2;
    return dispatch_gate<false>(kind, a, rows, C, stream);
}

extern "C" int cusrl_gate_bwd(int kind, const float *x, const float *y, const float *p, const float *p2, const float *q,
                              const float *q2, const float *dout, float *dx, float *dy, float *dp, float *dq, int64_t rows,
                              int64_t C, void *stream) {
    if (!known_gate(kind) || !p || !dout || !dp || rows < 0 || C < 1) return CUSRL_E_INVALID;
    if ((bwd_uses_x(kind) && (!x || !dx)) || (bwd_uses_y(kind) && (!y || !dy)) || (uses_q(kind) && (!q || !dq))) return CUSRL_E_INVALID;
    GateOperands a = {};
    a.p = p, a.p2 = p2, a.dout = dout, a.dp = dp;
    if (bwd_uses_x(kind)) a.x = x, a.dx = dx;
    if (bwd_uses_y(kind)) a.y = y, a.dy = dy;
    if (uses_q(kind)) a.q = q, a.q2 = q2, a.dq = dq;
    return dispatch_gate<true>(kind, a, rows, C, stream);
}

extern "C" int cusrl_glu_fwd(int kind, const float *input, float *out, int64_t rows, int64_t H, void *stream) {
    if (!input || !out || rows < 0 || H < 1) return CUSRL_E_INVALID;
    if (kind == CUSRL_GLU_GEGLU) return launch_glu<CUSRL_GLU_GEGLU, false>(input, nullptr, out, rows, H, stream);
    if (kind == CUSRL_GLU_SWIGLU) return launch_glu<CUSRL_GLU_SWIGLU, false>(input, nullptr, out, rows, H, stream);
    return CUSRL_E_INVALID;
}

extern "C" int cusrl_glu_bwd(int kind, const float *input, const float *dout, float *dinput, int64_t rows, int64_t H, void *stream) {
    if (!input || !dout || !dinput || rows < 0 || H < 1) return CUSRL_E_INVALID;
    if (kind == CUSRL_GLU_GEGLU) return launch_glu<CUSRL_GLU_GEGLU, true>(input, dout, dinput, rows, H, stream);
    if (kind == CUSRL_GLU_SWIGLU) return launch_glu<CUSRL_GLU_SWIGLU, true>(input, dout, dinput, rows, H, stream);
    return CUSRL_E_INVALID;
}
