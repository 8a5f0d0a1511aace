// Depthwise 2-D convolution, forward and both backward passes ("Depthwise convolution"): the spatial half of
// cusrl/nn/layer/separable_conv.py:52-64.  Every channel is a plane of its own with its own KH x KW taps, so the work is a stream:
// each input plane read, each output plane written.  The planes of an encoder are a few kilobytes; a thread owns ONE output
// element (forward: out, input gradient: dx) and gathers its taps through the caches — the halo a neighbour needs is the line
// this thread has just pulled into L1, and staging it in LDS would add a barrier per plane and save no memory traffic.  The
// input gradient is the same gather turned round (each dx element sums the windows that reach it): no atomics anywhere, and a
// position no window reads is the empty sum, +0.0f.  The parameter gradients are per-channel reductions over (n, oy, ox): float64
// sums in a fixed order, per-block partials and a finalize in block order, as csrc/layer_norm.hip does its column sums.
// One access width only: every load and store is 4 bytes, so any 4-byte aligned pointer gives the same bits.
#include "common.hpp"

namespace cusrl {
namespace {

constexpr int kMaxTaps = CUSRL_MAX_DWCONV_TAPS;
constexpr int kSlots = kMaxTaps + 1;        // a block's row of partials: the taps, then the bias sum in the last slot
constexpr int kMaxGrid = 2048;              // blocks of the element-wise passes; the rest is a grid stride
constexpr int kParamsElemsPerThread = 4;    // below the cap a thread of the parameter pass walks this many (n, oy, ox)
constexpr int kParamsMaxBlocks = 64;        // blocks per channel: what one thread of the finalize sums

// Index is int32_t whenever every element count and padded extent fits (with room for the grid stride), int64_t otherwise.
template <typename Index>
struct Geometry {
    Index C, H, W, Ho, Wo;
    Index SH, SW, PH, PW, DH, DW;
    int KH, KW;
};

template <typename Index>
__global__ __launch_bounds__(kBlock) void dwconv2d_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                              const float *__restrict__ bias, float *__restrict__ out,
                                                              Geometry<Index> g, Index total) {
    const Index stride = Index(gridDim.x) * kBlock;
    for (Index e = Index(blockIdx.x) * kBlock + Index(threadIdx.x); e < total; e += stride) {
        const Index ox = e % g.Wo, row = e / g.Wo;
        const Index oy = row % g.Ho, plane = row / g.Ho;
        const Index c = plane % g.C;
        const float *__restrict__ taps = w + c * Index(g.KH * g.KW);
        const float *__restrict__ image = x + plane * g.H * g.W;
        const Index y0 = oy * g.SH - g.PH, x0 = ox * g.SW - g.PW;
        float acc = bias != nullptr ? bias[c] : 0.f;
        for (int ky = 0; ky < g.KH; ++ky) {  // taps in (ky, kx) order, one rounded multiply and one rounded add each
            const Index iy = y0 + Index(ky) * g.DH;
            if (iy < 0 || iy >= g.H) continue;
            for (int kx = 0; kx < g.KW; ++kx) {
                const Index ix = x0 + Index(kx) * g.DW;
                if (ix < 0 || ix >= g.W) continue;
                acc = acc + taps[ky * g.KW + kx] * image[iy * g.W + ix];
            }
        }
        out[e] = acc;
    }
}

// The output coordinate whose window reaches input coordinate `i` through tap `k`, or -1: o * S - P + k * D == i, 0 <= o < limit.
template <typename Index>
__device__ __forceinline__ Index reaching_output(Index i, int k, Index S, Index P, Index D, Index limit) {
    const Index t = i + P - Index(k) * D;
    if (t < 0) return -1;
    const Index o = S == 1 ? t : t / S;
    return (o < limit && o * S == t) ? o : Index(-1);
}

template <typename Index>
__global__ __launch_bounds__(kBlock) void dwconv2d_bwd_input_kernel(const float *__restrict__ dout, const float *__restrict__ w,
                                                                    float *__restrict__ dx, Geometry<Index> g, Index total) {
    const Index stride = Index(gridDim.x) * kBlock;
    for (Index e = Index(blockIdx.x) * kBlock + Index(threadIdx.x); e < total; e += stride) {
        const Index ix = e % g.W, row = e / g.W;
        const Index iy = row % g.H, plane = row / g.H;
        const Index c = plane % g.C;
        const float *__restrict__ taps = w + c * Index(g.KH * g.KW);
        const float *__restrict__ image = dout + plane * g.Ho * g.Wo;
        float acc = 0.f;  // (what a position no window reads keeps)
        for (int ky = 0; ky < g.KH; ++ky) {
            const Index oy = reaching_output(iy, ky, g.SH, g.PH, g.DH, g.Ho);
            if (oy < 0) continue;
            for (int kx = 0; kx < g.KW; ++kx) {
                const Index ox = reaching_output(ix, kx, g.SW, g.PW, g.DW, g.Wo);
                if (ox < 0) continue;
                acc = acc + taps[ky * g.KW + kx] * image[oy * g.Wo + ox];
            }
        }
        dx[e] = acc;
    }
}

// Block b of channel c walks the (n, oy, ox) of that channel b * kBlock + thread, + blocks * kBlock, ... in ascending order; a
// thread keeps one float64 sum per tap (kTaps of them in registers: the tap loop is unrolled to its compile-time bound) and one
// for the bias.  Wave sums (wave_sum's order), then the four waves in index order; the only block of a channel writes dw and
// dbias itself, otherwise the sums go to the block's row [kSlots] of `partials`.
template <typename Index, int kTaps>
__global__ __launch_bounds__(kBlock) void dwconv2d_bwd_params_kernel(const float *__restrict__ x, const float *__restrict__ dout,
                                                                     float *__restrict__ dw, float *__restrict__ dbias,
                                                                     double *__restrict__ partials, Geometry<Index> g, Index M,
                                                                     int blocks) {
    __shared__ double sums[kWavesPerBlock][kSlots];
    const Index c = Index(blockIdx.x) / blocks;
    const int b = int(Index(blockIdx.x) % blocks), taps = g.KH * g.KW;
    double acc[kTaps], acc_bias = 0.0;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) acc[t] = 0.0;

    const Index stride = Index(blocks) * kBlock;
    for (Index m = Index(b) * kBlock + Index(threadIdx.x); m < M; m += stride) {
        const Index ox = m % g.Wo, row = m / g.Wo;
        const Index oy = row % g.Ho, plane = (row / g.Ho) * g.C + c;
        const float d = dout[(plane * g.Ho + oy) * g.Wo + ox];
        const float *__restrict__ image = x + plane * g.H * g.W;
        const Index y0 = oy * g.SH - g.PH, x0 = ox * g.SW - g.PW;
        acc_bias += double(d);
        int ky = 0, kx = 0;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            if (t < taps) {
                const Index iy = y0 + Index(ky) * g.DH, ix = x0 + Index(kx) * g.DW;
                if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) acc[t] += double(d) * double(image[iy * g.W + ix]);
                if (++kx == g.KW) kx = 0, ++ky;
            }
        }
    }

    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        if (t < taps) {
            const double total = wave_sum(acc[t]);
            if (lane == 0) sums[wave][t] = total;
        }
    }
    acc_bias = wave_sum(acc_bias);
    if (lane == 0) sums[wave][kMaxTaps] = acc_bias;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < taps || t == kMaxTaps) {
        double total = sums[0][t];
#pragma unroll
        for (int v = 1; v < kWavesPerBlock; ++v) total += sums[v][t];
        if (blocks > 1) partials[(int64_t(c) * blocks + b) * kSlots + t] = total;
        else if (t < taps) dw[c * Index(taps) + t] = float(total);
        else if (dbias != nullptr) dbias[c] = float(total);
    }
}

// One wave per channel: thread t sums slot t of the channel's `blocks` partial rows in block order.
__global__ __launch_bounds__(kWave) void dwconv2d_finalize_kernel(const double *__restrict__ partials, int blocks, int taps,
                                                                  float *__restrict__ dw, float *__restrict__ dbias) {
    const int64_t c = blockIdx.x;
    const int t = threadIdx.x;
    if (!(t < taps || (t == kMaxTaps && dbias != nullptr))) return;
    double total = 0.0;
    for (int b = 0; b < blocks; ++b) total += partials[(c * blocks + b) * kSlots + t];
    if (t < taps) dw[c * taps + t] = float(total);
    else dbias[c] = float(total);
}

struct Problem {
    int64_t N, C, H, W, Ho, Wo, KH, KW, SH, SW, PH, PW, DH, DW;
    int64_t in_total, out_total;  // N C H W and N C Ho Wo
    bool narrow;                  // every index fits int32_t
};

// Output extent of one axis by torch.nn.Conv2d's formula; false when an intermediate leaves int64.
inline bool output_extent(int64_t size, int64_t K, int64_t S, int64_t P, int64_t D, int64_t *extent) {
    int64_t span, padded;
    if (__builtin_mul_overflow(D, K - 1, &span) || __builtin_mul_overflow(P, int64_t(2), &padded) ||
        __builtin_add_overflow(padded, size, &padded))
        return false;
    *extent = padded - span - 1 < 0 ? 0 : (padded - span - 1) / S + 1;
    return true;
}

inline bool product(int64_t a, int64_t b, int64_t c, int64_t d, int64_t *out) {
    return !__builtin_mul_overflow(a, b, out) && !__builtin_mul_overflow(*out, c, out) && !__builtin_mul_overflow(*out, d, out);
}

// 0 with `p` filled, or the status to return (sizes only: the pointers are the caller's to check first).
inline int resolve(int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW,
                   int64_t DH, int64_t DW, Problem *p) {
    if (N < 0 || C < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || SH < 1 || SW < 1 || DH < 1 || DW < 1 || PH < 0 || PW < 0)
        return CUSRL_E_INVALID;
    if (KH > kMaxTaps || KW > kMaxTaps || KH * KW > kMaxTaps) return CUSRL_E_UNSUPPORTED;
    int64_t Ho, Wo;
    if (!output_extent(H, KH, SH, PH, DH, &Ho) || !output_extent(W, KW, SW, PW, DW, &Wo)) return CUSRL_E_UNSUPPORTED;
    if (Ho < 1 || Wo < 1) return CUSRL_E_INVALID;
    *p = Problem{N, C, H, W, Ho, Wo, KH, KW, SH, SW, PH, PW, DH, DW, 0, 0, false};
    // (with N == 0 the products are those of one image: the sizes are judged the same way whatever the batch)
    const int64_t images = N < 1 ? 1 : N;
    if (!product(images, C, H, W, &p->in_total) || !product(images, C, Ho, Wo, &p->out_total)) return CUSRL_E_UNSUPPORTED;
    if (C > INT32_MAX / (kParamsMaxBlocks * int64_t(kSlots))) return CUSRL_E_UNSUPPORTED;  // (the parameter pass's grid)
    const int64_t room = int64_t(INT32_MAX) - int64_t(kMaxGrid) * kBlock;  // an index plus one grid stride stays inside int32
    p->narrow = p->in_total <= room && p->out_total <= room && H + 2 * PH <= room && W + 2 * PW <= room;
    return 0;
}

template <typename Index>
inline Geometry<Index> geometry(const Problem &p) {
    return Geometry<Index>{Index(p.C),  Index(p.H),  Index(p.W),  Index(p.Ho), Index(p.Wo), Index(p.SH), Index(p.SW),
                           Index(p.PH), Index(p.PW), Index(p.DH), Index(p.DW), int(p.KH),   int(p.KW)};
}

inline dim3 elementwise_grid(int64_t total) {
    const int64_t want = ceil_div(total, kBlock);
    return dim3(uint32_t(want > kMaxGrid ? kMaxGrid : want));
}

inline int params_blocks(int64_t M) {
    const int64_t want = ceil_div(M, int64_t(kBlock) * kParamsElemsPerThread);
    return int(want < 1 ? 1 : want > kParamsMaxBlocks ? kParamsMaxBlocks : want);
}

template <typename Index, int kTaps>
inline void launch_params_tier(const float *x, const float *dout, float *dw, float *dbias, double *partials, const Problem &p, int blocks,
                          hipStream_t q) {
    hipLaunchKernelGGL((dwconv2d_bwd_params_kernel<Index, kTaps>), dim3(uint32_t(p.C * blocks)), dim3(kBlock), 0, q, x, dout, dw,
                       dbias, partials, geometry<Index>(p), Index(p.N * p.Ho * p.Wo), blocks);
}

template <typename Index>
inline void launch_params(const float *x, const float *dout, float *dw, float *dbias, double *partials, const Problem &p, int blocks,
                          hipStream_t q) {
    const int64_t taps = p.KH * p.KW;  // (one instantiation per register budget: 3 x 3, 5 x 5, 7 x 7)
    if (taps <= 9) launch_params_tier<Index, 9>(x, dout, dw, dbias, partials, p, blocks, q);
    else if (taps <= 25) launch_params_tier<Index, 25>(x, dout, dw, dbias, partials, p, blocks, q);
    else launch_params_tier<Index, kMaxTaps>(x, dout, dw, dbias, partials, p, blocks, q);
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_dwconv2d_fwd(const float *x, const float *w, const float *bias, float *out, int64_t N, int64_t C, int64_t H,
                                  int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW, int64_t DH,
                                  int64_t DW, void *stream) {
    if (!x || !w || !out) return CUSRL_E_INVALID;
    Problem p;
    if (int rc = resolve(N, C, H, W, KH, KW, SH, SW, PH, PW, DH, DW, &p)) return rc;
    if (N == 0) return 0;
    if (p.narrow)
        hipLaunchKernelGGL(dwconv2d_fwd_kernel<int32_t>, elementwise_grid(p.out_total), dim3(kBlock), 0, as_stream(stream), x, w, bias,
                           out, geometry<int32_t>(p), int32_t(p.out_total));
    else
        hipLaunchKernelGGL(dwconv2d_fwd_kernel<int64_t>, elementwise_grid(p.out_total), dim3(kBlock), 0, as_stream(stream), x, w, bias,
                           out, geometry<int64_t>(p), p.out_total);
    return launch_status();
}

extern "C" int cusrl_dwconv2d_bwd_input(const float *dout, const float *w, float *dx, int64_t N, int64_t C, int64_t H, int64_t W,
                                        int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW, int64_t DH,
                                        int64_t DW, void *stream) {
    if (!dout || !w || !dx) return CUSRL_E_INVALID;
    Problem p;
    if (int rc = resolve(N, C, H, W, KH, KW, SH, SW, PH, PW, DH, DW, &p)) return rc;
    if (N == 0) return 0;
    if (p.narrow)
        hipLaunchKernelGGL(dwconv2d_bwd_input_kernel<int32_t>, elementwise_grid(p.in_total), dim3(kBlock), 0, as_stream(stream), dout,
                           w, dx, geometry<int32_t>(p), int32_t(p.in_total));
    else
        hipLaunchKernelGGL(dwconv2d_bwd_input_kernel<int64_t>, elementwise_grid(p.in_total), dim3(kBlock), 0, as_stream(stream), dout,
                           w, dx, geometry<int64_t>(p), p.in_total);
    return launch_status();
}

extern "C" int64_t cusrl_dwconv2d_num_partials(int64_t N, int64_t C, int64_t Ho, int64_t Wo) {
    if (N <= 0 || C <= 0 || Ho <= 0 || Wo <= 0) return 0;
    int64_t M, count;
    if (!product(N, Ho, Wo, 1, &M)) return -1;
    const int blocks = params_blocks(M);
    if (blocks == 1) return 0;
    return product(C, blocks, kSlots, 1, &count) ? count : -1;
}

extern "C" int cusrl_dwconv2d_bwd_params(const float *x, const float *dout, float *dw, float *dbias, double *partials, int64_t N,
                                         int64_t C, int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH,
                                         int64_t PW, int64_t DH, int64_t DW, void *stream) {
    if (!x || !dout || !dw) return CUSRL_E_INVALID;
    Problem p;
    if (int rc = resolve(N, C, H, W, KH, KW, SH, SW, PH, PW, DH, DW, &p)) return rc;
    if (N == 0) return 0;
    const int blocks = params_blocks(p.N * p.Ho * p.Wo);
    if (blocks > 1 && !partials) return CUSRL_E_INVALID;
    hipStream_t q = as_stream(stream);
    if (p.narrow) launch_params<int32_t>(x, dout, dw, dbias, partials, p, blocks, q);
    else launch_params<int64_t>(x, dout, dw, dbias, partials, p, blocks, q);
    if (int rc = launch_status()) return rc;
    if (blocks == 1) return 0;  // the channel's one block wrote dw and dbias itself
    hipLaunchKernelGGL(dwconv2d_finalize_kernel, dim3(uint32_t(p.C)), dim3(kWave), 0, q, partials, blocks, int(p.KH * p.KW), dw, dbias);
    return launch_status();
}
