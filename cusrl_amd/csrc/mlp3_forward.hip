// Inference pass of a THREE-hidden-layer actor / critic MLP for gfx950: out = W4 act(W3 act(W2 act(W1 x + b1) + b2) + b3) + b4
// with act one of ReLU / ELU / Tanh — the (512, 256, 128) and (128, 128, 128) ELU networks of the robotics experiments — as ONE
// launch, optionally with the acting path's sampling epilogue behind it (mlp_tail.hpp: the tail mlp_forward.hip has).
//
// Formulation: mlp_forward.hip's (transposed, features x rows, v_mfma_f32_16x16x4_f32; read its header first).  A lane's float4
// of a weight row is the A operand of four consecutive MFMAs of a k-block; the four accumulator registers a lane holds of an
// output tile are the B operands of the next layer's k-block of the same index.  The 4 waves split every layer's OUTPUT
// features (wave w owns tiles T w .. T w + T - 1), so a layer's tiles meet in LDS as [tile][lane] float4 before the next layer
// reads all of them: after layer 1, after layer 2, and the head's four [out, 16] partial sums — three exchanges (barriers) per
// row tile.  Bias starts the accumulator; the activation is applied to the accumulator registers before they are published.
//
// Two regimes, one body.
//   * Resident (CH == 0): (128, 128, 128) and (256, 128, 64).  All four weight matrices (<= 57 K floats, <= ~230 registers per
//     lane) are loaded once per workgroup and stay in registers while the workgroup walks row tiles with stride gridDim.x.
//   * Streamed (CH > 0): (512, 256, 128).  W1, W3, W4 are resident (264 registers per lane at K = 64); W2 — 512 KB, a CU's whole
//     register file — is read from L2 for every row tile in chunks of CH k-blocks (CH x T2 float4 per lane, each a plain
//     16-byte load in the A-operand layout), double-buffered in registers: chunk c + 1 is requested before the MFMAs of chunk
//     c are issued, and the first chunk of the NEXT tile behind the last chunk of this one.  R 16-row sub-tiles share one
//     fetch of a chunk (R = 1: 16-row tiles, every CU busy at 4096 rows; R = 2: half the L2 traffic per row for the passes
//     over a whole buffer).  Every sub-tile has accumulators of its own and sees the k-blocks in the same order, so a row's
//     sums do not depend on R, on the tile or on the workgroup it lands in.
//
// Activations with the expressions of cusrl_bias_act (bias_act.hip): v > 0 ? v : alpha * expm1f(v) and tanhf(v), the accurate
// functions; ReLU is relu4 (a NaN stays a NaN, -0 becomes +0).  fp32 MFMA accumulation as in the library's fp32 GEMMs.
#include "mlp_tail.hpp"

namespace cusrl {

struct Mlp3ForwardArgs {
    const float *x;
    const float *w1, *b1, *w2, *b2, *w3, *b3, *w4, *b4;
    float *out;        // [rows, A] (NULL: not stored)
    const float *std;  // sampling epilogue (all NULL: none): [A] vector
    const float *eps;  // [rows, A]
    float *action, *logp, *std_out;
    int64_t rows;
    int K, A;
    float alpha;
};

// T1 / T2 / T3: 16-feature tiles of the hidden layers per wave (H = 64 T); KB: 16-wide k-blocks of the input; R: 16-row
// sub-tiles evaluated per pass of the weights; CH: k-blocks per streamed chunk of W2 (0: W2 resident).
template <int ACT, int T1, int T2, int T3, int KB, int R, int CH>
__global__ __launch_bounds__(kMlpThreads) void mlp3_forward_kernel(const Mlp3ForwardArgs p) {
    constexpr int NT1 = kMlpWaves * T1, NT2 = kMlpWaves * T2;  // tiles of layer 1 / 2 = k-blocks of layer 2 / 3
    constexpr int H1 = 16 * NT1, H2 = 16 * NT2, H3 = 16 * kMlpWaves * T3;
    constexpr bool kStream = CH > 0;
    constexpr int kChunks = kStream ? NT1 / CH : 2;
    static_assert(!kStream || (NT1 % CH == 0 && kChunks % 2 == 0), "chunk c lives in buffer c & 1, also across row tiles");
    __shared__ float4 hidden1[R][NT1][kWave];
    __shared__ float4 hidden2[R][NT2][kWave];
    __shared__ float4 partial[R][kMlpWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int i = lane & 15, kk = lane >> 4;
    const int K = p.K, A = p.A;
    const float alpha = p.alpha;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // ---- this wave's resident weights, once
    float4 a1[T1][KB], a2[kStream ? 1 : T2][kStream ? 1 : NT1], a3[T3][NT2], a4[T3];
    float4 ring[2][kStream ? CH : 1][T2];  // streamed W2: two chunks of CH k-blocks for this wave's T2 tiles
    mfma_f32x4 c1[T1], c2[T2], c3[T3], c4;
#pragma unroll
    for (int t1 = 0; t1 < T1; ++t1) {
        const int n = 16 * (T1 * wave + t1);
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            // (unpredicated 16-byte load from a clamped address, then a select: a predicated load is split into four guarded ones)
            const int k = 16 * t + 4 * kk;
            const float4 v = *reinterpret_cast<const float4 *>(p.w1 + int64_t(n + i) * K + (k < K ? k : 0));
            a1[t1][t] = k < K ? v : zero4;
        }
        c1[t1] = from_bias(p.b1 + n + 4 * kk);
    }
    const int64_t tiles = (p.rows + R * kMlpRows - 1) / (R * kMlpRows);  // passes: R sub-tiles each
    // the input rows of a pass are requested one pass ahead
    float4 ahead[R][KB];
    auto request = [&](int64_t tile) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = min((tile * R + r) * kMlpRows + i, p.rows - 1);  // (rows past the end re-read the last row; nothing is stored for them)
#pragma unroll
            for (int t = 0; t < KB; ++t) {
                const int k = 16 * t + 4 * kk;
                ahead[r][t] = *reinterpret_cast<const float4 *>(p.x + row * K + (k < K ? k : 0));
            }
        }
    };
    request(min(int64_t(blockIdx.x), tiles - 1));
    // W2: this lane's row of tile t2 is w2row + 16 H1 t2; k-block t adds 16 t
    const float *w2row = p.w2 + int64_t(16 * T2 * wave + i) * H1 + 4 * kk;
    auto fetch = [&](int chunk, int buffer) {
#pragma unroll
        for (int q = 0; q < (kStream ? CH : 0); ++q)
#pragma unroll
            for (int t2 = 0; t2 < T2; ++t2)
                ring[buffer][q][t2] = *reinterpret_cast<const float4 *>(w2row + 16 * H1 * t2 + 16 * (chunk * CH + q));
    };
    if constexpr (kStream) fetch(0, 0);
#pragma unroll
    for (int t2 = 0; t2 < T2; ++t2) {
        if constexpr (!kStream) {
#pragma unroll
            for (int t = 0; t < NT1; ++t) a2[t2][t] = *reinterpret_cast<const float4 *>(w2row + 16 * H1 * t2 + 16 * t);
        }
        c2[t2] = from_bias(p.b2 + 16 * (T2 * wave + t2) + 4 * kk);
    }
#pragma unroll
    for (int t3 = 0; t3 < T3; ++t3) {
        const int n = 16 * (T3 * wave + t3);
#pragma unroll
        for (int t = 0; t < NT2; ++t) a3[t3][t] = *reinterpret_cast<const float4 *>(p.w3 + int64_t(n + i) * H2 + 16 * t + 4 * kk);
        c3[t3] = from_bias(p.b3 + n + 4 * kk);
        // the head: rows = outputs (i < A), k-block = this wave's own tile t3 of the third hidden layer
        const float4 v = *reinterpret_cast<const float4 *>(p.w4 + int64_t(i < A ? i : 0) * H3 + n + 4 * kk);
        a4[t3] = i < A ? v : zero4;
    }
    c4 = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    if (wave == 0 && p.b4) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) c4[reg] = 4 * kk + reg < A ? p.b4[4 * kk + reg] : 0.f;
    }

    // sampling epilogue (wave 0): this lane's four std values once, its eps values requested at the top of every pass
    float sigma[4] = {1.f, 1.f, 1.f, 1.f}, noise[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) noise[r][0] = noise[r][1] = noise[r][2] = noise[r][3] = 0.f;
    const bool sampling = wave == 0 && p.eps != nullptr;
    if (sampling) mlp_tail_sigma(p.std, A, kk, sigma);

    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * R * kMlpRows;
        if (sampling) {
#pragma unroll
            for (int r = 0; r < R; ++r) mlp_tail_noise(p.eps, p.rows, A, row0 + r * kMlpRows, lane, noise[r]);
        }
        float4 xb[R][KB];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int t = 0; t < KB; ++t) xb[r][t] = 16 * t + 4 * kk < K ? ahead[r][t] : zero4;
        request(min(tile + gridDim.x, tiles - 1));
        // ---- layer 1: this wave's T1 tiles of H1^T, to LDS
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int t1 = 0; t1 < T1; ++t1) {
                mfma_f32x4 acc = c1[t1];
#pragma unroll
                for (int t = 0; t < KB; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a1[t1][t], j), pick(xb[r][t], j), acc, 0, 0, 0);
                acc = act4<ACT>(acc, alpha);
                hidden1[r][T1 * wave + t1][lane] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        __syncthreads();
        // ---- layer 2: this wave's T2 tiles of H2^T over all NT1 k-blocks, to LDS
        mfma_f32x4 h2[R][T2];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int t2 = 0; t2 < T2; ++t2) h2[r][t2] = c2[t2];
        auto layer2_block = [&](int t, const float4 (&a)[T2]) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float4 hb = hidden1[r][t][lane];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t2 = 0; t2 < T2; ++t2)
                        h2[r][t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a[t2], j), pick(hb, j), h2[r][t2], 0, 0, 0);
            }
        };
        if constexpr (kStream) {
#pragma unroll
            for (int c = 0; c < kChunks; ++c) {
                fetch((c + 1) % kChunks, (c + 1) & 1);  // (behind the last chunk: chunk 0 again, for the next pass)
                __builtin_amdgcn_sched_barrier(0);      // the request stays in front of the MFMAs it overlaps with
#pragma unroll
                for (int q = 0; q < CH; ++q) layer2_block(c * CH + q, ring[c & 1][q]);
            }
        } else {
#pragma unroll
            for (int t = 0; t < NT1; ++t) {
                float4 a[T2];
#pragma unroll
                for (int t2 = 0; t2 < T2; ++t2) a[t2] = a2[t2][t];
                layer2_block(t, a);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int t2 = 0; t2 < T2; ++t2) {
                const mfma_f32x4 h = act4<ACT>(h2[r][t2], alpha);
                hidden2[r][T2 * wave + t2][lane] = make_float4(h[0], h[1], h[2], h[3]);
            }
        __syncthreads();
        // ---- layer 3 (this wave's T3 tiles over all NT2 k-blocks) and the head's partial product over those tiles
#pragma unroll
        for (int r = 0; r < R; ++r) {
            mfma_f32x4 h3[T3];
#pragma unroll
            for (int t3 = 0; t3 < T3; ++t3) h3[t3] = c3[t3];
#pragma unroll
            for (int t = 0; t < NT2; ++t) {
                const float4 hb = hidden2[r][t][lane];
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t3 = 0; t3 < T3; ++t3)
                        h3[t3] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a3[t3][t], j), pick(hb, j), h3[t3], 0, 0, 0);
            }
            mfma_f32x4 head = c4;
#pragma unroll
            for (int t3 = 0; t3 < T3; ++t3) {
                const mfma_f32x4 h = act4<ACT>(h3[t3], alpha);
#pragma unroll
                for (int j = 0; j < 4; ++j) head = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a4[t3], j), h[j], head, 0, 0, 0);
            }
            partial[r][wave][lane] = make_float4(head[0], head[1], head[2], head[3]);
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) mlp_tail(p, partial[r], row0 + r * kMlpRows, lane, sigma, noise[r]);
        }
    }
}

template <int ACT, int T1, int T2, int T3, int R, int CH>
static int launch_mlp3_kb(const Mlp3ForwardArgs &p, int kb, dim3 grid, hipStream_t s) {
    switch (kb) {
        case 1: hipLaunchKernelGGL((mlp3_forward_kernel<ACT, T1, T2, T3, 1, R, CH>), grid, dim3(kMlpThreads), 0, s, p); break;
        case 2: hipLaunchKernelGGL((mlp3_forward_kernel<ACT, T1, T2, T3, 2, R, CH>), grid, dim3(kMlpThreads), 0, s, p); break;
        case 3: hipLaunchKernelGGL((mlp3_forward_kernel<ACT, T1, T2, T3, 3, R, CH>), grid, dim3(kMlpThreads), 0, s, p); break;
        case 4: hipLaunchKernelGGL((mlp3_forward_kernel<ACT, T1, T2, T3, 4, R, CH>), grid, dim3(kMlpThreads), 0, s, p); break;
        default: return CUSRL_E_UNSUPPORTED;
    }
    return launch_status();
}

// W2 chunk depth of the streamed regime in k-blocks (x T2 = 4 tiles x 16 bytes per lane and buffer): 128 MFMAs (~4 K cycles of
// the matrix pipe) per wave cover one request either way; two sub-tiles take the shallower chunk for the registers their second
// set of accumulators and inputs needs
constexpr int kMlp3Chunk1 = 4, kMlp3Chunk2 = 2;

template <int ACT>
static int launch_mlp3(const Mlp3ForwardArgs &p, int64_t h1, int64_t h2, int kb, int64_t tiles, int cus, hipStream_t s) {
    // one workgroup (4 waves, one per SIMD) per CU; beyond that the tiles are walked with the resident weights in place
    const auto grid = [&](int64_t passes) { return dim3(uint32_t(passes < cus ? passes : cus)); };
    if (h1 == 128) return launch_mlp3_kb<ACT, 2, 2, 2, 1, 0>(p, kb, grid(tiles), s);
    if (h1 == 256) return launch_mlp3_kb<ACT, 4, 2, 1, 1, 0>(p, kb, grid(tiles), s);
    // (512, 256, 128): 16-row passes while they fill the CUs at most once, then two sub-tiles per fetch of a W2 chunk
    if (tiles <= cus) return launch_mlp3_kb<ACT, 8, 4, 2, 1, kMlp3Chunk1>(p, kb, grid(tiles), s);
    return launch_mlp3_kb<ACT, 8, 4, 2, 2, kMlp3Chunk2>(p, kb, grid(ceil_div(tiles, 2)), s);
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_mlp3_forward_supported(int64_t in_features, int64_t hidden1, int64_t hidden2, int64_t hidden3, int64_t out_features) {
    const bool widths = (hidden1 == 512 && hidden2 == 256 && hidden3 == 128) || (hidden1 == 256 && hidden2 == 128 && hidden3 == 64) ||
                        (hidden1 == 128 && hidden2 == 128 && hidden3 == 128);
    return in_features >= 4 && in_features % 4 == 0 && in_features <= 64 && widths && out_features >= 1 && out_features <= 16;
}

extern "C" int cusrl_mlp3_forward(const float *input, int64_t rows, int64_t in_features, const float *w1, const float *b1,
                                  int64_t hidden1, const float *w2, const float *b2, int64_t hidden2, const float *w3,
                                  const float *b3, int64_t hidden3, const float *w4, const float *b4, int64_t out_features,
                                  int activation, float alpha, float *output, const float *std, const float *eps, float *action,
                                  float *logp, float *std_out, void *stream) {
    if (rows < 0 || !input || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4) return CUSRL_E_INVALID;
    if (rows == 0) return 0;
    if (!cusrl_mlp3_forward_supported(in_features, hidden1, hidden2, hidden3, out_features)) return CUSRL_E_UNSUPPORTED;
    if (activation != CUSRL_ACT_RELU && activation != CUSRL_ACT_ELU && activation != CUSRL_ACT_TANH) return CUSRL_E_UNSUPPORTED;
    const bool sampling = eps != nullptr;
    if (sampling ? !(std && action && logp) : (std || action || logp || std_out)) return CUSRL_E_INVALID;
    if (!sampling && !output) return CUSRL_E_INVALID;
    if (!aligned(input, 16) || !aligned(w1, 16) || !aligned(b1, 16) || !aligned(w2, 16) || !aligned(b2, 16) || !aligned(w3, 16) ||
        !aligned(b3, 16) || !aligned(w4, 16) || (output && out_features % 4 == 0 && !aligned(output, 16)))
        return CUSRL_E_UNSUPPORTED;
    Mlp3ForwardArgs p;
    p.x = input, p.w1 = w1, p.b1 = b1, p.w2 = w2, p.b2 = b2, p.w3 = w3, p.b3 = b3, p.w4 = w4, p.b4 = b4, p.out = output;
    p.std = std, p.eps = eps, p.action = action, p.logp = logp, p.std_out = std_out;
    p.rows = rows, p.K = int(in_features), p.A = int(out_features), p.alpha = alpha;
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t tiles = ceil_div(rows, kMlpRows);
    const int kb = int(ceil_div(in_features, 16));
    hipStream_t s = as_stream(stream);
    switch (activation) {
        case CUSRL_ACT_RELU: return launch_mlp3<CUSRL_ACT_RELU>(p, hidden1, hidden2, kb, tiles, cus, s);
        case CUSRL_ACT_ELU: return launch_mlp3<CUSRL_ACT_ELU>(p, hidden1, hidden2, kb, tiles, cus, s);
        default: return launch_mlp3<CUSRL_ACT_TANH>(p, hidden1, hidden2, kb, tiles, cus, s);
    }
}
