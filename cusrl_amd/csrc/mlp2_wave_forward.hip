// Inference pass of a SMALL two-hidden-layer actor / critic MLP for gfx950: out = W3 act(W2 act(W1 x + b1) + b2) + b3 with
// hidden widths in {32, 64}, act one of ReLU / ELU / Tanh and ANY input width 1 <= K <= 64 — the (64, 64) Tanh networks of the
// classic-control experiments over 2- to 6-wide observations — as ONE launch, optionally with the acting path's sampling epilogue
// (mlp_tail.hpp) behind it.
//
// Formulation: mlp_forward.hip's (transposed, features x rows, v_mfma_f32_16x16x4_f32; read its header first).  A lane's float4
// of a weight row is the A operand of four consecutive MFMAs of a k-block; the four accumulator registers a lane holds of an
// output tile are the B operands of the next layer's k-block of the same index.
//
// Wave-resident.  The whole (64, 64) stack is 8.3 K weights at K = 64: <= 64 + 64 + 16 registers per lane for W1 / W2 / W3 and
// 36 for the biases.  So ONE wave holds all three matrices and carries a 16-row tile from the input to the head: every tile of
// layer 1 it needs as a k-block of layer 2 is already in its own accumulators, and the head's sum over layer 2's tiles is
// complete inside the wave.  No __shared__ memory, no barrier, nothing between the layers but the activation on the
// accumulator registers.  The 2 or 4 independent output tiles of a layer are interleaved (tile index innermost), so consecutive
// MFMAs never wait on each other's accumulators; only the head (one tile) is a dependent chain, of at most 16 MFMAs.
//
// Work split.  kGroupWaves = 1 wave per workgroup, grid = min(tiles, 4 x CUs): the 256 tiles of a 4096-row act step reach every
// CU (four-wave workgroups would put them on 64), and up to four waves share a CU, one per SIMD.  Beyond that a wave walks tiles
// with stride (waves in the grid), weights in place, the next tile's input rows requested one tile ahead.
//
// Two read paths for x and W1, chosen per launch (wave-uniform): `wide` (K % 4 == 0, both 16-byte aligned) reads a lane's four
// k values as one clamped 16-byte load, as the existing kernels do; otherwise they are four 4-byte loads from clamped
// addresses, since the rows of a [B, 3] matrix are not 16-byte aligned.  Both leave the same values in the same registers:
// k = 16 t + 4 kk + j for j = 0..3, zero at k >= K (in A and in B), then one MFMA sequence in one k order.  A row's bits depend
// on neither the path nor the tile, the wave or the row count.
//
// Activations with the expressions of cusrl_bias_act (act4, mlp_tail.hpp); fp32 MFMA accumulation as in the library's GEMMs.
#include "mlp_tail.hpp"
#include "quad_load.hpp"  // quad_load / quad_select: the two read paths

// waves per workgroup (independent of each other; a build with 4 is the alternative DESIGN.md §7 names as not yet timed)
#ifndef CUSRL_MLP2_WAVE_GROUP
#define CUSRL_MLP2_WAVE_GROUP 1
#endif

namespace cusrl {

constexpr int kGroupWaves = CUSRL_MLP2_WAVE_GROUP;
constexpr int kWavesPerCu = 4;  // one per SIMD

struct Mlp2WaveArgs {
    const float *x;
    const float *w1, *b1, *w2, *b2, *w3, *b3;
    float *out;        // [rows, A] (NULL: not stored)
    const float *std;  // sampling epilogue (all NULL: none): [A] vector
    const float *eps;  // [rows, A]
    float *action, *logp, *std_out;
    int64_t rows;
    int K, A;
    float alpha;
    int wide;  // x and w1 are read 16 bytes at a time
};

// NT1 / NT2: 16-feature tiles of the first / second hidden layer (H = 16 NT); KB: 16-wide k-blocks of the input (K <= 16 KB).
template <int ACT, int NT1, int NT2, int KB>
__global__ __launch_bounds__(kGroupWaves *kWave) void mlp2_wave_forward_kernel(const Mlp2WaveArgs p) {
    constexpr int H1 = 16 * NT1, H2 = 16 * NT2;
    const int lane = threadIdx.x & (kWave - 1);
    const int i = lane & 15, kk = lane >> 4;
    const int K = p.K, A = p.A;
    const bool wide = p.wide != 0;
    const float alpha = p.alpha;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int64_t tiles = (p.rows + kMlpRows - 1) / kMlpRows;
    const int64_t first = int64_t(blockIdx.x) * kGroupWaves + threadIdx.x / kWave, stride = int64_t(gridDim.x) * kGroupWaves;
    if (first >= tiles) return;  // (only a four-wave group's last waves; nothing in this kernel waits for another wave)

    // the input rows of a tile are requested one tile ahead: with one wave per SIMD nothing else hides the load's latency
    float4 ahead[KB];
    auto request = [&](int64_t tile) {
        const int64_t row = min(tile * kMlpRows + i, p.rows - 1);  // (rows past the end re-read the last row; nothing is stored for them)
#pragma unroll
        for (int t = 0; t < KB; ++t) ahead[t] = quad_load(p.x, row, K, 16 * t + 4 * kk, wide);
    };
    request(first);

    // ---- all three weight matrices and the biases, once
    float4 a1[NT1][KB], a2[NT2][NT1], a3[NT2];
    mfma_f32x4 c1[NT1], c2[NT2], c3;
#pragma unroll
    for (int t1 = 0; t1 < NT1; ++t1) {
#pragma unroll
        for (int t = 0; t < KB; ++t) {
            const int k = 16 * t + 4 * kk;
            a1[t1][t] = quad_select(quad_load(p.w1, 16 * t1 + i, K, k, wide), K, k);
        }
        c1[t1] = from_bias(p.b1 + 16 * t1 + 4 * kk);
    }
#pragma unroll
    for (int t2 = 0; t2 < NT2; ++t2) {
        const int n = 16 * t2;
#pragma unroll
        for (int t = 0; t < NT1; ++t) a2[t2][t] = *reinterpret_cast<const float4 *>(p.w2 + int64_t(n + i) * H1 + 16 * t + 4 * kk);
        c2[t2] = from_bias(p.b2 + n + 4 * kk);
        // the head: rows = outputs (i < A), k-block = tile t2 of the second hidden layer
        const float4 v = *reinterpret_cast<const float4 *>(p.w3 + int64_t(i < A ? i : 0) * H2 + n + 4 * kk);
        a3[t2] = i < A ? v : zero4;
    }
    c3 = mfma_f32x4{0.f, 0.f, 0.f, 0.f};
    if (p.b3) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) c3[reg] = 4 * kk + reg < A ? p.b3[4 * kk + reg] : 0.f;
    }

    // sampling epilogue: this lane's four std values once, its four eps values requested at the top of every tile
    float sigma[4] = {1.f, 1.f, 1.f, 1.f}, noise[4] = {0.f, 0.f, 0.f, 0.f};
    const bool sampling = p.eps != nullptr;
    if (sampling) mlp_tail_sigma(p.std, A, kk, sigma);

    for (int64_t tile = first; tile < tiles; tile += stride) {
        const int64_t row0 = tile * kMlpRows;
        if (sampling) mlp_tail_noise(p.eps, p.rows, A, row0, lane, noise);
        float4 xb[KB];
#pragma unroll
        for (int t = 0; t < KB; ++t) xb[t] = quad_select(ahead[t], K, 16 * t + 4 * kk);
        request(min(tile + stride, tiles - 1));
        // ---- layer 1: all NT1 tiles of H1^T, bias in the accumulator, tiles interleaved
        mfma_f32x4 h1[NT1];
#pragma unroll
        for (int t1 = 0; t1 < NT1; ++t1) h1[t1] = c1[t1];
#pragma unroll
        for (int t = 0; t < KB; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t1 = 0; t1 < NT1; ++t1)
                    h1[t1] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a1[t1][t], j), pick(xb[t], j), h1[t1], 0, 0, 0);
#pragma unroll
        for (int t1 = 0; t1 < NT1; ++t1) h1[t1] = act4<ACT>(h1[t1], alpha);
        // ---- layer 2: tile t of layer 1 is k-block t, its registers the B operands as they are
        mfma_f32x4 h2[NT2];
#pragma unroll
        for (int t2 = 0; t2 < NT2; ++t2) h2[t2] = c2[t2];
#pragma unroll
        for (int t = 0; t < NT1; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int t2 = 0; t2 < NT2; ++t2)
                    h2[t2] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a2[t2][t], j), h1[t][j], h2[t2], 0, 0, 0);
        // ---- head: the whole contraction over layer 2's tiles, in this wave
        mfma_f32x4 head = c3;
#pragma unroll
        for (int t2 = 0; t2 < NT2; ++t2) {
            const mfma_f32x4 h = act4<ACT>(h2[t2], alpha);
#pragma unroll
            for (int j = 0; j < 4; ++j) head = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a3[t2], j), h[j], head, 0, 0, 0);
        }
        mlp_tail_body(p, make_float4(head[0], head[1], head[2], head[3]), row0, lane, sigma, noise);
    }
}

template <int ACT, int NT1, int NT2>
static int launch_mlp2_wave_kb(const Mlp2WaveArgs &p, int kb, dim3 grid, hipStream_t s) {
    const dim3 block(kGroupWaves * kWave);
    switch (kb) {
        case 1: hipLaunchKernelGGL((mlp2_wave_forward_kernel<ACT, NT1, NT2, 1>), grid, block, 0, s, p); break;
        case 2: hipLaunchKernelGGL((mlp2_wave_forward_kernel<ACT, NT1, NT2, 2>), grid, block, 0, s, p); break;
        case 3: hipLaunchKernelGGL((mlp2_wave_forward_kernel<ACT, NT1, NT2, 3>), grid, block, 0, s, p); break;
        case 4: hipLaunchKernelGGL((mlp2_wave_forward_kernel<ACT, NT1, NT2, 4>), grid, block, 0, s, p); break;
        default: return CUSRL_E_UNSUPPORTED;
    }
    return launch_status();
}

template <int ACT>
static int launch_mlp2_wave(const Mlp2WaveArgs &p, int64_t h1, int64_t h2, int kb, dim3 grid, hipStream_t s) {
    if (h1 == 64 && h2 == 64) return launch_mlp2_wave_kb<ACT, 4, 4>(p, kb, grid, s);
    if (h1 == 64) return launch_mlp2_wave_kb<ACT, 4, 2>(p, kb, grid, s);
    if (h2 == 64) return launch_mlp2_wave_kb<ACT, 2, 4>(p, kb, grid, s);
    return launch_mlp2_wave_kb<ACT, 2, 2>(p, kb, grid, s);
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_mlp2_wave_forward_supported(int64_t in_features, int64_t hidden1, int64_t hidden2, int64_t out_features) {
    return in_features >= 1 && in_features <= 64 && (hidden1 == 32 || hidden1 == 64) && (hidden2 == 32 || hidden2 == 64) &&
           out_features >= 1 && out_features <= 16;
}

extern "C" int cusrl_mlp2_wave_forward(const float *input, int64_t rows, int64_t in_features, const float *w1, const float *b1,
                                       int64_t hidden1, const float *w2, const float *b2, int64_t hidden2, const float *w3,
                                       const float *b3, int64_t out_features, int activation, float alpha, float *output,
                                       const float *std, const float *eps, float *action, float *logp, float *std_out, void *stream) {
    if (rows < 0 || !input || !w1 || !b1 || !w2 || !b2 || !w3) return CUSRL_E_INVALID;
    if (rows == 0) return 0;
    if (!cusrl_mlp2_wave_forward_supported(in_features, hidden1, hidden2, out_features)) return CUSRL_E_UNSUPPORTED;
    if (activation != CUSRL_ACT_RELU && activation != CUSRL_ACT_ELU && activation != CUSRL_ACT_TANH) return CUSRL_E_UNSUPPORTED;
    const bool sampling = eps != nullptr;
    if (sampling ? !(std && action && logp) : (std || action || logp || std_out)) return CUSRL_E_INVALID;
    if (!sampling && !output) return CUSRL_E_INVALID;
    // (input and w1 may sit at any float address: their alignment picks the read path)
    if (!aligned(b1, 16) || !aligned(w2, 16) || !aligned(b2, 16) || !aligned(w3, 16) ||
        (output && out_features % 4 == 0 && !aligned(output, 16)))
        return CUSRL_E_UNSUPPORTED;
    Mlp2WaveArgs p;
    p.x = input, p.w1 = w1, p.b1 = b1, p.w2 = w2, p.b2 = b2, p.w3 = w3, p.b3 = b3, p.out = output;
    p.std = std, p.eps = eps, p.action = action, p.logp = logp, p.std_out = std_out;
    p.rows = rows, p.K = int(in_features), p.A = int(out_features), p.alpha = alpha;
    p.wide = in_features % 4 == 0 && aligned(input, 16) && aligned(w1, 16);
    // (asked on every call: the current device may differ between calls, and the attribute is a cached property)
    int device = 0, cus = 0;
    if (hipGetDevice(&device) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    const int64_t tiles = ceil_div(rows, kMlpRows), waves = tiles < int64_t(kWavesPerCu) * cus ? tiles : int64_t(kWavesPerCu) * cus;
    const dim3 grid(uint32_t(ceil_div(waves, kGroupWaves)));
    const int kb = int(ceil_div(in_features, 16));
    hipStream_t s = as_stream(stream);
    switch (activation) {
        case CUSRL_ACT_RELU: return launch_mlp2_wave<CUSRL_ACT_RELU>(p, hidden1, hidden2, kb, grid, s);
        case CUSRL_ACT_ELU: return launch_mlp2_wave<CUSRL_ACT_ELU>(p, hidden1, hidden2, kb, grid, s);
        default: return launch_mlp2_wave<CUSRL_ACT_TANH>(p, hidden1, hidden2, kb, grid, s);
    }
}
