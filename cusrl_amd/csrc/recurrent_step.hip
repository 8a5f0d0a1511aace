// ONE no-grad time step of ONE GRU / LSTM layer for gfx950 as ONE launch: both projections on the matrix cores and the whole
// gate pass on the accumulator registers.  The acting step of a recurrent agent (rollout, Player, a deployed policy) is
// gru_forward / lstm_forward at L == 1 with nothing to differentiate: there the library chain is an addmm for gi, the recurrent
// mm for gh and the gate launch per layer, with gi / gh / the state slab written and read back for no backward that needs them.
//
//   GRU  (r, z, n):     r = s(W_ir x + b_ir + W_hr h + b_hr)   z likewise   n = tanh(W_in x + b_in + r (W_hn h + b_hn))
//                       h' = (1 - z) n + z h
//   LSTM (i, f, g, o):  pre = W_ih x + b_ih + W_hh h + b_hh    c' = s(f) c + s(i) tanh(g)    h' = s(o) tanh(c')
//
// Formulation: mlp_forward.hip's (transposed, features x rows, v_mfma_f32_16x16x4_f32; read its header first).  A 16-feature x
// 16-row output tile carries FOUR accumulators: for the LSTM i, f, g, o, each over both projections; for the GRU r and z over both
// projections and the n gate's two projections apart (gi_n over x, gh_n over h), since they meet only behind r.  A lane's register
// `reg` of every accumulator is the same (feature 16 tile + 4 kk + reg, row m), so the gate pass is in-lane arithmetic with the
// element expressions of gru.hip (recurrent_cell.hpp); h / c of the previous step are one 16-byte load per lane, h' / c' one
// 16-byte store.  No pre-activation reaches memory.
//
// Operands.  B: the rows' x and h quads, loaded ONCE per wave and kept in registers ((I + H) / 16 float4 per lane).  A: the
// weight rows of the gates (3 for the GRU, 4 for the LSTM), streamed from global memory (the matrices stay in L2) as one float4
// per lane, gate and k-block, requested one k-block ahead of the MFMAs that consume them — across the x / h boundary and across
// column tiles.  The gates' MFMAs of a k-block are interleaved (gate index innermost): consecutive instructions never wait on the
// same accumulator.
//
// Work split.  One wave per workgroup, grid = row tiles x column slices: a wave owns one 16-row tile and a contiguous slice of
// the H / 16 column tiles.  The slice count grows while there are fewer waves than 4 per CU (a 64-row step at H = 256 runs
// 4 x 16 waves), and is 1 when the row tiles alone fill the chip (a 16 384-row step reads its rows once).  No LDS, no barrier:
// nothing in the kernel waits for another wave.
//
// One sum order: x part (k = 0 .. I - 1, zero contributions at k >= I of the last k-block) then h part, whatever the slice count,
// the tile, the wave or B.  x and W_ih take the two read paths of quad_load.hpp — same values in the same registers.
//
// Register arrays are sized by the template (KXM / KHM k-blocks of x / h, 4 or 16 each); the k-block loops are unrolled to that
// size and guarded by the wave-uniform true counts, so a bucket costs registers, not work.
#include <atomic>
#include <initializer_list>

#include "mlp_tail.hpp"  // mfma_f32x4, pick, from_bias, kMlpRows
#include "quad_load.hpp"
#include "recurrent_cell.hpp"

namespace cusrl {

constexpr int kGruCell = 0, kLstmCell = 1;
constexpr int kStepWavesPerCu = 4;  // one per SIMD: the slice count stops growing there
constexpr int kStepMaxWidth = 256;  // of x and of h

struct RecurrentStepArgs {
    const float *x, *h, *c;  // c: LSTM only
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *h_out, *c_out;
    int64_t B, ld_h, ld_out;
    int I, H, slices;
    int wide;  // x and w_ih are read 16 bytes at a time
};

__device__ __forceinline__ float4 load4_or_zero(const float *p, int at) {
    return p ? *reinterpret_cast<const float4 *>(p + at) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int CELL, int KXM, int KHM>
__global__ __launch_bounds__(kWave) void recurrent_step_kernel(const RecurrentStepArgs p) {
    constexpr int G = CELL == kGruCell ? 3 : 4;  // weight row groups = A operands per k-block
    const int lane = threadIdx.x, i = lane & 15, kk = lane >> 4;
    const int I = p.I, H = p.H, KX = (I + 15) / 16, KH = H / 16;
    const bool wide = p.wide != 0;
    const int64_t tile = blockIdx.x / uint32_t(p.slices);
    const int slice = int(blockIdx.x - tile * p.slices);
    const int c0 = slice * KH / p.slices, c1 = (slice + 1) * KH / p.slices;  // this wave's column tiles (slices <= KH: never empty)
    const int64_t row0 = tile * kMlpRows;
    const int64_t row = min(row0 + i, p.B - 1);  // (rows past the end re-read the last row; nothing is stored for them)
    const bool live = row0 + i < p.B;
    const float *h_row = p.h + row * p.ld_h;

    // ---- the B operands, once
    float4 bx[KXM], bh[KHM];
#pragma unroll
    for (int t = 0; t < KXM; ++t)
        if (t < KX) bx[t] = quad_select(quad_load(p.x, row, I, 16 * t + 4 * kk, wide), I, 16 * t + 4 * kk);
#pragma unroll
    for (int t = 0; t < KHM; ++t)
        if (t < KH) bh[t] = *reinterpret_cast<const float4 *>(h_row + 16 * t + 4 * kk);

    // ---- the A operands of the next k-block (UNSELECTED for the x part: quad_select when they are used)
    float4 ahead[G];
    auto request_x = [&](int c, int t) {
#pragma unroll
        for (int g = 0; g < G; ++g) ahead[g] = quad_load(p.w_ih, g * H + 16 * c + i, I, 16 * t + 4 * kk, wide);
    };
    auto request_h = [&](int c, int t) {
#pragma unroll
        for (int g = 0; g < G; ++g)
            ahead[g] = *reinterpret_cast<const float4 *>(p.w_hh + int64_t(g * H + 16 * c + i) * H + 16 * t + 4 * kk);
    };
    request_x(c0, 0);

    for (int c = c0; c < c1; ++c) {
        const int f = 16 * c + 4 * kk;  // this lane's four features
        // the previous state and the recurrent bias of these features: requested here, used behind the MFMAs
        const float4 hp = *reinterpret_cast<const float4 *>(h_row + f);
        float4 cp = make_float4(0.f, 0.f, 0.f, 0.f), bias[4];
        if constexpr (CELL == kLstmCell) cp = *reinterpret_cast<const float4 *>(p.c + row * p.ld_h + f);
#pragma unroll
        for (int g = 0; g < G; ++g) bias[g] = load4_or_zero(p.b_hh, g * H + f);
        // accumulators: the input bias in front of the sum (GRU: r, z, gi_n, gh_n — gh_n's bias b_hn is added behind the sum)
        mfma_f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = g < G && p.b_ih ? from_bias(p.b_ih + g * H + f) : mfma_f32x4{0.f, 0.f, 0.f, 0.f};

        // ---- x part
#pragma unroll
        for (int t = 0; t < KXM; ++t) {
            if (t < KX) {
                float4 a[G];
#pragma unroll
                for (int g = 0; g < G; ++g) a[g] = quad_select(ahead[g], I, 16 * t + 4 * kk);
                if (t + 1 < KX) request_x(c, t + 1);
                else request_h(c, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < G; ++g)
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a[g], j), pick(bx[t], j), acc[g], 0, 0, 0);
            }
        }
        // ---- h part (GRU: the n rows of W_hh go to the fourth accumulator)
#pragma unroll
        for (int t = 0; t < KHM; ++t) {
            if (t < KH) {
                float4 a[G];
#pragma unroll
                for (int g = 0; g < G; ++g) a[g] = ahead[g];
                if (t + 1 < KH) request_h(c, t + 1);
                else request_x(min(c + 1, c1 - 1), 0);  // (the last tile re-reads its own first k-block; unused)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        constexpr int kToN = CELL == kGruCell ? 3 : 2;
                        const int to = g == 2 ? kToN : g;
                        acc[to] = __builtin_amdgcn_mfma_f32_16x16x4f32(pick(a[g], j), pick(bh[t], j), acc[to], 0, 0, 0);
                    }
            }
        }

        // ---- the gate pass, in-lane
        float hn[4], cn[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            if constexpr (CELL == kGruCell) {
                // (both projections of r and z are already summed: the recurrent halves gru_gates adds are zero)
                const GruGates g = gru_gates(acc[0][reg], acc[1][reg], acc[2][reg], 0.0f, 0.0f, acc[3][reg], pick(bias[0], reg),
                                             pick(bias[1], reg), pick(bias[2], reg));
                hn[reg] = gru_next(g, pick(hp, reg));
            } else {
                const LstmState s = lstm_next(acc[0][reg] + pick(bias[0], reg), acc[1][reg] + pick(bias[1], reg),
                                              acc[2][reg] + pick(bias[2], reg), acc[3][reg] + pick(bias[3], reg), pick(cp, reg));
                hn[reg] = s.h, cn[reg] = s.c;
            }
        }
        if (live) {
            *reinterpret_cast<float4 *>(p.h_out + (row0 + i) * p.ld_out + f) = make_float4(hn[0], hn[1], hn[2], hn[3]);
            if constexpr (CELL == kLstmCell)
                *reinterpret_cast<float4 *>(p.c_out + (row0 + i) * p.ld_out + f) = make_float4(cn[0], cn[1], cn[2], cn[3]);
        }
    }
}

template <int CELL>
static int launch_recurrent_step(const RecurrentStepArgs &p, dim3 grid, hipStream_t s) {
    const bool wide_x = p.I > 64, wide_h = p.H > 64;  // more than 4 k-blocks
    const dim3 block(kWave);
    if (wide_x && wide_h) hipLaunchKernelGGL((recurrent_step_kernel<CELL, 16, 16>), grid, block, 0, s, p);
    else if (wide_x) hipLaunchKernelGGL((recurrent_step_kernel<CELL, 16, 4>), grid, block, 0, s, p);
    else if (wide_h) hipLaunchKernelGGL((recurrent_step_kernel<CELL, 4, 16>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((recurrent_step_kernel<CELL, 4, 4>), grid, block, 0, s, p);
    return launch_status();
}

// CUs of the current device, asked once per device (the current device may differ between calls)
static int compute_units() {
    constexpr int kDevices = 64;
    static std::atomic<int> cached[kDevices];
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return 256;
    const bool slot = device >= 0 && device < kDevices;
    int cus = slot ? cached[device].load(std::memory_order_relaxed) : 0;
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) return 256;
        if (slot) cached[device].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// [B, width] floats with row stride ld
struct Rows {
    const float *at;
    int64_t B, ld, width;
    const float *end() const { return at + (B - 1) * ld + width; }
};

// May the two share a float?  Apart when their address ranges are; two column slices of one row stride (layer slices of the same
// memory matrix) are also apart when their columns are.  Anything else that interleaves counts as overlapping.
static bool overlap(const Rows &a, const Rows &b) {
    if (!a.at || !b.at) return false;
    if (a.end() <= b.at || b.end() <= a.at) return false;
    if (a.ld != b.ld) return true;
    const int64_t d = ((b.at - a.at) % a.ld + a.ld) % a.ld;  // column of b's first float, counted from a's
    return !(d >= a.width && d + b.width <= a.ld);
}

// The ONE statement of what the step kernel takes (c / c_out: NULL for the GRU).
static bool step_supported(bool lstm, const float *x, int64_t B, int64_t I, const float *h, const float *c, int64_t ld_h,
                           const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int64_t H,
                           const float *h_out, const float *c_out, int64_t ld_out) {
    if (B < 1 || I < 1 || I > kStepMaxWidth || H < 16 || H > kStepMaxWidth || H % 16 != 0) return false;
    if ((b_ih == nullptr) != (b_hh == nullptr)) return false;
    if (ld_h < H || ld_h % 4 != 0 || ld_out < H || ld_out % 4 != 0) return false;
    // (x and w_ih may sit at any float address: their alignment picks the read path)
    for (const void *ptr : {(const void *)h, (const void *)c, (const void *)w_hh, (const void *)b_ih, (const void *)b_hh,
                            (const void *)h_out, (const void *)c_out})
        if (!aligned(ptr, 16)) return false;
    if (ceil_div(B, kMlpRows) > INT32_MAX / (kStepMaxWidth / 16)) return false;  // row tiles x slices is the grid
    const Rows in[3] = {{x, B, I, I}, {h, B, ld_h, H}, {c, B, ld_h, H}}, out[2] = {{h_out, B, ld_out, H}, {c_out, B, ld_out, H}};
    for (const Rows &o : out)
        for (const Rows &r : in)
            if (overlap(o, r)) return false;  // another slice's wave may still be reading those rows
    return !(lstm && overlap(out[0], out[1]));
}

static int step_forward(bool lstm, const float *x, int64_t B, int64_t I, const float *h, const float *c, int64_t ld_h,
                        const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int64_t H, float *h_out,
                        float *c_out, int64_t ld_out, void *stream) {
    if (B < 0 || !x || !h || !w_ih || !w_hh || !h_out || (lstm && (!c || !c_out))) return CUSRL_E_INVALID;
    if (B == 0) return 0;
    if (!step_supported(lstm, x, B, I, h, c, ld_h, w_ih, w_hh, b_ih, b_hh, H, h_out, c_out, ld_out)) return CUSRL_E_UNSUPPORTED;
    RecurrentStepArgs p;
    p.x = x, p.h = h, p.c = c, p.w_ih = w_ih, p.w_hh = w_hh, p.b_ih = b_ih, p.b_hh = b_hh, p.h_out = h_out, p.c_out = c_out;
    p.B = B, p.ld_h = ld_h, p.ld_out = ld_out, p.I = int(I), p.H = int(H);
    p.wide = I % 4 == 0 && aligned(x, 16) && aligned(w_ih, 16);
    // slices: as many as it takes to reach kStepWavesPerCu waves per CU, at most one per column tile
    const int64_t tiles = ceil_div(B, kMlpRows), wanted = ceil_div(int64_t(kStepWavesPerCu) * compute_units(), tiles);
    p.slices = int(wanted < H / 16 ? wanted : H / 16);
    const dim3 grid(uint32_t(tiles * p.slices));
    return lstm ? launch_recurrent_step<kLstmCell>(p, grid, as_stream(stream)) : launch_recurrent_step<kGruCell>(p, grid, as_stream(stream));
}

}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_gru_step_forward_supported(const float *x, int64_t B, int64_t I, const float *h, int64_t ld_h, const float *w_ih,
                                                const float *w_hh, const float *b_ih, const float *b_hh, int64_t H,
                                                const float *h_out, int64_t ld_out) {
    return x && h && w_ih && w_hh && h_out && step_supported(false, x, B, I, h, nullptr, ld_h, w_ih, w_hh, b_ih, b_hh, H, h_out, nullptr, ld_out);
}

extern "C" int cusrl_gru_step_forward(const float *x, int64_t B, int64_t I, const float *h, int64_t ld_h, const float *w_ih,
                                      const float *w_hh, const float *b_ih, const float *b_hh, int64_t H, float *h_out,
                                      int64_t ld_out, void *stream) {
    return step_forward(false, x, B, I, h, nullptr, ld_h, w_ih, w_hh, b_ih, b_hh, H, h_out, nullptr, ld_out, stream);
}

extern "C" int cusrl_lstm_step_forward_supported(const float *x, int64_t B, int64_t I, const float *h, const float *c, int64_t ld_h,
                                                 const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh,
                                                 int64_t H, const float *h_out, const float *c_out, int64_t ld_out) {
    return x && h && c && w_ih && w_hh && h_out && c_out &&
           step_supported(true, x, B, I, h, c, ld_h, w_ih, w_hh, b_ih, b_hh, H, h_out, c_out, ld_out);
}

extern "C" int cusrl_lstm_step_forward(const float *x, int64_t B, int64_t I, const float *h, const float *c, int64_t ld_h,
                                       const float *w_ih, const float *w_hh, const float *b_ih, const float *b_hh, int64_t H,
                                       float *h_out, float *c_out, int64_t ld_out, void *stream) {
    return step_forward(true, x, B, I, h, c, ld_h, w_ih, w_hh, b_ih, b_hh, H, h_out, c_out, ld_out, stream);
}
