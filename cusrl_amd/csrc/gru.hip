// GRU / LSTM / RNN time-step epilogues for gfx950 (recurrent BPTT, config 4).
//
// torch.nn.GRU on ROCm is MIOpen's RNN: per time step it issues generic tensor kernels (Op2dTensorLite,
// SubTensorOpWithSubTensor2d: ~24 000 launches per iteration of config 4) and reduces the bias gradients with
// Op2dTensorSquash at 7.6 ms a call — 45 % of the device time of that config (profiles/r02/config4_miopen_kernel_stats.csv).
// Here the layer is what it is algebraically: ONE input-projection GEMM for all time steps, per step one recurrent GEMM
// (rocBLAS, [B, H] x [H, 3H]) and ONE pass over the gates; backward mirrors it, and the weight / bias gradients are
// batched GEMMs / column sums over all steps at once.  These kernels are that one pass:
//
//   r = sigmoid(gi_r + gh_r + b_hr)      z = sigmoid(gi_z + gh_z + b_hz)
//   q = gh_n + b_hn                      n = tanh(gi_n + r * q)
//   h' = (1 - z) * n + z * h             (torch.nn.GRU; gi = W_ih x + b_ih, gh = W_hh h)
//
// `lengths` (optional) gives packed-sequence semantics without packing: a sequence that has ended (t >= lengths[b]) keeps
// its state, emits zeros, and lets the state gradient pass through untouched — so the final state is the state at each
// sequence's own last step (cusrl/nn/module/rnn.py:273-291 obtains that through a PackedSequence and a host read of the
// lengths).  Streaming, HBM-bound: 36 B per state element forward, 64 B backward; 16-byte lanes when H % 4 == 0.
//
// Layout of the file: `Lanes<V>` (the floats of one access) and `element` (which ones a thread owns) are what every kernel
// body is written over; `gru_bwd_row` is the GRU backward of one (row, column chunk), shared by the plain pass and the one
// that folds the bias sums; `gate_pass` is the host sequence of all seven launch entry points.
#include <initializer_list>
#include <type_traits>

#include "common.hpp"

namespace cusrl {

// The kW floats a thread handles at a time: V = float4 (H % 4 == 0, aligned rows — ONE 16-byte access) or float.  The value
// is kept as the V it was loaded as; the only view of a V as floats is in here.
template <typename V>
struct Lanes {
    static constexpr int kW = sizeof(V) / sizeof(float);
    V raw;

    __device__ __forceinline__ float &operator[](int k) { return reinterpret_cast<float *>(&raw)[k]; }
    __device__ __forceinline__ float operator[](int k) const { return reinterpret_cast<const float *>(&raw)[k]; }

    static __device__ __forceinline__ Lanes zero() {
        Lanes lanes;
#pragma unroll
        for (int k = 0; k < kW; ++k) lanes[k] = 0.0f;
        return lanes;
    }
    static __device__ __forceinline__ Lanes load(const float *p) {
        Lanes lanes;
        lanes.raw = *reinterpret_cast<const V *>(p);
        return lanes;
    }
    // an optional operand (b_hh, d_out): zeros when it is absent
    static __device__ __forceinline__ Lanes load_or_zero(const float *p, int64_t offset) {
        return p ? load(p + offset) : zero();
    }
    __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<V *>(p) = raw; }
};

// What a thread of an element-per-thread pass owns: columns [j, j + kW) of row b — or nothing, in the tail of the last block.
struct Element {
    int64_t b;
    int j;
    bool none;
};

template <typename V>
__device__ __forceinline__ Element element(int64_t B, int H) {
    constexpr int kW = Lanes<V>::kW;
    const int cols = H / kW;
    const int64_t e = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= B * cols) return {0, 0, true};
    const int64_t b = e / cols;
    return {b, int(e - b * cols) * kW, false};
}

// false: the sequence of row b has ended before step t
__device__ __forceinline__ bool row_live(const int64_t *__restrict__ lengths, int64_t t, int64_t b) {
    return !lengths || t < lengths[b];
}

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct GruGates {
    float r, z, q, n;
};

__device__ __forceinline__ GruGates gru_gates(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n,
                                              float b_r, float b_z, float b_n) {
    GruGates g;
    g.r = gru_sigmoid(gi_r + gh_r + b_r);
    g.z = gru_sigmoid(gi_z + gh_z + b_z);
    g.q = gh_n + b_n;
    g.n = tanhf(gi_n + g.r * g.q);
    return g;
}

// b_hh = {b_hr, b_hz, b_hn} at columns [j, j + kW); zeros without a bias
template <typename V>
struct GruBias {
    Lanes<V> r, z, n;
    __device__ __forceinline__ GruBias(const float *__restrict__ b_hh, int H, int j) {
        if (b_hh)
            r = Lanes<V>::load(b_hh + j), z = Lanes<V>::load(b_hh + H + j), n = Lanes<V>::load(b_hh + 2 * H + j);
        else
            r = z = n = Lanes<V>::zero();
    }
};

template <typename V>
__global__ __launch_bounds__(kBlock) void gru_gates_fwd_kernel(const float *__restrict__ gi, const float *__restrict__ gh,
                                                               const float *__restrict__ b_hh, float *__restrict__ h,
                                                               float *__restrict__ out,
                                                               const int64_t *__restrict__ lengths, int64_t t,
                                                               int64_t B, int H) {
    using L = Lanes<V>;
    const Element at = element<V>(B, H);
    if (at.none) return;
    const int64_t b = at.b;
    const int j = at.j;
    const float *gi_row = gi + b * 3 * H, *gh_row = gh + b * 3 * H;
    const L gir = L::load(gi_row + j), giz = L::load(gi_row + H + j), gin = L::load(gi_row + 2 * H + j);
    const L ghr = L::load(gh_row + j), ghz = L::load(gh_row + H + j), ghn = L::load(gh_row + 2 * H + j);
    const L hp = L::load(h + b * H + j);
    const GruBias<V> bias(b_hh, H, j);
    const bool live = row_live(lengths, t, b);
    L hn, o;
#pragma unroll
    for (int k = 0; k < L::kW; ++k) {
        const GruGates g = gru_gates(gir[k], giz[k], gin[k], ghr[k], ghz[k], ghn[k], bias.r[k], bias.z[k], bias.n[k]);
        const float next = (1.0f - g.z) * g.n + g.z * hp[k];
        hn[k] = live ? next : hp[k];
        o[k] = live ? next : 0.0f;
    }
    hn.store(h + b * H + j);
    o.store(out + b * H + j);
}

// What gru_bwd_row wrote for its row: gi = {d_r, d_z, d_n}, gh = {d_r, d_z, d_q} (zeros for an ended sequence).
template <typename V>
struct GruRowGrads {
    Lanes<V> r, z, n, q;
    bool live;
};

// The GRU backward of columns [j, j + kW) of row b, in place: gi <- d(loss)/d(gi), gh <- d(loss)/d(gh) (the saved
// pre-activations are consumed), dh <- dh_t * z (the direct path to h_{t-1}; the caller adds d_gh @ W_hh).  dh on entry =
// gradient arriving from step t + 1.  An ended sequence has no gate gradients and its state gradient passes through (dh
// stays as it is); none of its per-row operands is read, and `bias_of_row()` -> GruBias<V> is asked for a live row only.
template <typename V, typename Bias>
__device__ __forceinline__ GruRowGrads<V> gru_bwd_row(float *__restrict__ gi, float *__restrict__ gh, Bias bias_of_row,
                                                      const float *__restrict__ h_prev, const float *__restrict__ d_out,
                                                      float *__restrict__ dh, const int64_t *__restrict__ lengths,
                                                      int64_t t, int64_t b, int j, int H) {
    using L = Lanes<V>;
    float *gi_row = gi + b * 3 * H, *gh_row = gh + b * 3 * H;
    GruRowGrads<V> d;
    d.live = row_live(lengths, t, b);
    if (!d.live) {
        d.r = d.z = d.n = d.q = L::zero();
    } else {
        const L gir = L::load(gi_row + j), giz = L::load(gi_row + H + j), gin = L::load(gi_row + 2 * H + j);
        const L ghr = L::load(gh_row + j), ghz = L::load(gh_row + H + j), ghn = L::load(gh_row + 2 * H + j);
        const L hp = L::load(h_prev + b * H + j);
        const L dhn = L::load(dh + b * H + j);
        const L dout = L::load_or_zero(d_out, b * H + j);
        const GruBias<V> bias = bias_of_row();
        L d_h;
#pragma unroll
        for (int k = 0; k < L::kW; ++k) {
            const GruGates g = gru_gates(gir[k], giz[k], gin[k], ghr[k], ghz[k], ghn[k], bias.r[k], bias.z[k], bias.n[k]);
            const float dht = dhn[k] + dout[k];
            const float dn_pre = dht * (1.0f - g.z) * (1.0f - g.n * g.n);
            d.n[k] = dn_pre;
            d.q[k] = dn_pre * g.r;
            d.r[k] = dn_pre * g.q * g.r * (1.0f - g.r);
            d.z[k] = dht * (hp[k] - g.n) * g.z * (1.0f - g.z);
            d_h[k] = dht * g.z;
        }
        d_h.store(dh + b * H + j);
    }
    d.r.store(gi_row + j);
    d.z.store(gi_row + H + j);
    d.n.store(gi_row + 2 * H + j);
    d.r.store(gh_row + j);
    d.z.store(gh_row + H + j);
    d.q.store(gh_row + 2 * H + j);
    return d;
}

template <typename V>
__global__ __launch_bounds__(kBlock) void gru_gates_bwd_kernel(float *__restrict__ gi, float *__restrict__ gh,
                                                               const float *__restrict__ b_hh,
                                                               const float *__restrict__ h_prev,
                                                               const float *__restrict__ d_out, float *__restrict__ dh,
                                                               const int64_t *__restrict__ lengths, int64_t t,
                                                               int64_t B, int H) {
    const Element at = element<V>(B, H);
    if (at.none) return;
    gru_bwd_row<V>(gi, gh, [&] { return GruBias<V>(b_hh, H, at.j); }, h_prev, d_out, dh, lengths, t, at.b, at.j, H);
}

// The same pass with the bias gradients folded in: a block owns kBiasRows consecutive rows, every thread keeps one column
// chunk (kBlock % cols == 0) and sums what it writes — d_r, d_z, d_n, d_q — over its rows; the block's row groups are
// folded through LDS and the block leaves ONE partial row [4H] = {sum d_r, sum d_z, sum d_n, sum d_q}.  The caller sums the
// L x ceil(B / kBiasRows) partial rows once per layer: d b_ih = {r, z, n}, d b_hh = {r, z, q}.  Replaces two column-sum
// passes over the [L * B, 3H] gradient arrays (config 4: 2 x 408 MB read again per layer at the HBM roofline, 14 ms per
// iteration) by 2 x 17 MB of partial rows.  Fixed summation order (deterministic).
constexpr int kBiasRowsDefault = 16;
static int bias_rows() {
    const int r = int(option(kOptGruBiasRows));  // cusrl_set_option("gru_bias_rows", 4 | 8 | 16 | 32)
    return (r == 4 || r == 8 || r == 16 || r == 32) ? r : kBiasRowsDefault;
}

template <typename V>
__global__ __launch_bounds__(kBlock) void gru_gates_bwd_bias_kernel(float *__restrict__ gi, float *__restrict__ gh,
                                                                    const float *__restrict__ b_hh,
                                                                    const float *__restrict__ h_prev,
                                                                    const float *__restrict__ d_out, float *__restrict__ dh,
                                                                    const int64_t *__restrict__ lengths, int64_t t,
                                                                    int64_t B, int H, float *__restrict__ bias_partials,
                                                                    int kBiasRows) {
    constexpr int kW = Lanes<V>::kW;
    const int cols = H / kW;              // divides kBlock (checked by the entry point)
    const int groups = kBlock / cols;     // rows in flight per pass of the block
    const int col = threadIdx.x % cols, group = threadIdx.x / cols;
    const int j = col * kW;
    const int64_t row0 = int64_t(blockIdx.x) * kBiasRows;
    float acc[4][kW];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int k = 0; k < kW; ++k) acc[g][k] = 0.0f;
    const GruBias<V> bias(b_hh, H, j);  // once for all rows of the thread
    for (int r = group; r < kBiasRows; r += groups) {
        const int64_t b = row0 + r;
        if (b >= B) break;
        const GruRowGrads<V> d = gru_bwd_row<V>(gi, gh, [&] { return bias; }, h_prev, d_out, dh, lengths, t, b, j, H);
        if (d.live) {  // (an ended row adds nothing)
#pragma unroll
            for (int k = 0; k < kW; ++k) acc[0][k] += d.r[k], acc[1][k] += d.z[k], acc[2][k] += d.n[k], acc[3][k] += d.q[k];
        }
    }
    // fold the block's row groups (same column chunk: threads col, col + cols, ...), group 0 first
    __shared__ float fold[kBlock][4 * kW];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int k = 0; k < kW; ++k) fold[threadIdx.x][g * kW + k] = acc[g][k];
    __syncthreads();
    if (group == 0) {
        float *out = bias_partials + int64_t(blockIdx.x) * 4 * H;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float total[kW];
#pragma unroll
            for (int k = 0; k < kW; ++k) total[k] = 0.0f;
            for (int q = 0; q < groups; ++q)
#pragma unroll
                for (int k = 0; k < kW; ++k) total[k] += fold[q * cols + col][g * kW + k];
#pragma unroll
            for (int k = 0; k < kW; ++k) out[g * H + j + k] = total[k];
        }
    }
}


// ---- LSTM (the default core of RecurrentPpoAgentFactory, cusrl/preset/ppo.py:189) --------------------------------------
//   pre = gi + gh + b_hh   (gi = W_ih x + b_ih, gh = W_hh h; gate order i, f, g, o as torch.nn.LSTM)
//   i, f, o = sigmoid(pre_i, pre_f, pre_o);  g = tanh(pre_g);  c' = f * c + i * g;  h' = o * tanh(c')
// Both biases are additive, so d(pre) is the gradient of gi AND of gh: the forward stores `pre` over gi (kSave) and the
// backward overwrites it with d(pre) — one [B, 4H] array per step is all the layer keeps besides the cell states.
template <typename V, bool kSave>
__global__ __launch_bounds__(kBlock) void lstm_gates_fwd_kernel(float *__restrict__ gi, const float *__restrict__ gh,
                                                                const float *__restrict__ b_hh, float *__restrict__ h,
                                                                float *__restrict__ c, float *__restrict__ out,
                                                                float *__restrict__ c_saved,
                                                                const int64_t *__restrict__ lengths, int64_t t,
                                                                int64_t B, int H) {
    using L = Lanes<V>;
    const Element at = element<V>(B, H);
    if (at.none) return;
    const int64_t b = at.b;
    const int j = at.j;
    float *gi_row = gi + b * 4 * H;
    const float *gh_row = gh + b * 4 * H;
    L pre[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const L a = L::load(gi_row + g * H + j), r = L::load(gh_row + g * H + j), bias = L::load_or_zero(b_hh, g * H + j);
#pragma unroll
        for (int k = 0; k < L::kW; ++k) pre[g][k] = a[k] + r[k] + bias[k];
    }
    const L hp = L::load(h + b * H + j), cp = L::load(c + b * H + j);
    const bool live = row_live(lengths, t, b);
    L hn, cn, o;
#pragma unroll
    for (int k = 0; k < L::kW; ++k) {
        const float c_next = gru_sigmoid(pre[1][k]) * cp[k] + gru_sigmoid(pre[0][k]) * tanhf(pre[2][k]);
        const float h_next = gru_sigmoid(pre[3][k]) * tanhf(c_next);
        cn[k] = live ? c_next : cp[k];
        hn[k] = live ? h_next : hp[k];
        o[k] = live ? h_next : 0.0f;
    }
    hn.store(h + b * H + j);
    cn.store(c + b * H + j);
    o.store(out + b * H + j);
    if constexpr (kSave) {
        cn.store(c_saved + b * H + j);
#pragma unroll
        for (int g = 0; g < 4; ++g) pre[g].store(gi_row + g * H + j);
    }
}

// pre <- d(loss)/d(pre) in place; dc <- gradient of c_{t-1}; dh <- the part of the state gradient that bypasses this step
// (all of it for an ended sequence, nothing otherwise): the caller then adds d(pre) @ W_hh.
template <typename V>
__global__ __launch_bounds__(kBlock) void lstm_gates_bwd_kernel(float *__restrict__ pre, const float *__restrict__ c_prev,
                                                                const float *__restrict__ c_next,
                                                                const float *__restrict__ d_out, float *__restrict__ dh,
                                                                float *__restrict__ dc,
                                                                const int64_t *__restrict__ lengths, int64_t t,
                                                                int64_t B, int H) {
    using L = Lanes<V>;
    const Element at = element<V>(B, H);
    if (at.none) return;
    const int64_t b = at.b;
    const int j = at.j;
    float *row = pre + b * 4 * H;
    if (!row_live(lengths, t, b)) {
#pragma unroll
        for (int g = 0; g < 4; ++g) L::zero().store(row + g * H + j);
        return;  // dh and dc pass through untouched
    }
    const L vi = L::load(row + j), vf = L::load(row + H + j), vg = L::load(row + 2 * H + j), vo = L::load(row + 3 * H + j);
    const L vcp = L::load(c_prev + b * H + j), vcn = L::load(c_next + b * H + j);
    const L vdh = L::load(dh + b * H + j), vdc = L::load(dc + b * H + j);
    const L vdo = L::load_or_zero(d_out, b * H + j);
    L di, df, dg, dO, dcp;
#pragma unroll
    for (int k = 0; k < L::kW; ++k) {
        const float i = gru_sigmoid(vi[k]), f = gru_sigmoid(vf[k]), g = tanhf(vg[k]), o = gru_sigmoid(vo[k]);
        const float tc = tanhf(vcn[k]);
        const float dht = vdh[k] + vdo[k];
        const float dct = vdc[k] + dht * o * (1.0f - tc * tc);
        dO[k] = dht * tc * o * (1.0f - o);
        di[k] = dct * g * i * (1.0f - i);
        df[k] = dct * vcp[k] * f * (1.0f - f);
        dg[k] = dct * i * (1.0f - g * g);
        dcp[k] = dct * f;
    }
    di.store(row + j);
    df.store(row + H + j);
    dg.store(row + 2 * H + j);
    dO.store(row + 3 * H + j);
    dcp.store(dc + b * H + j);
    L::zero().store(dh + b * H + j);
}

// ---- vanilla RNN (torch.nn.RNN, tanh | relu): h' = act(gi + gh + b_hh).  The output IS the saved state: the backward
// needs act'(h') only, so nothing but `out` is kept; d(pre) is written over gi.
template <typename V, bool kRelu>
__global__ __launch_bounds__(kBlock) void rnn_cell_fwd_kernel(const float *__restrict__ gi, const float *__restrict__ gh,
                                                              const float *__restrict__ b_hh, float *__restrict__ h,
                                                              float *__restrict__ out,
                                                              const int64_t *__restrict__ lengths, int64_t t, int64_t B,
                                                              int H) {
    using L = Lanes<V>;
    const Element at = element<V>(B, H);
    if (at.none) return;
    const int64_t b = at.b;
    const int j = at.j;
    const L a = L::load(gi + b * H + j), r = L::load(gh + b * H + j), hp = L::load(h + b * H + j);
    const L bias = L::load_or_zero(b_hh, j);
    const bool live = row_live(lengths, t, b);
    L hn, o;
#pragma unroll
    for (int k = 0; k < L::kW; ++k) {
        const float pre = a[k] + r[k] + bias[k];
        const float next = kRelu ? fmaxf(pre, 0.0f) : tanhf(pre);
        hn[k] = live ? next : hp[k];
        o[k] = live ? next : 0.0f;
    }
    hn.store(h + b * H + j);
    o.store(out + b * H + j);
}

template <typename V, bool kRelu>
__global__ __launch_bounds__(kBlock) void rnn_cell_bwd_kernel(float *__restrict__ d_pre, const float *__restrict__ out,
                                                              const float *__restrict__ d_out, float *__restrict__ dh,
                                                              const int64_t *__restrict__ lengths, int64_t t, int64_t B,
                                                              int H) {
    using L = Lanes<V>;
    const Element at = element<V>(B, H);
    if (at.none) return;
    const int64_t b = at.b;
    const int j = at.j;
    if (!row_live(lengths, t, b)) {
        L::zero().store(d_pre + b * H + j);
        return;  // dh passes through
    }
    const L y = L::load(out + b * H + j), vdh = L::load(dh + b * H + j), vdo = L::load_or_zero(d_out, b * H + j);
    L g;
#pragma unroll
    for (int k = 0; k < L::kW; ++k) {
        const float dht = vdh[k] + vdo[k];
        g[k] = kRelu ? (y[k] > 0.0f ? dht : 0.0f) : dht * (1.0f - y[k] * y[k]);
    }
    g.store(d_pre + b * H + j);
    L::zero().store(dh + b * H + j);
}

// ---- host: one launch sequence for all seven entry points ---------------------------------------------------------------
enum Form { kNoForm, kScalar, kLanes };  // kNoForm: the pass does not take this launch (bias folding only)

// 16-byte lanes need H % 4 == 0 and every operand that is given on a 16-byte boundary; scalars otherwise.
static Form lane_form(int64_t H, std::initializer_list<const void *> operands) {
    if (H % 4 != 0) return kScalar;
    for (const void *p : operands)
        if (!aligned(p, 16)) return kScalar;  // (nullptr, an absent operand, counts as aligned)
    return kLanes;
}

// Which form of the bias-folding pass a launch with these pointers takes (every other argument valid), if any: the column
// chunks of a row have to tile a block, and the rows the block then has in flight have to fit into the rows it owns (wide
// or narrow layers that do not: the caller keeps the plain pass + column sums).  The ONE statement of that rule.
static Form bias_form(int64_t H, int rows_per_block, std::initializer_list<const void *> operands) {
    if (H <= 0 || H > INT32_MAX / 3) return kNoForm;
    const Form form = lane_form(H, operands);
    const int64_t cols = form == kLanes ? H / 4 : H;
    return cols <= kBlock && kBlock % cols == 0 && kBlock / cols <= rows_per_block ? form : kNoForm;
}

// The checks every entry point makes, in this order, then the launch.  `rows_per_block`: of the bias-folding pass; 0 for
// the element-per-thread passes (one thread per kW columns).  `pick(V{}, flag)` names the kernel instantiation: V = float4 |
// float by `form`, flag = std::true_type | std::false_type by `flag` for the kernels that have a second parameter.
template <typename Pick, typename... Args>
static int gate_pass(int64_t B, int64_t H, int64_t t, int gates, std::initializer_list<const void *> required, Form form,
                     int rows_per_block, bool flag, void *stream, Pick pick, Args... args) {
    if (B < 0 || H <= 0 || t < 0) return CUSRL_E_INVALID;
    if (B == 0) return 0;
    for (const void *p : required)
        if (!p) return CUSRL_E_INVALID;
    if (H > INT32_MAX / gates || form == kNoForm) return CUSRL_E_UNSUPPORTED;
    const int64_t blocks = rows_per_block ? ceil_div(B, rows_per_block) : ceil_div(B * (form == kLanes ? H / 4 : H), kBlock);
    if (blocks > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    const auto kernel = form == kLanes ? (flag ? pick(float4{}, std::true_type{}) : pick(float4{}, std::false_type{}))
                                       : (flag ? pick(float{}, std::true_type{}) : pick(float{}, std::false_type{}));
    hipLaunchKernelGGL(kernel, dim3(uint32_t(blocks)), dim3(kBlock), 0, as_stream(stream), args...);
    return launch_status();
}

}  // namespace cusrl

extern "C" int cusrl_gru_gates_fwd(const float *gi, const float *gh, const float *b_hh, float *h, float *out,
                                   const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 3, {gi, gh, h, out}, lane_form(H, {gi, gh, b_hh, h, out}), 0, false, stream,
                     [](auto v, auto) { return gru_gates_fwd_kernel<decltype(v)>; }, gi, gh, b_hh, h, out, lengths, t, B, int(H));
}

extern "C" int cusrl_gru_gates_bwd(float *gi, float *gh, const float *b_hh, const float *h_prev, const float *d_out,
                                   float *dh, const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 3, {gi, gh, h_prev, dh}, lane_form(H, {gi, gh, b_hh, h_prev, d_out, dh}), 0, false, stream,
                     [](auto v, auto) { return gru_gates_bwd_kernel<decltype(v)>; }, gi, gh, b_hh, h_prev, d_out, dh, lengths, t,
                     B, int(H));
}

extern "C" int64_t cusrl_gru_bias_partial_rows(int64_t B) { return B <= 0 ? 0 : cusrl::ceil_div(B, cusrl::bias_rows()); }

// 1: cusrl_gru_gates_bwd_bias takes a launch with these pointers (every other argument valid); 0: CUSRL_E_UNSUPPORTED.
// The host asks here instead of restating the rule (bias_form).
extern "C" int cusrl_gru_bias_supported(int64_t H, const float *gi, const float *gh, const float *b_hh, const float *h_prev,
                                        const float *d_out, const float *dh, const float *bias_partials) {
    return cusrl::bias_form(H, cusrl::bias_rows(), {gi, gh, b_hh, h_prev, d_out, dh, bias_partials}) != cusrl::kNoForm;
}

extern "C" int cusrl_gru_gates_bwd_bias(float *gi, float *gh, const float *b_hh, const float *h_prev, const float *d_out,
                                        float *dh, const int64_t *lengths, int64_t t, int64_t B, int64_t H,
                                        float *bias_partials, void *stream) {
    using namespace cusrl;
    const int rows_per_block = bias_rows();
    return gate_pass(B, H, t, 3, {gi, gh, h_prev, dh, bias_partials},
                     bias_form(H, rows_per_block, {gi, gh, b_hh, h_prev, d_out, dh, bias_partials}), rows_per_block, false, stream,
                     [](auto v, auto) { return gru_gates_bwd_bias_kernel<decltype(v)>; }, gi, gh, b_hh, h_prev, d_out, dh, lengths,
                     t, B, int(H), bias_partials, rows_per_block);
}

extern "C" int cusrl_lstm_gates_fwd(float *gi, const float *gh, const float *b_hh, float *h, float *c, float *out,
                                    float *c_saved, const int64_t *lengths, int64_t t, int64_t B, int64_t H,
                                    void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 4, {gi, gh, h, c, out}, lane_form(H, {gi, gh, b_hh, h, c, out, c_saved}), 0, c_saved != nullptr,
                     stream, [](auto v, auto save) { return lstm_gates_fwd_kernel<decltype(v), decltype(save)::value>; }, gi, gh,
                     b_hh, h, c, out, c_saved, lengths, t, B, int(H));
}

extern "C" int cusrl_lstm_gates_bwd(float *pre, const float *c_prev, const float *c_next, const float *d_out, float *dh,
                                    float *dc, const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 4, {pre, c_prev, c_next, dh, dc}, lane_form(H, {pre, c_prev, c_next, d_out, dh, dc}), 0, false,
                     stream, [](auto v, auto) { return lstm_gates_bwd_kernel<decltype(v)>; }, pre, c_prev, c_next, d_out, dh, dc,
                     lengths, t, B, int(H));
}

extern "C" int cusrl_rnn_cell_fwd(const float *gi, const float *gh, const float *b_hh, float *h, float *out,
                                  const int64_t *lengths, int64_t t, int64_t B, int64_t H, int relu, void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 1, {gi, gh, h, out}, lane_form(H, {gi, gh, b_hh, h, out}), 0, relu != 0, stream,
                     [](auto v, auto act) { return rnn_cell_fwd_kernel<decltype(v), decltype(act)::value>; }, gi, gh, b_hh, h, out,
                     lengths, t, B, int(H));
}

extern "C" int cusrl_rnn_cell_bwd(float *d_pre, const float *out, const float *d_out, float *dh, const int64_t *lengths,
                                  int64_t t, int64_t B, int64_t H, int relu, void *stream) {
    using namespace cusrl;
    return gate_pass(B, H, t, 1, {d_pre, out, dh}, lane_form(H, {d_pre, out, d_out, dh}), 0, relu != 0, stream,
                     [](auto v, auto act) { return rnn_cell_bwd_kernel<decltype(v), decltype(act)::value>; }, d_pre, out, d_out, dh,
                     lengths, t, B, int(H));
}
