// The element expressions of the recurrent cells, shared by the per-step gate passes (gru.hip: forward and backward) and the
// one-launch time step (recurrent_step.hip): one statement of each, so the two paths evaluate a gate with the same instructions.
#pragma once

#include "common.hpp"

namespace cusrl {

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

struct GruGates {
    float r, z, q, n;
};

// gi = W_ih x + b_ih, gh = W_hh h, b = b_hh (torch.nn.GRU: the n gate's recurrent projection is scaled by r before it is added)
__device__ __forceinline__ GruGates gru_gates(float gi_r, float gi_z, float gi_n, float gh_r, float gh_z, float gh_n,
                                              float b_r, float b_z, float b_n) {
    GruGates g;
    g.r = gru_sigmoid(gi_r + gh_r + b_r);
    g.z = gru_sigmoid(gi_z + gh_z + b_z);
    g.q = gh_n + b_n;
    g.n = tanhf(gi_n + g.r * g.q);
    return g;
}

// h' of the GRU
__device__ __forceinline__ float gru_next(const GruGates &g, float h) { return (1.0f - g.z) * g.n + g.z * h; }

struct LstmState {
    float c, h;
};

// c', h' of the LSTM from the four summed pre-activations (gate order i, f, g, o as torch.nn.LSTM) and the previous cell state
__device__ __forceinline__ LstmState lstm_next(float pre_i, float pre_f, float pre_g, float pre_o, float c) {
    LstmState s;
    s.c = gru_sigmoid(pre_f) * c + gru_sigmoid(pre_i) * tanhf(pre_g);
    s.h = gru_sigmoid(pre_o) * tanhf(s.c);
    return s;
}

}  // namespace cusrl
