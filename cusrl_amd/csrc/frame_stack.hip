// Observation history of a frame-stacking wrapper (cusrl_amd/nn/stacker.py ObservationStacker, cusrl_amd/environment/frame_stack.py
// FrameStack; DESIGN.md §7, "Frame stacking"; contracts: include/cusrl_hip.h).  The history H [N, S, K] keeps the last S
// observations of every env, slot 0 the oldest and slot S - 1 the newest; a stacked observation is H's own memory order,
// [N, S * K].  Written as torch ops a push is a slice, a cat, a clone and an indexed assignment per env step and the reset has no
// shape-static form at all; here it is
//   push    H[n, s] = H[n, s + 1] (s < S - 1), H[n, S - 1] = obs[n, columns], out[n] = H[n]        ONE launch
//   reset   H[indices[j]] refilled from reset_obs[j, columns] for j < *count, out[j] = H[indices[j]]   ONE launch
// Both only MOVE 32-bit words (as integers: no floating-point instruction sees them), so NaN payloads, -0.0 and Inf pass bit for
// bit; the padding word is +0.0.  One lane owns one column (n, k) — or four adjacent ones as one 16-byte word — through all S
// slots: it reads slot s + 1 before it writes slot s and no other lane touches those words, so the in-place shift has no race for
// any S.  Plain vector stores only.  The host restatements (`*_cpu`, below) are what the GPU tests compare bits against.
#include "common.hpp"

#include <string.h>

namespace cusrl {
namespace {

constexpr int kFrameStackMaxBlocks = 2048;  // 8 blocks per CU; the stride loops cover what is left

__host__ __device__ __forceinline__ uint32_t zero_word(const uint32_t *) { return 0u; }
__host__ __device__ __forceinline__ uint4 zero_word(const uint4 *) { return make_uint4(0u, 0u, 0u, 0u); }

// the word a lane stacks: column k of row `row` of the source, through the column table when there is one (an entry outside
// [0, K0) reads nothing and gives the padding word)
template <typename W>
__device__ __forceinline__ W source_word(const W *__restrict__ source, const int32_t *__restrict__ columns, int64_t row, int k, int K0) {
    if (columns == nullptr) return source[row * K0 + k];
    const int32_t column = columns[k];
    return uint32_t(column) < uint32_t(K0) ? source[row * K0 + column] : zero_word(static_cast<const W *>(nullptr));
}

// W = uint32_t: one column per lane; W = uint4: four adjacent columns per lane (no column table, K % 4 == 0, K counted in words).
// A block takes tiles of `tile_rows` whole rows (256 / K of them, at least one), its threads the tile's rows * K column lanes: every
// lane of a row reads the row's `fresh` flag in front of the block's barrier and the flag is cleared behind it, by this block alone.
template <typename W>
__global__ __launch_bounds__(kBlock) void frame_stack_push_kernel(W *H, const W *__restrict__ obs, const int32_t *__restrict__ columns,
                                                                  uint8_t *fresh, W *__restrict__ out, int64_t N, int S, int K, int K0,
                                                                  int padding, int tile_rows, int64_t tiles) {
    const W zero = zero_word(static_cast<const W *>(nullptr));
    const int64_t pitch = int64_t(S) * K;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t first = tile * tile_rows;
        const int rows = int(N - first < tile_rows ? N - first : tile_rows);
        const int64_t lanes = int64_t(rows) * K;
        for (int64_t lane = threadIdx.x; lane < lanes; lane += kBlock) {
            const int64_t n = first + lane / K;
            const int k = int(lane % K);
            const W newest = source_word(obs, columns, n, k, K0);
            const bool refill = fresh != nullptr && fresh[n] != 0;
            const W pad = padding == CUSRL_FRAME_STACK_PAD_RESET ? newest : zero;
            W *h = H + n * pitch + k;
            W *o = out + n * pitch + k;
            for (int s = 0; s + 1 < S; ++s) {  // ascending: slot s + 1 is read before slot s is written, by this lane alone
                const W word = refill ? pad : h[int64_t(s + 1) * K];
                h[int64_t(s) * K] = word;
                o[int64_t(s) * K] = word;
            }
            h[int64_t(S - 1) * K] = newest;
            o[int64_t(S - 1) * K] = newest;
        }
        if (fresh != nullptr) {  // (block-uniform)
            __syncthreads();
            for (int r = threadIdx.x; r < rows; r += kBlock)
                if (fresh[first + r] != 0) fresh[first + r] = 0;
        }
    }
}

// One lane per (slot j, column k).  j < live: H[indices[j]] is refilled and copied to out[j]; j >= live: out[j] is what
// H[indices[j]] holds and H is not written.  An id outside [0, N) touches no history; its out row is the padding word.
template <typename W>
__global__ __launch_bounds__(kBlock) void frame_stack_reset_kernel(W *H, const int64_t *__restrict__ indices, const int32_t *__restrict__ count,
                                                                   const W *__restrict__ reset_obs, const int32_t *__restrict__ columns,
                                                                   W *__restrict__ out, int64_t L, int64_t N, int S, int K, int K0, int padding,
                                                                   int64_t lanes) {
    const W zero = zero_word(static_cast<const W *>(nullptr));
    const int64_t pitch = int64_t(S) * K, stride = int64_t(gridDim.x) * kBlock;
    int64_t live = count != nullptr ? int64_t(*count) : L;
    live = live < 0 ? 0 : (live > L ? L : live);
    for (int64_t lane = int64_t(blockIdx.x) * kBlock + threadIdx.x; lane < lanes; lane += stride) {
        const int64_t j = lane / K;
        const int k = int(lane % K);
        const int64_t env = indices[j];
        W *o = out + j * pitch + k;
        if (env < 0 || env >= N) {
            for (int s = 0; s < S; ++s) o[int64_t(s) * K] = zero;
            continue;
        }
        W *h = H + env * pitch + k;
        if (j < live) {
            const W newest = source_word(reset_obs, columns, j, k, K0);
            const W pad = padding == CUSRL_FRAME_STACK_PAD_RESET ? newest : zero;
            for (int s = 0; s < S; ++s) {
                const W word = s == S - 1 ? newest : pad;
                h[int64_t(s) * K] = word;
                o[int64_t(s) * K] = word;
            }
        } else {
            for (int s = 0; s < S; ++s) o[int64_t(s) * K] = h[int64_t(s) * K];
        }
    }
}

bool overlap(const void *a, int64_t a_bytes, const void *b, int64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + uintptr_t(b_bytes) && y < x + uintptr_t(a_bytes);
}

// extents and pairs shared by the four entries; `rows` is N (push) or L (reset)
int check_extents(int64_t rows, int64_t N, int64_t S, int64_t K, int64_t K0, const void *columns, int padding) {
    if (rows < 0 || N < 0 || S < 1 || K < 1 || K0 < 1) return CUSRL_E_INVALID;
    if (padding != CUSRL_FRAME_STACK_PAD_RESET && padding != CUSRL_FRAME_STACK_PAD_ZERO) return CUSRL_E_INVALID;
    if (columns == nullptr && K != K0) return CUSRL_E_INVALID;
    if (S > INT32_MAX || K > INT32_MAX || K0 > INT32_MAX) return CUSRL_E_UNSUPPORTED;
    if (S > INT64_MAX / 4 / K) return CUSRL_E_UNSUPPORTED;
    const int64_t pitch = S * K;
    const int64_t most = rows > N ? rows : N;
    if (most > 0 && (pitch > INT64_MAX / 4 / most || K0 > INT64_MAX / 4 / most)) return CUSRL_E_UNSUPPORTED;
    return 0;
}

int check_push(const void *H, const void *obs, const void *columns, const void *out, int64_t N, int64_t S, int64_t K, int64_t K0,
               int padding) {
    if (int rc = check_extents(N, N, S, K, K0, columns, padding)) return rc;
    if (N == 0) return 0;
    if (!H || !obs || !out) return CUSRL_E_INVALID;
    if (!aligned(H, 4) || !aligned(obs, 4) || !aligned(out, 4) || !aligned(columns, 4)) return CUSRL_E_INVALID;
    if (overlap(H, N * S * K * 4, out, N * S * K * 4)) return CUSRL_E_INVALID;
    return 0;
}

int check_reset(const void *H, const void *indices, const void *count, const void *reset_obs, const void *columns, const void *out,
                int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0, int padding) {
    if (int rc = check_extents(L, N, S, K, K0, columns, padding)) return rc;
    if (L == 0) return 0;
    if (!indices || !reset_obs || !out || (N > 0 && !H)) return CUSRL_E_INVALID;
    if (!aligned(H, 4) || !aligned(reset_obs, 4) || !aligned(out, 4) || !aligned(columns, 4) || !aligned(count, 4) || !aligned(indices, 8))
        return CUSRL_E_INVALID;
    if (N > 0 && overlap(H, N * S * K * 4, out, L * S * K * 4)) return CUSRL_E_INVALID;
    return 0;
}

int capped(int64_t blocks) { return int(blocks < 1 ? 1 : (blocks > kFrameStackMaxBlocks ? kFrameStackMaxBlocks : blocks)); }

template <typename W>
void launch_push(float *H, const float *obs, const int32_t *columns, uint8_t *fresh, float *out, int64_t N, int64_t S, int64_t K,
                 int64_t K0, int padding, void *stream) {
    const int tile_rows = K >= kBlock ? 1 : int(kBlock / K);
    const int64_t tiles = ceil_div(N, tile_rows);
    hipLaunchKernelGGL(frame_stack_push_kernel<W>, dim3(capped(tiles)), dim3(kBlock), 0, as_stream(stream), reinterpret_cast<W *>(H),
                       reinterpret_cast<const W *>(obs), columns, fresh, reinterpret_cast<W *>(out), N, int(S), int(K), int(K0), padding,
                       tile_rows, tiles);
}

template <typename W>
void launch_reset(float *H, const int64_t *indices, const int32_t *count, const float *reset_obs, const int32_t *columns, float *out,
                  int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0, int padding, void *stream) {
    const int64_t lanes = L * K;
    hipLaunchKernelGGL(frame_stack_reset_kernel<W>, dim3(capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, as_stream(stream),
                       reinterpret_cast<W *>(H), indices, count, reinterpret_cast<const W *>(reset_obs), columns,
                       reinterpret_cast<W *>(out), L, N, int(S), int(K), int(K0), padding, lanes);
}

// host restatement of source_word
uint32_t host_word(const float *source, const int32_t *columns, int64_t row, int64_t k, int64_t K0) {
    int64_t column = k;
    if (columns) {
        column = columns[k];
        if (column < 0 || column >= K0) return 0u;
    }
    uint32_t word;
    memcpy(&word, source + row * K0 + column, sizeof word);
    return word;
}

void store_word(float *destination, uint32_t word) { memcpy(destination, &word, sizeof word); }

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_frame_stack_push(float *H, const float *obs, const int32_t *columns, uint8_t *fresh, float *out, int64_t N, int64_t S,
                                      int64_t K, int64_t K0, int padding, void *stream) {
    if (int rc = check_push(H, obs, columns, out, N, S, K, K0, padding)) return rc;
    if (N == 0) return 0;
    if (columns == nullptr && K % 4 == 0 && aligned(H, 16) && aligned(obs, 16) && aligned(out, 16))
        launch_push<uint4>(H, obs, nullptr, fresh, out, N, S, K / 4, K0 / 4, padding, stream);
    else
        launch_push<uint32_t>(H, obs, columns, fresh, out, N, S, K, K0, padding, stream);
    return launch_status();
}

extern "C" int cusrl_frame_stack_push_cpu(float *H, const float *obs, const int32_t *columns, uint8_t *fresh, float *out, int64_t N,
                                          int64_t S, int64_t K, int64_t K0, int padding) {
    if (int rc = check_push(H, obs, columns, out, N, S, K, K0, padding)) return rc;
    for (int64_t n = 0; n < N; ++n) {
        const bool refill = fresh && fresh[n];
        for (int64_t k = 0; k < K; ++k) {
            const uint32_t newest = host_word(obs, columns, n, k, K0);
            const uint32_t pad = padding == CUSRL_FRAME_STACK_PAD_RESET ? newest : 0u;
            float *h = H + n * S * K + k, *o = out + n * S * K + k;
            for (int64_t s = 0; s + 1 < S; ++s) {
                uint32_t word = pad;
                if (!refill) memcpy(&word, h + (s + 1) * K, sizeof word);
                store_word(h + s * K, word);
                store_word(o + s * K, word);
            }
            store_word(h + (S - 1) * K, newest);
            store_word(o + (S - 1) * K, newest);
        }
        if (refill) fresh[n] = 0;
    }
    return 0;
}

extern "C" int cusrl_frame_stack_reset(float *H, const int64_t *indices, const int32_t *count, const float *reset_obs,
                                       const int32_t *columns, float *out, int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0,
                                       int padding, void *stream) {
    if (int rc = check_reset(H, indices, count, reset_obs, columns, out, L, N, S, K, K0, padding)) return rc;
    if (L == 0) return 0;
    if (columns == nullptr && K % 4 == 0 && aligned(H, 16) && aligned(reset_obs, 16) && aligned(out, 16))
        launch_reset<uint4>(H, indices, count, reset_obs, nullptr, out, L, N, S, K / 4, K0 / 4, padding, stream);
    else
        launch_reset<uint32_t>(H, indices, count, reset_obs, columns, out, L, N, S, K, K0, padding, stream);
    return launch_status();
}

extern "C" int cusrl_frame_stack_reset_cpu(float *H, const int64_t *indices, const int32_t *count, const float *reset_obs,
                                           const int32_t *columns, float *out, int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0,
                                           int padding) {
    if (int rc = check_reset(H, indices, count, reset_obs, columns, out, L, N, S, K, K0, padding)) return rc;
    int64_t live = count ? int64_t(*count) : L;
    live = live < 0 ? 0 : (live > L ? L : live);
    for (int64_t j = 0; j < L; ++j) {
        const int64_t env = indices[j];
        for (int64_t k = 0; k < K; ++k) {
            float *o = out + j * S * K + k;
            if (env < 0 || env >= N) {
                for (int64_t s = 0; s < S; ++s) store_word(o + s * K, 0u);
                continue;
            }
            float *h = H + env * S * K + k;
            if (j < live) {
                const uint32_t newest = host_word(reset_obs, columns, j, k, K0);
                const uint32_t pad = padding == CUSRL_FRAME_STACK_PAD_RESET ? newest : 0u;
                for (int64_t s = 0; s < S; ++s) {
                    store_word(h + s * K, s == S - 1 ? newest : pad);
                    store_word(o + s * K, s == S - 1 ? newest : pad);
                }
            } else {
                for (int64_t s = 0; s < S; ++s) memcpy(o + s * K, h + s * K, sizeof(float));
            }
        }
    }
    return 0;
}
