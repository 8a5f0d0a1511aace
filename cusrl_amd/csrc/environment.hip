// Five classic-control tasks as device-resident environments (cusrl_amd/environment/; DESIGN.md, "Classic-control
// environments"; contracts: include/cusrl_hip.h): CartPole, Pendulum, MountainCar, Acrobot and MountainCarContinuous with the
// constants and update order of their textbook forms.  Per env a contiguous fp32 state row, an int32 step counter and an int64 episode counter, all in HBM;
//   cusrl_classic_step    ONE launch: advance state and counter in place, write observation, reward and the two flags
//   cusrl_classic_reset   ONE launch: re-initialise the envs behind the first `count` index slots from Philox draws keyed on
//                         (seed, env, episode), write one observation row per slot
// ONE THREAD PER ENV (step) or per index slot (reset).  A step thread reads and writes only its own env's row of every array,
// so the in-place update has no cross-thread hazard; a reset thread below `count` owns env indices[k] (the ids there are
// distinct), a thread at or above `count` only reads.  Every step of the arithmetic is one rounded fp32 operation (the library
// is built with -ffp-contract=off); the bodies are __host__ __device__ and the `*_cpu` entries run the same bodies on the
// host, so the two differ only where sinf / cosf do.  Plain vector stores only.  No loop's trip count depends on data: Acrobot's
// angle wrap is a closed form (a `while` over a NaN, an Inf or a huge loaded angle would not end).
//
// Layout.  A TASK IS ONE BLOCK: `Task<kind>` holds the row widths and its own `observe`, `advance` and `initial_state`.  What runs
// a task is written once over `Task<kind>`: `step_env` (one env of the step) and `reset_slot` (one index slot of the reset), each
// called per thread by its kernel and per loop iteration by its `*_cpu` entry.  `for_task` is the one place that maps a runtime
// kind to its `Task<>`.  A new task: one `Task<>` block, one line in `for_task`, one `#define` in the header.
#include "common.hpp"
#include "philox.hpp"

#include <math.h>

#include <type_traits>

namespace cusrl {
namespace {

constexpr float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f;

__host__ __device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// the first maximal column (a NaN never wins against column 0)
template <int kN>
__host__ __device__ __forceinline__ int first_max(const float *a) {
    int best = 0;
#pragma unroll
    for (int j = 1; j < kN; ++j)
        if (a[j] > a[best]) best = j;
    return best;
}

// ---- the tasks.  kState / kAction / kObservation: the row widths; kObservationBytes: the widest access an observation row moves
// by where it is aligned to it (4: scalars); observe: state row -> observation row; advance: ONE transition, s advanced in place,
// returns `terminated`; initial_state: the state of a fresh episode from one Philox call (documented ranges: include/cusrl_hip.h).
template <int kKind>
struct Task;

template <int kWidth>
struct ObservesItsState {  // the observation is the state row
    static constexpr int kState = kWidth, kObservation = kWidth, kObservationBytes = 4 * kWidth;
    static __host__ __device__ __forceinline__ void observe(const float *s, float *o) {
#pragma unroll
        for (int j = 0; j < kWidth; ++j) o[j] = s[j];
    }
};

template <>
struct Task<CUSRL_CLASSIC_CARTPOLE> : ObservesItsState<4> {  // state x, x', theta, theta'; action: logits over {push left, push right}
    static constexpr int kAction = 2;
    static __host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
        constexpr float kGravity = 9.8f, kTotalMass = 1.1f, kPoleMass = 0.1f, kLength = 0.5f, kPoleMassLength = 0.05f, kTau = 0.02f;
        const float force = first_max<2>(a) == 1 ? 10.0f : -10.0f;
        const float x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
        const float cos_theta = cosf(theta), sin_theta = sinf(theta);
        const float temp = (force + kPoleMassLength * (theta_dot * theta_dot) * sin_theta) / kTotalMass;
        const float theta_acc = (kGravity * sin_theta - cos_theta * temp) /
                                (kLength * (4.0f / 3.0f - kPoleMass * (cos_theta * cos_theta) / kTotalMass));
        const float x_acc = temp - kPoleMassLength * theta_acc * cos_theta / kTotalMass;
        s[0] = x + kTau * x_dot;  // explicit Euler: every line uses the old derivatives
        s[1] = x_dot + kTau * x_acc;
        s[2] = theta + kTau * theta_dot;
        s[3] = theta_dot + kTau * theta_acc;
        reward = 1.0f;
        return fabsf(s[0]) > 2.4f || fabsf(s[2]) > 0.20943951023931953f;  // 12 degrees
    }
    static __host__ __device__ __forceinline__ void initial_state(const Philox &r, float *s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = -0.05f + 0.1f * philox_uniform(r.c[j]);
    }
};

template <>
struct Task<CUSRL_CLASSIC_PENDULUM> {  // state theta, theta'; action: one torque; observation cos, sin, theta'
    static constexpr int kState = 2, kAction = 1, kObservation = 3, kObservationBytes = 4;
    static __host__ __device__ __forceinline__ void observe(const float *s, float *o) {
        o[0] = cosf(s[0]);
        o[1] = sinf(s[0]);
        o[2] = s[1];
    }
    static __host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
        constexpr float kDt = 0.05f;
        const float u = clampf(a[0], -2.0f, 2.0f);
        const float theta = s[0], theta_dot = s[1];
        float wrapped = fmodf(theta + kPi, kTwoPi);  // Python's floor-mod: the sign of the divisor
        if (wrapped < 0.0f) wrapped = wrapped + kTwoPi;
        wrapped = wrapped - kPi;
        reward = -(wrapped * wrapped + 0.1f * (theta_dot * theta_dot) + 0.001f * (u * u));  // of the OLD state
        s[1] = clampf(theta_dot + (15.0f * sinf(theta) + 3.0f * u) * kDt, -8.0f, 8.0f);  // 3g / (2l) = 15, 3 / (m l^2) = 3
        s[0] = theta + s[1] * kDt;
        return false;
    }
    static __host__ __device__ __forceinline__ void initial_state(const Philox &r, float *s) {
        s[0] = -kPi + kTwoPi * philox_uniform(r.c[0]);
        s[1] = -1.0f + 2.0f * philox_uniform(r.c[1]);
    }
};

// What the two mountain cars share: state position, velocity; the start; and everything after the raw velocity increment.  The
// increment itself is each task's own: the two associate it differently, and each keeps its textbook order.
struct MountainCarTrack : ObservesItsState<2> {
    static __host__ __device__ __forceinline__ void move(float *s, float raw_velocity) {
        float velocity = clampf(raw_velocity, -0.07f, 0.07f);
        const float position = clampf(s[0] + velocity, -1.2f, 0.6f);
        if (position == -1.2f && velocity < 0.0f) velocity = 0.0f;  // the left wall is inelastic
        s[0] = position;
        s[1] = velocity;
    }
    static __host__ __device__ __forceinline__ void initial_state(const Philox &r, float *s) {
        s[0] = -0.6f + 0.2f * philox_uniform(r.c[0]);
        s[1] = 0.0f;
    }
};

template <>
struct Task<CUSRL_CLASSIC_MOUNTAINCAR> : MountainCarTrack {  // action: logits over {left, none, right}
    static constexpr int kAction = 3;
    static __host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
        const int push = first_max<3>(a);
        move(s, s[1] + float(push - 1) * 0.001f - 0.0025f * cosf(3.0f * s[0]));
        reward = -1.0f;
        return s[0] >= 0.5f && s[1] >= 0.0f;
    }
};

template <>
struct Task<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS> : MountainCarTrack {  // action: one force
    static constexpr int kAction = 1;
    static __host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
        const float force = clampf(a[0], -1.0f, 1.0f);
        move(s, s[1] + (force * 0.0015f - 0.0025f * cosf(3.0f * s[0])));
        const bool ended = s[0] >= 0.45f && s[1] >= 0.0f;
        reward = (ended ? 100.0f : 0.0f) - 0.1f * (a[0] * a[0]);  // the RAW action, not the clamped force
        return ended;
    }
};

// Acrobot's equations of motion with the unit constants folded (m1 = m2 = l1 = I1 = I2 = 1, lc1 = lc2 = 0.5, g = 9.8) and
// sin x for cos(x - pi/2): d = (theta1', theta2', theta1'', theta2'') at s under a constant torque
__host__ __device__ __forceinline__ void acrobot_derivative(const float *s, float torque, float *d) {
    const float theta1 = s[0], theta2 = s[1], omega1 = s[2], omega2 = s[3];
    float sin2, cos2;
    sincosf(theta2, &sin2, &cos2);
    const float d1 = 3.5f + cos2;
    const float d2 = 1.25f + 0.5f * cos2;
    const float phi2 = 4.9f * sinf(theta1 + theta2);
    const float phi1 = -0.5f * (omega2 * omega2) * sin2 - omega2 * omega1 * sin2 + 14.7f * sinf(theta1) + phi2;
    const float acc2 = (torque + d2 / d1 * phi1 - 0.5f * (omega1 * omega1) * sin2 - phi2) / (1.25f - d2 * d2 / d1);
    d[0] = omega1;
    d[1] = omega2;
    d[2] = -((d2 * acc2 + phi1) / d1);
    d[3] = acc2;
}

// x into [-pi, pi] by whole turns, loop-free: a NaN stays a NaN, an Inf becomes one
__host__ __device__ __forceinline__ float wrap_angle(float x) {
    if (x > kPi) return x - kTwoPi * ceilf((x - kPi) / kTwoPi);
    if (x < -kPi) return x + kTwoPi * ceilf((-kPi - x) / kTwoPi);
    return x;
}

template <>
struct Task<CUSRL_CLASSIC_ACROBOT> {  // state theta1, theta2, theta1', theta2'; action: logits over torque {-1, 0, +1};
    static constexpr int kState = 4, kAction = 3, kObservation = 6, kObservationBytes = 8;  // observation cos, sin, cos, sin, ', '
    static __host__ __device__ __forceinline__ void observe(const float *s, float *o) {
        o[0] = cosf(s[0]);
        o[1] = sinf(s[0]);
        o[2] = cosf(s[1]);
        o[3] = sinf(s[1]);
        o[4] = s[2];
        o[5] = s[3];
    }
    static __host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
        constexpr float kHalfDt = 0.1f, kDt = 0.2f, kSixthDt = 0.2f / 6.0f;  // (the fp32 quotient)
        const float torque = float(first_max<3>(a) - 1);
        float k1[4], k2[4], k3[4], k4[4], y[4];  // classical Runge-Kutta over [0, dt], the torque held
        acrobot_derivative(s, torque, k1);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + kHalfDt * k1[j];
        acrobot_derivative(y, torque, k2);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + kHalfDt * k2[j];
        acrobot_derivative(y, torque, k3);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + kDt * k3[j];
        acrobot_derivative(y, torque, k4);
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = s[j] + kSixthDt * (k1[j] + 2.0f * k2[j] + 2.0f * k3[j] + k4[j]);
        s[0] = wrap_angle(y[0]);
        s[1] = wrap_angle(y[1]);
        s[2] = clampf(y[2], -12.566370614359172f, 12.566370614359172f);  // 4 pi
        s[3] = clampf(y[3], -28.274333882308138f, 28.274333882308138f);  // 9 pi
        const bool ended = -cosf(s[0]) - cosf(s[0] + s[1]) > 1.0f;
        reward = ended ? 0.0f : -1.0f;
        return ended;
    }
    static __host__ __device__ __forceinline__ void initial_state(const Philox &r, float *s) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = -0.1f + 0.2f * philox_uniform(r.c[j]);
    }
};

// The one map from a runtime kind to its Task<>: f(integral_constant<int, kind>) -> status; an unknown kind is CUSRL_E_INVALID.
template <typename F>
int for_task(int kind, F &&f) {
    switch (kind) {
        case CUSRL_CLASSIC_CARTPOLE: return f(std::integral_constant<int, CUSRL_CLASSIC_CARTPOLE>{});
        case CUSRL_CLASSIC_PENDULUM: return f(std::integral_constant<int, CUSRL_CLASSIC_PENDULUM>{});
        case CUSRL_CLASSIC_MOUNTAINCAR: return f(std::integral_constant<int, CUSRL_CLASSIC_MOUNTAINCAR>{});
        case CUSRL_CLASSIC_ACROBOT: return f(std::integral_constant<int, CUSRL_CLASSIC_ACROBOT>{});
        case CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS: return f(std::integral_constant<int, CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS>{});
    }
    return CUSRL_E_INVALID;
}

// counter = (env id, episode number with the stream in its two top bits), key = seed.  Stream 0: the state, 1: the progress.
__host__ __device__ __forceinline__ Philox episode_draw(uint64_t seed, int64_t env, int64_t episode, uint32_t stream) {
    const uint64_t e = uint64_t(env), n = uint64_t(episode);
    return philox4x32_10(uint32_t(e), uint32_t(e >> 32), uint32_t(n), (uint32_t(n >> 32) & 0x3fffffffu) | (stream << 30), uint32_t(seed),
                         uint32_t(seed >> 32));
}

// kVec: the state rows (and the observation rows of the tasks whose observation is the state) move as one 16- or 8-byte access,
// Acrobot's 6-wide observation row as three 8-byte ones
template <int kWidth, bool kVec>
__host__ __device__ __forceinline__ void load_row(const float *p, float *v) {
    if constexpr (kVec && kWidth == 4) {
        const float4 r = *reinterpret_cast<const float4 *>(p);
        v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
    } else if constexpr (kVec && kWidth == 2) {
        const float2 r = *reinterpret_cast<const float2 *>(p);
        v[0] = r.x, v[1] = r.y;
    } else {
#pragma unroll
        for (int j = 0; j < kWidth; ++j) v[j] = p[j];
    }
}
template <int kWidth, bool kVec>
__host__ __device__ __forceinline__ void store_row(float *p, const float *v) {
    if constexpr (kVec && kWidth == 4) {
        *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else if constexpr (kVec && kWidth == 2) {
        *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
    } else if constexpr (kVec && kWidth == 6) {
#pragma unroll
        for (int j = 0; j < 6; j += 2) *reinterpret_cast<float2 *>(p + j) = make_float2(v[j], v[j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < kWidth; ++j) p[j] = v[j];
    }
}

// ---- one env of the step, rows already in registers: shared by the kernel and cusrl_classic_step_cpu
template <int kKind>
__host__ __device__ __forceinline__ void step_env(float *s, const float *a, int32_t &steps, int32_t max_steps, float *o, float &reward,
                                                  uint8_t &terminated, uint8_t &truncated) {
    const bool ended = Task<kKind>::advance(s, a, reward);
    steps = steps + 1;
    terminated = ended ? 1 : 0;
    truncated = (!ended && steps >= max_steps) ? 1 : 0;
    Task<kKind>::observe(s, o);
}

// ---- index slot k of the reset, through local rows: shared by the kernel and cusrl_classic_reset_cpu
template <int kKind>
__host__ __device__ __forceinline__ void reset_slot(int64_t k, uint64_t seed, const int64_t *indices, const int32_t *count, float *state,
                                                    int32_t *steps, int64_t *episode, float *observation_out, int64_t rows,
                                                    int randomize_progress, int32_t max_steps, int64_t N) {
    using T = Task<kKind>;
    const int64_t live = count ? int64_t(*count) : rows;  // (a count beyond `rows` covers every slot, a negative one none)
    const int64_t e = indices[k];
    float s[T::kState], o[T::kObservation];
    if (e < 0 || e >= N) {  // not an env: nothing is touched, the slot's row is zeros
#pragma unroll
        for (int j = 0; j < T::kObservation; ++j) observation_out[k * T::kObservation + j] = 0.0f;
        return;
    }
    if (k < live) {  // a new episode of env e
        int64_t number = episode[e];
        T::initial_state(episode_draw(seed, e, number, 0u), s);
        int32_t progress = 0;
        if (randomize_progress)  // floor(max_steps * word / 2^32): an integer in [0, max_steps)
            progress = int32_t((uint64_t(episode_draw(seed, e, number, 1u).c[0]) * uint64_t(uint32_t(max_steps))) >> 32);
        number = number + 1;
        store_row<T::kState, false>(state + e * T::kState, s);
        steps[e] = progress;
        episode[e] = number;
    } else {
        load_row<T::kState, false>(state + e * T::kState, s);
    }
    T::observe(s, o);
    store_row<T::kObservation, false>(observation_out + k * T::kObservation, o);
}

template <int kKind, bool kVec>
__global__ __launch_bounds__(kBlock) void classic_step_kernel(const float *__restrict__ action, float *state, int32_t *steps,
                                                              int32_t max_steps, float *__restrict__ next_observation,
                                                              float *__restrict__ reward, uint8_t *__restrict__ terminated,
                                                              uint8_t *__restrict__ truncated, int64_t N) {
    using T = Task<kKind>;
    const int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= N) return;
    float s[T::kState], a[T::kAction], o[T::kObservation], r;
    load_row<T::kState, kVec>(state + i * T::kState, s);
    load_row<T::kAction, false>(action + i * T::kAction, a);
    int32_t count = steps[i];
    uint8_t ended, cut;
    step_env<kKind>(s, a, count, max_steps, o, r, ended, cut);
    store_row<T::kState, kVec>(state + i * T::kState, s);
    steps[i] = count;
    store_row<T::kObservation, kVec && (T::kObservationBytes > 4)>(next_observation + i * T::kObservation, o);
    reward[i] = r;
    terminated[i] = ended;
    truncated[i] = cut;
}

template <int kKind>
__global__ __launch_bounds__(kBlock) void classic_reset_kernel(uint64_t seed, const int64_t *__restrict__ indices,
                                                               const int32_t *__restrict__ count, float *state, int32_t *steps,
                                                               int64_t *episode, float *__restrict__ observation_out, int64_t rows,
                                                               int randomize_progress, int32_t max_steps, int64_t N) {
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= rows) return;
    reset_slot<kKind>(k, seed, indices, count, state, steps, episode, observation_out, rows, randomize_progress, max_steps, N);
}

int check_step(const void *action, const void *state, const void *steps, int64_t max_steps, const void *next_observation,
               const void *reward, const void *terminated, const void *truncated, int64_t N) {
    if (N < 0 || max_steps < 1 || max_steps > INT32_MAX) return CUSRL_E_INVALID;
    if (N > 0 && (!action || !state || !steps || !next_observation || !reward || !terminated || !truncated)) return CUSRL_E_INVALID;
    if (N > int64_t(INT32_MAX) * kBlock / 4) return CUSRL_E_UNSUPPORTED;
    return 0;
}

int check_reset(const void *indices, const void *state, const void *steps, const void *episode, const void *observation_out,
                int64_t rows, int64_t max_steps, int64_t N) {
    if (N < 0 || rows < 0 || max_steps < 1 || max_steps > INT32_MAX) return CUSRL_E_INVALID;
    if (rows > 0 && (N < 1 || !indices || !state || !steps || !episode || !observation_out)) return CUSRL_E_INVALID;
    if (rows > int64_t(INT32_MAX) * kBlock / 4 || N > int64_t(INT32_MAX) * kBlock / 4) return CUSRL_E_UNSUPPORTED;
    return 0;
}

template <int kKind>
void launch_step(const float *action, float *state, int32_t *steps, int32_t max_steps, float *next_observation, float *reward,
                 uint8_t *terminated, uint8_t *truncated, int64_t N, hipStream_t stream) {
    using T = Task<kKind>;
    const dim3 grid(uint32_t(ceil_div(N, kBlock))), block(kBlock);
    const bool vec = aligned(state, 4 * T::kState) && aligned(next_observation, T::kObservationBytes);
    if (vec)
        hipLaunchKernelGGL((classic_step_kernel<kKind, true>), grid, block, 0, stream, action, state, steps, max_steps,
                           next_observation, reward, terminated, truncated, N);
    else
        hipLaunchKernelGGL((classic_step_kernel<kKind, false>), grid, block, 0, stream, action, state, steps, max_steps,
                           next_observation, reward, terminated, truncated, N);
}

template <int kKind>
void launch_reset(uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps, int64_t *episode,
                  float *observation_out, int64_t rows, int randomize_progress, int32_t max_steps, int64_t N, hipStream_t stream) {
    hipLaunchKernelGGL(classic_reset_kernel<kKind>, dim3(uint32_t(ceil_div(rows, kBlock))), dim3(kBlock), 0, stream, seed, indices, count,
                       state, steps, episode, observation_out, rows, randomize_progress, max_steps, N);
}

}  // namespace
}  // namespace cusrl

using namespace cusrl;

// In every entry the kind is looked at first: an unknown one is CUSRL_E_INVALID whatever the other arguments are.
extern "C" int cusrl_classic_step(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps,
                                  float *next_observation, float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N,
                                  void *stream) {
    return for_task(kind, [&](auto task) {
        if (int rc = check_step(action, state, steps, max_steps, next_observation, reward, terminated, truncated, N)) return rc;
        if (N == 0) return 0;
        if (!aligned(action, 4) || !aligned(state, 4) || !aligned(steps, 4) || !aligned(next_observation, 4) || !aligned(reward, 4))
            return int(CUSRL_E_INVALID);
        launch_step<task.value>(action, state, steps, int32_t(max_steps), next_observation, reward, terminated, truncated, N, as_stream(stream));
        return launch_status();
    });
}

extern "C" int cusrl_classic_step_cpu(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps,
                                      float *next_observation, float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N) {
    return for_task(kind, [&](auto task) {
        using T = Task<task.value>;
        if (int rc = check_step(action, state, steps, max_steps, next_observation, reward, terminated, truncated, N)) return rc;
        for (int64_t i = 0; i < N; ++i)
            step_env<task.value>(state + i * T::kState, action + i * T::kAction, steps[i], int32_t(max_steps),
                                 next_observation + i * T::kObservation, reward[i], terminated[i], truncated[i]);
        return 0;
    });
}

extern "C" int cusrl_classic_reset(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps,
                                   int64_t *episode, float *observation_out, int64_t rows, int randomize_progress, int64_t max_steps,
                                   int64_t N, void *stream) {
    return for_task(kind, [&](auto task) {
        if (int rc = check_reset(indices, state, steps, episode, observation_out, rows, max_steps, N)) return rc;
        if (rows == 0) return 0;
        if (!aligned(indices, 8) || !aligned(episode, 8) || !aligned(state, 4) || !aligned(steps, 4) || !aligned(observation_out, 4) ||
            (count && !aligned(count, 4)))
            return int(CUSRL_E_INVALID);
        launch_reset<task.value>(seed, indices, count, state, steps, episode, observation_out, rows, randomize_progress != 0,
                                 int32_t(max_steps), N, as_stream(stream));
        return launch_status();
    });
}

extern "C" int cusrl_classic_reset_cpu(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state,
                                       int32_t *steps, int64_t *episode, float *observation_out, int64_t rows, int randomize_progress,
                                       int64_t max_steps, int64_t N) {
    return for_task(kind, [&](auto task) {
        if (int rc = check_reset(indices, state, steps, episode, observation_out, rows, max_steps, N)) return rc;
        for (int64_t k = 0; k < rows; ++k)
            reset_slot<task.value>(k, seed, indices, count, state, steps, episode, observation_out, rows, randomize_progress != 0,
                                   int32_t(max_steps), N);
        return 0;
    });
}
