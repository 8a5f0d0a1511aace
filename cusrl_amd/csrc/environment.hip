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
#include "common.hpp"
#include "philox.hpp"

#include <math.h>

namespace cusrl {
namespace {

template <int kKind>
struct Task;
// (kObservationBytes: the widest access an observation row moves by where it is aligned to it; 4: scalars)
template <>
struct Task<CUSRL_CLASSIC_CARTPOLE> {  // state x, x', theta, theta'; action: logits over {push left, push right}
    static constexpr int kState = 4, kAction = 2, kObservation = 4, kObservationBytes = 16;
};
template <>
struct Task<CUSRL_CLASSIC_PENDULUM> {  // state theta, theta'; action: one torque; observation cos, sin, theta'
    static constexpr int kState = 2, kAction = 1, kObservation = 3, kObservationBytes = 4;
};
template <>
struct Task<CUSRL_CLASSIC_MOUNTAINCAR> {  // state position, velocity; action: logits over {left, none, right}
    static constexpr int kState = 2, kAction = 3, kObservation = 2, kObservationBytes = 8;
};
template <>
struct Task<CUSRL_CLASSIC_ACROBOT> {  // state theta1, theta2, theta1', theta2'; action: logits over torque {-1, 0, +1};
    static constexpr int kState = 4, kAction = 3, kObservation = 6, kObservationBytes = 8;  // observation cos, sin, cos, sin, ', '
};
template <>
struct Task<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS> {  // state position, velocity; action: one force
    static constexpr int kState = 2, kAction = 1, kObservation = 2, kObservationBytes = 8;
};

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

template <int kKind>
__host__ __device__ __forceinline__ void observe(const float *s, float *o) {
    if constexpr (kKind == CUSRL_CLASSIC_PENDULUM) {
        o[0] = cosf(s[0]);
        o[1] = sinf(s[0]);
        o[2] = s[1];
    } else if constexpr (kKind == CUSRL_CLASSIC_ACROBOT) {
        o[0] = cosf(s[0]);
        o[1] = sinf(s[0]);
        o[2] = cosf(s[1]);
        o[3] = sinf(s[1]);
        o[4] = s[2];
        o[5] = s[3];
    } else {
#pragma unroll
        for (int j = 0; j < Task<kKind>::kState; ++j) o[j] = s[j];
    }
}

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
    constexpr float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f;
    if (x > kPi) return x - kTwoPi * ceilf((x - kPi) / kTwoPi);
    if (x < -kPi) return x + kTwoPi * ceilf((-kPi - x) / kTwoPi);
    return x;
}

// One transition of one env: s is advanced in place; returns `terminated`.
template <int kKind>
__host__ __device__ __forceinline__ bool advance(float *s, const float *a, float &reward) {
    if constexpr (kKind == CUSRL_CLASSIC_CARTPOLE) {
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
    } else if constexpr (kKind == CUSRL_CLASSIC_PENDULUM) {
        constexpr float kPi = 3.14159265358979323846f, kTwoPi = 6.28318530717958647692f, kDt = 0.05f;
        const float u = clampf(a[0], -2.0f, 2.0f);
        const float theta = s[0], theta_dot = s[1];
        float wrapped = fmodf(theta + kPi, kTwoPi);  // Python's floor-mod: the sign of the divisor
        if (wrapped < 0.0f) wrapped = wrapped + kTwoPi;
        wrapped = wrapped - kPi;
        reward = -(wrapped * wrapped + 0.1f * (theta_dot * theta_dot) + 0.001f * (u * u));  // of the OLD state
        s[1] = clampf(theta_dot + (15.0f * sinf(theta) + 3.0f * u) * kDt, -8.0f, 8.0f);  // 3g / (2l) = 15, 3 / (m l^2) = 3
        s[0] = theta + s[1] * kDt;
        return false;
    } else if constexpr (kKind == CUSRL_CLASSIC_ACROBOT) {
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
    } else if constexpr (kKind == CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS) {
        const float force = clampf(a[0], -1.0f, 1.0f);
        float position = s[0], velocity = s[1];
        velocity = clampf(velocity + (force * 0.0015f - 0.0025f * cosf(3.0f * position)), -0.07f, 0.07f);
        position = clampf(position + velocity, -1.2f, 0.6f);
        if (position == -1.2f && velocity < 0.0f) velocity = 0.0f;
        s[0] = position;
        s[1] = velocity;
        const bool ended = position >= 0.45f && velocity >= 0.0f;
        reward = (ended ? 100.0f : 0.0f) - 0.1f * (a[0] * a[0]);  // the RAW action, not the clamped force
        return ended;
    } else {
        const int push = first_max<3>(a);
        float position = s[0], velocity = s[1];
        velocity = clampf(velocity + float(push - 1) * 0.001f - 0.0025f * cosf(3.0f * position), -0.07f, 0.07f);
        position = clampf(position + velocity, -1.2f, 0.6f);
        if (position == -1.2f && velocity < 0.0f) velocity = 0.0f;
        s[0] = position;
        s[1] = velocity;
        reward = -1.0f;
        return position >= 0.5f && velocity >= 0.0f;
    }
}

// The state of a fresh episode from one Philox call (documented ranges: include/cusrl_hip.h).
template <int kKind>
__host__ __device__ __forceinline__ void initial_state(const Philox &r, float *s) {
    if constexpr (kKind == CUSRL_CLASSIC_CARTPOLE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = -0.05f + 0.1f * philox_uniform(r.c[j]);
    } else if constexpr (kKind == CUSRL_CLASSIC_PENDULUM) {
        s[0] = -3.14159265358979323846f + 6.28318530717958647692f * philox_uniform(r.c[0]);
        s[1] = -1.0f + 2.0f * philox_uniform(r.c[1]);
    } else if constexpr (kKind == CUSRL_CLASSIC_ACROBOT) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = -0.1f + 0.2f * philox_uniform(r.c[j]);
    } else {  // MountainCar and MountainCarContinuous
        s[0] = -0.6f + 0.2f * philox_uniform(r.c[0]);
        s[1] = 0.0f;
    }
}

// counter = (env id, episode number with the stream in its two top bits), key = seed.  Stream 0: the state, 1: the progress.
__host__ __device__ __forceinline__ Philox episode_draw(uint64_t seed, int64_t env, int64_t episode, uint32_t stream) {
    const uint64_t e = uint64_t(env), n = uint64_t(episode);
    return philox4x32_10(uint32_t(e), uint32_t(e >> 32), uint32_t(n), (uint32_t(n >> 32) & 0x3fffffffu) | (stream << 30), uint32_t(seed),
                         uint32_t(seed >> 32));
}

// ---- one env of the step, rows already in registers: shared by the kernel and cusrl_classic_step_cpu
template <int kKind>
__host__ __device__ __forceinline__ void step_env(float *s, const float *a, int32_t &steps, int32_t max_steps, float *o, float &reward,
                                                  uint8_t &terminated, uint8_t &truncated) {
    const bool ended = advance<kKind>(s, a, reward);
    steps = steps + 1;
    terminated = ended ? 1 : 0;
    truncated = (!ended && steps >= max_steps) ? 1 : 0;
    observe<kKind>(s, o);
}

// ---- env `e` of a reset slot below `count`: s, steps and episode come back holding what to store
template <int kKind>
__host__ __device__ __forceinline__ void reset_env(uint64_t seed, int64_t e, float *s, int32_t &steps, int64_t &episode,
                                                   int randomize_progress, int32_t max_steps) {
    initial_state<kKind>(episode_draw(seed, e, episode, 0u), s);
    steps = 0;
    if (randomize_progress)  // floor(max_steps * word / 2^32): an integer in [0, max_steps)
        steps = int32_t((uint64_t(episode_draw(seed, e, episode, 1u).c[0]) * uint64_t(uint32_t(max_steps))) >> 32);
    episode = episode + 1;
}

// kVec: the state rows (and the observation rows of the tasks whose observation is the state) move as one 16- or 8-byte access,
// Acrobot's 6-wide observation row as three 8-byte ones
template <int kWidth, bool kVec>
__device__ __forceinline__ void load_row(const float *p, float *v) {
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
__device__ __forceinline__ void store_row(float *p, const float *v) {
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
    using T = Task<kKind>;
    const int64_t k = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (k >= rows) return;
    const int64_t live = count ? int64_t(*count) : rows;  // (a count beyond `rows` covers every slot, a negative one none)
    const int64_t e = indices[k];
    float s[T::kState], o[T::kObservation];
    if (e < 0 || e >= N) {  // not an env: nothing is touched, the slot's row is zeros
#pragma unroll
        for (int j = 0; j < T::kObservation; ++j) observation_out[k * T::kObservation + j] = 0.0f;
        return;
    }
    if (k < live) {
        int32_t progress;
        int64_t number = episode[e];
        reset_env<kKind>(seed, e, s, progress, number, randomize_progress, max_steps);
        store_row<T::kState, false>(state + e * T::kState, s);
        steps[e] = progress;
        episode[e] = number;
    } else {
        load_row<T::kState, false>(state + e * T::kState, s);
    }
    observe<kKind>(s, o);
    store_row<T::kObservation, false>(observation_out + k * T::kObservation, o);
}

template <int kKind>
void step_rows_cpu(const float *action, float *state, int32_t *steps, int32_t max_steps, float *next_observation, float *reward,
                   uint8_t *terminated, uint8_t *truncated, int64_t N) {
    using T = Task<kKind>;
    for (int64_t i = 0; i < N; ++i)
        step_env<kKind>(state + i * T::kState, action + i * T::kAction, steps[i], max_steps, next_observation + i * T::kObservation,
                        reward[i], terminated[i], truncated[i]);
}

template <int kKind>
void reset_rows_cpu(uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps, int64_t *episode,
                    float *observation_out, int64_t rows, int randomize_progress, int32_t max_steps, int64_t N) {
    using T = Task<kKind>;
    const int64_t live = count ? int64_t(*count) : rows;
    for (int64_t k = 0; k < rows; ++k) {
        const int64_t e = indices[k];
        if (e < 0 || e >= N) {
            for (int j = 0; j < T::kObservation; ++j) observation_out[k * T::kObservation + j] = 0.0f;
            continue;
        }
        if (k < live) reset_env<kKind>(seed, e, state + e * T::kState, steps[e], episode[e], randomize_progress, max_steps);
        observe<kKind>(state + e * T::kState, observation_out + k * T::kObservation);
    }
}

bool known(int kind) { return kind >= CUSRL_CLASSIC_CARTPOLE && kind <= CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS; }

int check_step(int kind, const void *action, const void *state, const void *steps, int64_t max_steps, const void *next_observation,
               const void *reward, const void *terminated, const void *truncated, int64_t N) {
    if (!known(kind) || N < 0 || max_steps < 1 || max_steps > INT32_MAX) return CUSRL_E_INVALID;
    if (N > 0 && (!action || !state || !steps || !next_observation || !reward || !terminated || !truncated)) return CUSRL_E_INVALID;
    if (N > int64_t(INT32_MAX) * kBlock / 4) return CUSRL_E_UNSUPPORTED;
    return 0;
}

int check_reset(int kind, const void *indices, const void *state, const void *steps, const void *episode, const void *observation_out,
                int64_t rows, int64_t max_steps, int64_t N) {
    if (!known(kind) || N < 0 || rows < 0 || max_steps < 1 || max_steps > INT32_MAX) return CUSRL_E_INVALID;
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

}  // namespace
}  // namespace cusrl

using namespace cusrl;

extern "C" int cusrl_classic_step(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps,
                                  float *next_observation, float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N,
                                  void *stream) {
    if (int rc = check_step(kind, action, state, steps, max_steps, next_observation, reward, terminated, truncated, N)) return rc;
    if (N == 0) return 0;
    if (!aligned(action, 4) || !aligned(state, 4) || !aligned(steps, 4) || !aligned(next_observation, 4) || !aligned(reward, 4))
        return CUSRL_E_INVALID;
    const int32_t limit = int32_t(max_steps);
    switch (kind) {
        case CUSRL_CLASSIC_CARTPOLE:
            launch_step<CUSRL_CLASSIC_CARTPOLE>(action, state, steps, limit, next_observation, reward, terminated, truncated, N, as_stream(stream));
            break;
        case CUSRL_CLASSIC_PENDULUM:
            launch_step<CUSRL_CLASSIC_PENDULUM>(action, state, steps, limit, next_observation, reward, terminated, truncated, N, as_stream(stream));
            break;
        case CUSRL_CLASSIC_MOUNTAINCAR:
            launch_step<CUSRL_CLASSIC_MOUNTAINCAR>(action, state, steps, limit, next_observation, reward, terminated, truncated, N,
                                                   as_stream(stream));
            break;
        case CUSRL_CLASSIC_ACROBOT:
            launch_step<CUSRL_CLASSIC_ACROBOT>(action, state, steps, limit, next_observation, reward, terminated, truncated, N, as_stream(stream));
            break;
        default:
            launch_step<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS>(action, state, steps, limit, next_observation, reward, terminated, truncated, N,
                                                             as_stream(stream));
    }
    return launch_status();
}

extern "C" int cusrl_classic_step_cpu(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps,
                                      float *next_observation, float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N) {
    if (int rc = check_step(kind, action, state, steps, max_steps, next_observation, reward, terminated, truncated, N)) return rc;
    const int32_t limit = int32_t(max_steps);
    switch (kind) {
        case CUSRL_CLASSIC_CARTPOLE:
            step_rows_cpu<CUSRL_CLASSIC_CARTPOLE>(action, state, steps, limit, next_observation, reward, terminated, truncated, N);
            break;
        case CUSRL_CLASSIC_PENDULUM:
            step_rows_cpu<CUSRL_CLASSIC_PENDULUM>(action, state, steps, limit, next_observation, reward, terminated, truncated, N);
            break;
        case CUSRL_CLASSIC_MOUNTAINCAR:
            step_rows_cpu<CUSRL_CLASSIC_MOUNTAINCAR>(action, state, steps, limit, next_observation, reward, terminated, truncated, N);
            break;
        case CUSRL_CLASSIC_ACROBOT:
            step_rows_cpu<CUSRL_CLASSIC_ACROBOT>(action, state, steps, limit, next_observation, reward, terminated, truncated, N);
            break;
        default:
            step_rows_cpu<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS>(action, state, steps, limit, next_observation, reward, terminated, truncated, N);
    }
    return 0;
}

extern "C" int cusrl_classic_reset(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps,
                                   int64_t *episode, float *observation_out, int64_t rows, int randomize_progress, int64_t max_steps,
                                   int64_t N, void *stream) {
    if (int rc = check_reset(kind, indices, state, steps, episode, observation_out, rows, max_steps, N)) return rc;
    if (rows == 0) return 0;
    if (!aligned(indices, 8) || !aligned(episode, 8) || !aligned(state, 4) || !aligned(steps, 4) || !aligned(observation_out, 4) ||
        (count && !aligned(count, 4)))
        return CUSRL_E_INVALID;
    const dim3 grid(uint32_t(ceil_div(rows, kBlock))), block(kBlock);
    const int32_t limit = int32_t(max_steps);
    const int randomize = randomize_progress != 0;
    switch (kind) {
        case CUSRL_CLASSIC_CARTPOLE:
            hipLaunchKernelGGL(classic_reset_kernel<CUSRL_CLASSIC_CARTPOLE>, grid, block, 0, as_stream(stream), seed, indices, count, state,
                               steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_PENDULUM:
            hipLaunchKernelGGL(classic_reset_kernel<CUSRL_CLASSIC_PENDULUM>, grid, block, 0, as_stream(stream), seed, indices, count, state,
                               steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_MOUNTAINCAR:
            hipLaunchKernelGGL(classic_reset_kernel<CUSRL_CLASSIC_MOUNTAINCAR>, grid, block, 0, as_stream(stream), seed, indices, count,
                               state, steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_ACROBOT:
            hipLaunchKernelGGL(classic_reset_kernel<CUSRL_CLASSIC_ACROBOT>, grid, block, 0, as_stream(stream), seed, indices, count, state,
                               steps, episode, observation_out, rows, randomize, limit, N);
            break;
        default:
            hipLaunchKernelGGL(classic_reset_kernel<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS>, grid, block, 0, as_stream(stream), seed, indices,
                               count, state, steps, episode, observation_out, rows, randomize, limit, N);
    }
    return launch_status();
}

extern "C" int cusrl_classic_reset_cpu(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state,
                                       int32_t *steps, int64_t *episode, float *observation_out, int64_t rows, int randomize_progress,
                                       int64_t max_steps, int64_t N) {
    if (int rc = check_reset(kind, indices, state, steps, episode, observation_out, rows, max_steps, N)) return rc;
    const int32_t limit = int32_t(max_steps);
    const int randomize = randomize_progress != 0;
    switch (kind) {
        case CUSRL_CLASSIC_CARTPOLE:
            reset_rows_cpu<CUSRL_CLASSIC_CARTPOLE>(seed, indices, count, state, steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_PENDULUM:
            reset_rows_cpu<CUSRL_CLASSIC_PENDULUM>(seed, indices, count, state, steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_MOUNTAINCAR:
            reset_rows_cpu<CUSRL_CLASSIC_MOUNTAINCAR>(seed, indices, count, state, steps, episode, observation_out, rows, randomize, limit, N);
            break;
        case CUSRL_CLASSIC_ACROBOT:
            reset_rows_cpu<CUSRL_CLASSIC_ACROBOT>(seed, indices, count, state, steps, episode, observation_out, rows, randomize, limit, N);
            break;
        default:
            reset_rows_cpu<CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS>(seed, indices, count, state, steps, episode, observation_out, rows, randomize,
                                                                limit, N);
    }
    return 0;
}
