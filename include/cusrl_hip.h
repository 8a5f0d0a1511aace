/*
 * cusrl_hip.h — C ABI of libcusrl_hip.so: the MI355X (gfx950) rollout + PPO-update hot path.
 *
 * Drop-in boundary.  The reference (chengruiz/cusrl) has no FFI: its hot path is
 * chains of PyTorch ops behind a Python plugin API (Buffer / Sampler / Hook).  Each entry point below
 * replaces the torch-op chain of ONE reference function, cited as file:line relative to the
 * reference repo root; the Python host (cusrl_amd/) keeps the reference's class and method names
 * and binds these symbols with ctypes (INTEGRATION.md shows the binding a cusrl maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked "host";
 *   - the caller owns all memory (no allocation, no hidden synchronisation, no host<->device copies);
 *   - every launch goes to `stream` (a hipStream_t passed as void*; NULL = the null stream);
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative CUSRL_E_* code;
 *   - tensors are contiguous, row-major, fp32 unless stated; flags are 1-byte bools;
 *   - layouts follow the reference Buffer: a leaf is [T, N, C] (capacity, parallelism, channels),
 *     a "slot" is one (t, n) pair, its flat index is t * N + n (buffer.py:124-151).
 */
#ifndef CUSRL_HIP_H
#define CUSRL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CUSRL_ABI_VERSION 7
#define CUSRL_MAX_FIELDS 24 /* leaves per push / gather launch; larger tables are split by the host */
#define CUSRL_MAX_PACKED 16 /* 1-8 byte entries of the per-slot record (cusrl_pack_rows); wide fields count as leaves */
#define CUSRL_MAX_RECORD_BYTES 1024
#define CUSRL_MAX_MIRROR_FIELDS 24 /* fields per cusrl_mirror_rows launch */
#define CUSRL_MAX_SYMMETRIZE_CHANNELS 4096 /* channels of cusrl_symmetrize_mean_var (one workgroup, LDS-staged) */
#define CUSRL_MAX_SYMMETRIC_HEAD_ACTIONS 64 /* widest action row of the cusrl_symmetric_head_* entries */

#define CUSRL_E_INVALID (-1)     /* NULL pointer, negative size, inconsistent arguments */
#define CUSRL_E_TOO_MANY (-2)    /* n_fields > CUSRL_MAX_FIELDS */
#define CUSRL_E_UNSUPPORTED (-3) /* shape outside what the kernels handle */
#define CUSRL_E_COMM (-4)        /* RCCL unavailable or an RCCL call failed: see cusrl_comm_last_error() */

/* One leaf of a multi-leaf copy.  `row_bytes` = bytes of one slot (C * element size). */
typedef struct {
    const void *src;
    void *dst;
    int64_t row_bytes;
} cusrl_field_t;

int cusrl_abi_version(void);
/* Human-readable text for a return code (host string, static storage). */
const char *cusrl_error_string(int code);

/* Launch-shape and cache-policy overrides (ABI 6).  Every kernel chooses its launch shape and cache policy by a measured rule
 * of its own (footprint against the 256 MB Infinity Cache, rows per block); these exist for A/B measurements and sweeps.  Up
 * to ABI 5 the library read them from CUSRL_* environment variables inside the launch entry points — invisible to a caller
 * binding this header; now they are part of it, and the only environment variable the library itself reads is
 * CUSRL_RCCL_LIBRARY (where to find RCCL, cusrl_comm_*).  value 0 = back to the kernel's own rule.
 *   "gae_policy"    1 + {0, 5, 7}: cache policy of cusrl_gae's scan (bit 0 non-temporal loads, bit 1 `advantage`, bit 2 `return`)
 *   "gae_block"     128 | 256 threads per block of the scan
 *   "loss_policy"   1 default policy | 2 non-temporal [B, A] streams in cusrl_ppo_loss_fwd_bwd
 *   "push_policy"   1 default policy | 2 streaming in cusrl_buffer_push*
 *   "colsum_rows"   rows per block of cusrl_relu_bwd_colsum (4 .. 4096)
 *   "head_rows"     rows per block of cusrl_narrow_linear_bwd (8 .. 4096)
 *   "gru_bias_rows" rows per partial row of cusrl_gru_gates_bwd_bias (4 | 8 | 16 | 32)
 * Returns 0, CUSRL_E_INVALID for an unknown key, CUSRL_E_UNSUPPORTED for a value outside the list.  Host-side, thread-safe
 * (relaxed atomics); takes effect at the next launch.  Every setting changes how bytes move, never a result bit
 * (tests/test_hip_kernels.py: *_every_cache_policy_*, *_cache_policies_change_no_bit). */
int cusrl_set_option(const char *key, int64_t value);
int cusrl_get_option(const char *key, int64_t *value_out);

/* Node census of a captured hipGraph (`graph` = hipGraph_t): a host-side walk, no launch, no stream.  The reference's
 * `compile=True` (cusrl/template/actor_critic.py:217-220) hands its loops to torch.compile; here they are hipGraphs, and
 * what a captured step is made of is checkable: type_counts[k] (HOST, n_types entries) = number of nodes of
 * hipGraphNodeType k (0 kernel, 1 memcpy, 2 memset, ...); `names` (HOST, `capacity` bytes, may be NULL with capacity 0)
 * receives the mangled names of the kernel nodes in node order, '\n'-terminated, truncated at capacity;
 * *names_len = bytes the full list needs.  The host (template/graphs.py `_Capture.capture`) walks every captured region with
 * this before it instantiates it and rewrites the region's memset nodes (cusrl_graph_replace_memsets below: they do not
 * replay reliably on this stack); ATen global-reduce kernels are allowed (their semaphore memsets are what gets rewritten),
 * the tests assert that the stock compositions contain none. */
int cusrl_graph_census(void *graph, int64_t *type_counts, int n_types, char *names, int64_t capacity, int64_t *names_len);

/* Replace every memset node of a captured, not yet instantiated hipGraph by a kernel node (a plain fill kernel) with the
 * same destination, value, extent and edges; *replaced_out (HOST, may be NULL) = how many.  Host-side graph surgery, no
 * launch.  What torch.compile does for the reference's `compile=True` (cusrl/template/hook.py:396-399) is a hipGraph here,
 * and the ROCm 7.0 runtime of PyTorch 2.10 does not replay memset nodes reliably (scripts/probe_aten_reduce_capture.py:
 * ATen's split reductions zero their semaphores with hipMemsetAsync, Reduce.cuh:1294-1301) — a captured region is only
 * instantiated once it has none.  CUSRL_E_UNSUPPORTED: a memset node with an element size other than 1 / 2 / 4. */
int cusrl_graph_replace_memsets(void *graph, int64_t *replaced_out);

/* ---- a1  Buffer.push — cusrl/template/buffer.py:124-151 (`storage[cursor] = value` per leaf) ----
 * fields[i].src = step leaf [N, row_bytes];  fields[i].dst = storage leaf base [T, N, row_bytes].
 * Copies every leaf's step into slot row `cursor` in ONE launch.  `fields` is a HOST array. */
int cusrl_buffer_push(const cusrl_field_t *fields, int n_fields, int64_t cursor, int64_t N, void *stream);

/* The same append with WRITE-THROUGH into the per-slot record of cusrl_pack_rows / cusrl_gather_rows_packed (below):
 * record_offset[i] >= 0 (n_fields HOST entries): leaf i also lives in the record at that byte offset, and its step row n
 * is additionally stored at record[(cursor * N + n) * record_bytes + record_offset[i]] from the registers that already
 * hold it; -1: the leaf is not in the record.  Only whole 16-byte chunks are written through (row_bytes and the offset
 * multiples of 16, 16-byte aligned pointers: the wide leaves — observation, action); narrow leaves are produced or
 * edited at update time anyway and keep going through cusrl_pack_rows.  With this the once-per-update pack of the
 * `ppo` record moves 13 instead of 253 bytes per slot. */
int cusrl_buffer_push_through(const cusrl_field_t *fields, int n_fields, int64_t cursor, int64_t N, void *record,
                              int64_t record_bytes, const int32_t *record_offset, void *stream);

/* ---- a3  ValueComputation.pre_update — cusrl/hook/on_policy/value.py:56-82 ----
 * next_value[:-1] = value[1:]; next_value[-1] = last_value [N,D]; next_value[terminated] = termination_value;
 * truncated slots: mode 0 = left for the caller to bootstrap (value.py:72-78), mode 1 = value[truncated]
 * (value.py:79-80).  Also counts truncated slots per block into `block_counts`
 * (cusrl_flag_blocks(T*N) int32 entries) for cusrl_compact_flags. */
int cusrl_next_value(const float *value, const uint8_t *terminated, const uint8_t *truncated,
                     const float *last_value, float termination_value, int truncated_mode, float *next_value,
                     int32_t *block_counts, int64_t T, int64_t N, int64_t D, void *stream);

/* Number of per-block counters cusrl_next_value / cusrl_compact_flags use for `n` flags. */
int64_t cusrl_flag_blocks(int64_t n);

/* Ordered stream compaction of a flag array (replaces `next_state[truncated]` boolean-mask indexing,
 * value.py:75): indices_out[0..count) = ascending flat slots with flags != 0, *count_out = count.
 * `block_counts` must have been filled by cusrl_next_value over the same flags, or pass recount != 0
 * to have this call count first.  `count_out` is written with a system-scope store and may point to pinned host
 * memory (device-mapped): the host can then poll it instead of a device->host copy + stream synchronisation (the
 * trainer's per-step read of the finished-env count, trainer.py:365-372). */
int cusrl_compact_flags(const uint8_t *flags, int64_t n, int32_t *block_counts, int recount,
                        int64_t *indices_out, int32_t *count_out, void *stream);

/* dst[indices[k], :] = src[k, :] for k < K (row_bytes per row): `next_value[truncated] = critic(...)`,
 * value.py:78.  If count_dev != NULL the effective K is min(K, *count_dev) read on the device. */
int cusrl_scatter_rows(const void *src, const int64_t *indices, void *dst, int64_t K, int64_t row_bytes,
                       const int32_t *count_dev, void *stream);

/* ---- the next act input of a vectorised rollout — cusrl/template/environment.py:365-379 (`update_observation_and_state`:
 * `last_observation[indices] = init_observation`) fused with the copy into the act step's input buffer ----
 * dst[n] = src[n] for every env n with done[n] == 0, and dst[indices[k]] = init[k] for k < min(N, *count_dev): `done`
 * [N] and (indices, count_dev) must describe the same set of finished envs (cusrl_step_epilogue emits both), src / init
 * / dst are [N, row_bytes] with dst distinct from src and init; the count is read by the kernel (device or pinned host
 * memory), so a captured env step needs no host read to reset its finished envs. */
int cusrl_splice_rows(const void *src, const void *init, const int64_t *indices, const int32_t *count_dev,
                      const uint8_t *done, void *dst, int64_t N, int64_t row_bytes, void *stream);

/* ---- a4  GAE(lambda) + return — cusrl/hook/on_policy/gae.py:8-20, 85-110 ----
 * delta = (r + nv*gamma) - v;  A[T-1] = delta;  A[t] = delta[t] + ((done[t] ? 0 : gamma*lamda) * A[t+1])
 * (separate multiply and add, bit-exact with the reference);  ret = value + A, or value + A' where A' is the
 * same scan with lamda_value when lamda_value >= 0 (pass < 0 for None).  done is [T,N,1].
 * stat_partials (optional): [cusrl_gae_num_partials(T,N,D)] rows of {sum, sumsq} per channel, i.e.
 * double[num_partials][D][2], of the advantage — consumed by cusrl_stats_finalize (fuses the statistics
 * pass of advantage.py:111 into the scan). */
int cusrl_gae(const float *reward, const float *value, const float *next_value, const uint8_t *done,
              float *advantage, float *ret, double *stat_partials, int64_t T, int64_t N, int64_t D,
              double gamma, double lamda, double lamda_value, void *stream);
int64_t cusrl_gae_num_partials(int64_t T, int64_t N, int64_t D);

/* ---- a5  AdvantageNormalization.normalize_ — cusrl/hook/on_policy/advantage.py:108-115 ----
 * Column statistics of x [rows, D] as per-block {sum, sumsq} partials (double[num_partials][D][2]). */
int cusrl_col_stats(const float *x, int64_t rows, int64_t D, double *stat_partials, void *stream);
int64_t cusrl_col_stats_num_partials(int64_t rows, int64_t D);
/* mean[d], var[d] (unbiased, correction = 1, like torch.var_mean) from partials, fixed summation order.  mean and var may be the
 * halves of ONE float[2 D] row (var = mean + D): what a cross-rank merge all-gathers (cusrl_normalize_from_gathered). */
int cusrl_stats_finalize(const double *stat_partials, int64_t num_partials, int64_t D, int64_t count,
                         float *mean, float *var, void *stream);
/* x = (x - mean) / sqrt(var + eps) in place, true division (advantage.py:114-115). */
int cusrl_normalize(float *x, const float *mean, const float *var, float eps, int64_t rows, int64_t D,
                    void *stream);

/* The two steps above in ONE launch for the single-process case (no cross-rank merge between statistics and their
 * use): every block reduces the partial rows itself (same fixed order), then normalises its share of x; mean_out /
 * var_out [D] receive the statistics (block 0).  Bit-identical to cusrl_stats_finalize + cusrl_normalize. */
int cusrl_normalize_from_partials(float *x, const double *stat_partials, int64_t num_partials, int64_t count, float eps,
                                  int64_t rows, int64_t D, float *mean_out, float *var_out, void *stream);

/* ---- a6  reduce_mean_var_ merge — cusrl/utils/distributed.py:175-183 ----
 * gathered = [W, 2*D] rows of cat(mean_r, var_r) (the all_gather result); writes the equal-weight merge
 * mean = avg_r mean_r, var = avg_r (var_r + (mean_r - mean)^2) into mean[D], var[D]. */
int cusrl_merge_mean_var(const float *gathered, int64_t W, int64_t D, float *mean, float *var, void *stream);

/* cusrl_merge_mean_var + cusrl_normalize as ONE launch (ABI 6, second part of round 6): the advantage normalisation of a job with
 * several ranks (hook/on_policy/advantage.py:108-115 with `reduce_mean_var_`, distributed.py:175-183, between the statistics and
 * their use).  gathered: float[W][2 D], every rank's mean | var (cusrl_stats_finalize writes both into one [2 D] row, which
 * cusrl_allgather collects); every block re-derives the merged statistics — the same operations in the same order as
 * cusrl_merge_mean_var — and normalises its share of x [rows, D] in place; mean_out / var_out [D] receive the merged statistics.
 * Bit-identical to cusrl_merge_mean_var + cusrl_normalize.  D <= 256. */
int cusrl_normalize_from_gathered(float *x, const float *gathered, int64_t W, float eps, int64_t rows, int64_t D,
                                  float *mean_out, float *var_out, void *stream);

/* ---- a7/a8  minibatch gather — cusrl/sampler/mini_batch_sampler.py:87-89, 113-114; buffer.py:153-162 ----
 * For every leaf i: temporal == 0:  dst_i[b]       = src_i.flatten(0,1)[indices[b]]      b < B
 *                   temporal != 0:  dst_i[t, b]    = src_i[t, indices[b]]                t < T, b < B
 * All leaves in ONE launch; `fields` is a HOST array; indices are int64 (torch.randperm's dtype). */
int cusrl_gather_rows(const cusrl_field_t *fields, int n_fields, const int64_t *indices, int64_t B, int64_t T,
                      int64_t N, int temporal, void *stream);

/* ---- a7/a8 with the narrow leaves packed — same reference lines, different byte traffic ----
 * A minibatch row of a 1-8 byte leaf (action_logp, value, reward, next_value, advantage, return, the three flags of
 * the `ppo` buffer) costs one memory sector per leaf when fetched from a random slot.  cusrl_pack_rows interleaves
 * such leaves ONCE per update into one record per slot — record[s] = { field_0[s], field_1[s], ... } at the given
 * byte offsets, record_bytes a multiple of 16 up to CUSRL_MAX_RECORD_BYTES, `record` 16-byte aligned — and
 * cusrl_gather_rows_packed gathers the plain leaves as cusrl_gather_rows does plus, for every sampled slot, ONE record
 * read fanned out to the separate contiguous batch tensors (dst_k[b] = field_k of record[slot(b)]): identical results.
 * Wide leaves (a multiple of 16 bytes per slot: observation, action) may live in the record as well: when the record
 * holds exactly what a training step reads (253 B for the `ppo` preset -> 256 B, two 128-byte memory lines), a sampled
 * slot costs 256 fetched bytes instead of ~550 (measured 128 B per random row of ANY size <= 128 B on MI355X:
 * profiles/r02/pmc_summary.json).  The host keeps the record valid (rebuilds it after any write to a packed leaf). */
typedef struct {
    void *ptr;      /* pack: source leaf base [rows, width] (read only); gather: destination base [B or T*B, width] */
    int32_t offset; /* byte offset of the field inside the record; a multiple of min(width, 16) */
    int32_t width;  /* 1, 2, 4, 8 bytes, or any multiple of 16 (wide field) */
} cusrl_packed_field_t;
int cusrl_pack_rows(const cusrl_packed_field_t *fields, int n_fields, void *record, int64_t record_bytes,
                    int64_t rows, void *stream);
/* cusrl_pack_rows where the caller owns `owned_chunks` (1 or 2) whole 16-byte chunks of every record, starting at chunk
 * `owned_first_chunk`: every narrow field of the call lies inside them and nothing else lives there (no other leaf of
 * the record, no wide field).  The narrow fields then leave as ONE 16-byte store per chunk instead of one 1-4 byte store
 * per field (bytes of the owned chunks no field covers become zero).  The update-time leaves of the `ppo` hot record
 * (action_logp, advantage, return, done: 13 bytes in the record's last chunk) are the case it is there for. */
int cusrl_pack_rows_owned(const cusrl_packed_field_t *fields, int n_fields, void *record, int64_t record_bytes,
                          int64_t rows, int32_t owned_first_chunk, int32_t owned_chunks, void *stream);
int cusrl_gather_rows_packed(const cusrl_field_t *fields, int n_fields, const void *record, int64_t record_bytes,
                             const cusrl_packed_field_t *packed, int n_packed, const int64_t *indices, int64_t B,
                             int64_t T, int64_t N, int temporal, void *stream);

/* ---- random temporal windows — cusrl/sampler/random_sampler.py:95-113 (`TemporalRandomSampler`) ----
 * out[t * B + b] = ((cursor + start[b] + t) % T) * N + env[b] for t < L, b < B: the flat slots of B windows of L
 * consecutive steps, window b belonging to env[b] and starting at LOGICAL step start[b] (physical row `cursor` is
 * logical step 0 of a full ring; pass cursor = 0 while the ring is still filling).  The list feeds cusrl_gather_rows
 * (temporal = 0, B' = L * B) — `data[time_indices, env_indices]` of the reference for every leaf in one launch. */
int cusrl_window_indices(const int64_t *start, const int64_t *env, int64_t *out, int64_t B, int64_t L, int64_t T,
                         int64_t N, int64_t cursor, void *stream);

/* ---- a9-a13  PPO objective, forward + backward ----
 * common.py:29-43 (Normal log-prob / entropy / ratio), ppo.py:10-18,50-55 (clipped surrogate),
 * value.py:85-89,121-137 (MSE or clipped value loss), ppo.py:82-84 (entropy bonus),
 * actor_critic.py:309 (sum).  Shapes: advantage, old_logp [B,1]; action, mean, std [B,A];
 * ret, curr_value, old_value [B,D] (old_value may be NULL when value_clip < 0 = None).
 * Outputs: losses_out[7] = {value_loss, surrogate_loss, entropy_loss} (already weighted), the three per-minibatch
 * metrics the hooks record — mean |logp ratio|, mean entropy, mean curr_value.sum(-1) — and the total loss
 * (value + surrogate) + entropy that the agent differentiates (actor_critic.py:309);
 * logp_out, entropy_out, logp_ratio_out, ratio_out [B] (each optional);
 * d_mean, d_std [B,A], d_value [B,D] = d(value_loss + surrogate_loss + entropy_loss)/d(.) .
 * partials: double[cusrl_ppo_loss_num_partials(B)][5] workspace.
 * std_rows = B: `std` is the [B,A] matrix of the reference's repeated std vector (distribution.py:228-247);
 * std_rows = 1: `std` is that vector itself, [A] — it is broadcast inside the kernel and d_std is the gradient of the
 * vector, [A] (= the column sums a sum(0) over [B,A] would give); needs A % 4 == 0, A <= 32 and the workspace
 * d_std_partials: float[cusrl_ppo_loss_std_partial_rows(B)][A] (may be NULL otherwise).
 * flags: 0, or CUSRL_LOSS_DEFER — ONE launch, no finalize: nothing inside an optimizer step consumes the loss VALUES
 * (actor_critic.py:311-312 differentiates them with a unit gradient; the values only feed the metrics read once per
 * update), so the caller may own the reductions instead of paying a one-block launch per minibatch step:
 *   - every block ADDS its five partial sums {sum sq. value error, sum min(..) surrogate, sum entropy, sum |logp ratio|,
 *     sum value} to ITS row of `partials` (cusrl_ppo_loss_blocks(B, A) rows; zero-fill once): launches of the same
 *     shape on one stream build running sums in a fixed order, the caller forms the means whenever it reads them;
 *   - with a std vector every block leaves its [A] column sums of d_std in its row of d_std_partials — exactly the
 *     "partial rows" form cusrl_assemble_gradients reduces into the parameter's slot (row_stride = A);
 *   - losses_out and (std vector) d_std are not written and may be NULL. */
#define CUSRL_LOSS_DEFER 1
int cusrl_ppo_loss_fwd_bwd(const float *advantage, const float *old_logp, const float *action, const float *mean,
                           const float *std, const float *ret, const float *curr_value, const float *old_value,
                           int64_t B, int64_t A, int64_t D, double clip, double value_clip, double w_sur,
                           double w_val, double w_ent, float *losses_out, float *logp_out, float *entropy_out,
                           float *logp_ratio_out, float *ratio_out, float *d_mean, float *d_std, float *d_value,
                           double *partials, int64_t std_rows, float *d_std_partials, int flags, void *stream);
/* workspace rows (enough for any action width) and the exact number of blocks = partial rows of one launch
 * (A = 0: the categorical form) */
int64_t cusrl_ppo_loss_num_partials(int64_t B);
int64_t cusrl_ppo_loss_std_partial_rows(int64_t B);
int64_t cusrl_ppo_loss_blocks(int64_t B, int64_t A);

/* D == 0 in cusrl_ppo_loss_fwd_bwd / cusrl_ppo_loss_categorical_fwd_bwd (ABI 6): the launch carries NO value term — ret,
 * curr_value, old_value, d_value may be NULL, losses_out[0] = losses_out[5] = 0 and losses_out[6] = surrogate + entropy.
 * The value term then comes from the launch below.
 *
 * ValueLoss.objective on its own — cusrl/hook/on_policy/value.py:121-137 (`mse_loss(return, curr_value) * weight`) and the
 * clipped form `_clipped_value_loss` value.py:85-89 — forward AND backward in one pass over ret / curr_value / old_value
 * [B, D]: d_value [B, D] = d(value_loss)/d(curr_value) (optional), losses_out[0] = the weighted loss, losses_out[1] = mean of
 * curr_value.sum(-1) (the `value` metric, value.py:139-141).  The sum `value + surrogate + entropy` the agent differentiates
 * with a unit gradient (cusrl/template/actor_critic.py:309-312) splits into its summands; the host evaluates this one on the
 * stream the critic runs on, so that critic forward -> value term -> critic backward is one branch of the captured
 * minibatch step.  Same per-element arithmetic as the one-launch objective (d_value bit-identical).
 * partials: double[cusrl_value_loss_blocks(B, D)][2]; flags: 0 or CUSRL_LOSS_DEFER (every block ADDS {sum sq. error, sum value}
 * to its row; losses_out may be NULL). */
int cusrl_value_loss_fwd_bwd(const float *ret, const float *curr_value, const float *old_value, int64_t B, int64_t D,
                             double value_clip, double w_val, float *losses_out, float *d_value, double *partials, int flags,
                             void *stream);
int64_t cusrl_value_loss_blocks(int64_t B, int64_t D);

/* The same objective for one-hot categorical policies (discrete action spaces) —
 * cusrl/nn/module/distribution.py:332-366 over torch.distributions.OneHotCategorical: action [B,A] one-hot (the taken
 * action is its first arg-max), logits [B,A] unnormalised; logp = log_softmax(logits)[taken],
 * entropy = -sum_j p_j log p_j, ratio / surrogate / value / entropy terms and losses_out[7] exactly as above;
 * d_logits [B,A], d_value [B,D] = d(total loss)/d(.).  partials: double[cusrl_ppo_loss_num_partials(B)][5];
 * flags as above (CUSRL_LOSS_DEFER: block rows accumulate into `partials`, cusrl_ppo_loss_blocks(B, 0) of them;
 * a masked action's logit may be -inf: p = 0 and, as in torch.distributions.Categorical.entropy, its log p is clamped to
 * the smallest finite float before the product, so every output of the row stays finite and its d_logits is 0). */
int cusrl_ppo_loss_categorical_fwd_bwd(const float *advantage, const float *old_logp, const float *action,
                                       const float *logits, const float *ret, const float *curr_value,
                                       const float *old_value, int64_t B, int64_t A, int64_t D, double clip,
                                       double value_clip, double w_sur, double w_val, double w_ent, float *losses_out,
                                       float *logp_out, float *entropy_out, float *logp_ratio_out, float *ratio_out,
                                       float *d_logits, float *d_value, double *partials, int flags, void *stream);

/* ---- §8f row 1: GRU time step (torch.nn.GRU, the recurrent backbone of cusrl/nn/module/rnn.py:21-120) ----
 * One pass over the gates of one time step, between the rocBLAS GEMMs that produce gi = W_ih x + b_ih [B, 3H] (all steps
 * at once) and gh = W_hh h [B, 3H] (per step):
 *   r = sigmoid(gi_r + gh_r + b_hr); z = sigmoid(gi_z + gh_z + b_hz); n = tanh(gi_n + r * (gh_n + b_hn));
 *   h <- (1 - z) * n + z * h (in place); out = h.           b_hh may be NULL (bias=False).
 * lengths (int64[B], may be NULL): a sequence with t >= lengths[b] keeps h, emits out = 0 (the semantics of a
 * PackedSequence, cusrl/nn/module/rnn.py:273-291, without packing or a host read of the lengths).
 * cusrl_gru_gates_bwd consumes the saved pre-activations IN PLACE: gi <- dL/dgi, gh <- dL/dgh, and
 * dh <- (dh + d_out) * z, the direct path to h_{t-1} (the caller adds dL/dgh @ W_hh); d_out may be NULL; ended
 * sequences get zero gate gradients and leave dh untouched. */
int cusrl_gru_gates_fwd(const float *gi, const float *gh, const float *b_hh, float *h, float *out,
                        const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream);
int cusrl_gru_gates_bwd(float *gi, float *gh, const float *b_hh, const float *h_prev, const float *d_out, float *dh,
                        const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream);
/* cusrl_gru_gates_bwd with the bias gradients folded in: every block of 16 rows also leaves the column sums of what it
 * wrote, bias_partials[block][4H] = {sum d_r, sum d_z, sum d_n, sum d_q} (block = row / 16, cusrl_gru_bias_partial_rows(B)
 * rows); summed over all blocks and steps, d b_ih = {r, z, n} and d b_hh = {r, z, q} — instead of two column-sum passes
 * over the [L * B, 3H] gradient arrays.  Needs H / 4 (H for unaligned rows) to divide 256; CUSRL_E_UNSUPPORTED otherwise. */
int cusrl_gru_gates_bwd_bias(float *gi, float *gh, const float *b_hh, const float *h_prev, const float *d_out, float *dh,
                             const int64_t *lengths, int64_t t, int64_t B, int64_t H, float *bias_partials, void *stream);
int64_t cusrl_gru_bias_partial_rows(int64_t B);
/* 1 when cusrl_gru_gates_bwd_bias accepts a launch with this hidden size and these (device) pointers — alignment and the
 * column-chunk tiling decide — 0 when it would return CUSRL_E_UNSUPPORTED: the host asks instead of restating the rule. */
int cusrl_gru_bias_supported(int64_t H, const float *gi, const float *gh, const float *b_hh, const float *h_prev,
                             const float *d_out, const float *dh, const float *bias_partials);

/* The same for torch.nn.LSTM (gate order i, f, g, o), the default core of RecurrentPpoAgentFactory (cusrl/preset/ppo.py:189):
 *   pre = gi + gh + b_hh; c <- sigmoid(pre_f) * c + sigmoid(pre_i) * tanh(pre_g); h <- sigmoid(pre_o) * tanh(c); out = h.
 * With c_saved != NULL (training) the new cell state is also stored there and `pre` is written over gi — both biases are
 * additive, so d(pre) is the gradient of gi and of gh alike.  cusrl_lstm_gates_bwd: pre <- dL/dpre in place,
 * dc <- dL/dc_{t-1}, dh <- the part of the state gradient that bypasses the step (everything for an ended sequence,
 * zero otherwise; the caller adds dL/dpre @ W_hh).  c_prev / c_next: cell state before / after the step. */
int cusrl_lstm_gates_fwd(float *gi, const float *gh, const float *b_hh, float *h, float *c, float *out, float *c_saved,
                         const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream);
int cusrl_lstm_gates_bwd(float *pre, const float *c_prev, const float *c_next, const float *d_out, float *dh, float *dc,
                         const int64_t *lengths, int64_t t, int64_t B, int64_t H, void *stream);

/* ... and for torch.nn.RNN (relu != 0: ReLU, else tanh): h <- act(gi + gh + b_hh), out = h.  The output is the only
 * saved state (act' is a function of it); cusrl_rnn_cell_bwd writes dL/dpre = (dh + d_out) * act'(out) into d_pre (the
 * caller passes the gi slice) and leaves in dh what bypasses the step, as the LSTM form does. */
int cusrl_rnn_cell_fwd(const float *gi, const float *gh, const float *b_hh, float *h, float *out, const int64_t *lengths,
                       int64_t t, int64_t B, int64_t H, int relu, void *stream);
int cusrl_rnn_cell_bwd(float *d_pre, const float *out, const float *d_out, float *dh, const int64_t *lengths, int64_t t,
                       int64_t B, int64_t H, int relu, void *stream);

/* ---- rollout-side: sampling and episode statistics ----
 * Normal sample + log-prob of the sample in one pass — cusrl/nn/module/distribution.py:198-205 (`rsample`, then
 * `log_prob(sample).sum(-1, keepdim)`): action = mean + eps * std with eps ~ N(0,1) supplied by the caller (drawn
 * from torch's generator so the random stream is the reference's); logp[B] as in cusrl_ppo_loss_fwd_bwd.
 * std_rows = B: std [B,A]; std_rows = 1: std is the [A] vector a state-independent std repeats for every row
 * (distribution.py:228-247, `param.repeat(B, 1)`) — broadcast inside the kernel, and std_out [B,A] (optional) receives
 * the repeated matrix the rollout buffer stores as a leaf, so the acting path needs no `repeat` launch.
 * mean_bias [A] + mean_out [B,A] (both or neither): `mean` is the policy head's product WITHOUT its bias
 * (`latent @ W^T`, distribution.py:195-197 `mean_head`); the bias is added here and the finished mean written to
 * mean_out — the library adds a 12-column bias by broadcasting it into the output with a copy launch before the GEMM. */
int cusrl_normal_sample_logp(const float *mean, const float *std, const float *eps, float *action, float *logp,
                             int64_t B, int64_t A, int64_t std_rows, float *std_out, const float *mean_bias,
                             float *mean_out, void *stream);

/* One-hot categorical sample + its log-prob in one pass — cusrl/nn/module/distribution.py:332-366
 * (`OneHotCategorical(logits).sample()`, `log_prob(sample)`): idx = argmax_j softmax(logits)_j / noise_j with
 * noise ~ Exp(1) supplied by the caller from torch's generator (the way torch.multinomial draws one sample on the
 * device); action[B, A] = one_hot(idx), logp[B] = logits[idx] - logsumexp(logits).  Ties go to the lower index. */
int cusrl_categorical_sample_logp(const float *logits, const float *noise, float *action, float *logp, int64_t B,
                                  int64_t A, void *stream);

/* EnvironmentStats.track_step + track_episode — cusrl/template/trainer.py:54-76, in one launch and without the
 * host round trip of `get_done_indices(...).tolist()` (environment.py:356-362):
 *   episode_rew[n] += reward[n]; episode_len[n] += 1; step_reward_sum[d] += sum_n reward[n,d];
 *   for done[n], in ASCENDING n: slot = (num_episodes++) % R; ring_rew[slot] = episode_rew[n];
 *                ring_len[slot] = episode_len[n]; episode_rew[n] = 0; episode_len[n] = 0.
 * reward, episode_rew [N,D]; done [N] bytes; episode_len [N]; ring_rew [R,D]; ring_len [R];
 * num_episodes: device uint64[2], double-buffered — the launch reads num_episodes[parity] and leaves the updated count
 * in num_episodes[parity ^ 1]; the caller flips `parity` (0 / 1) every call; step_reward_sum: device double[D].
 * (Beyond 262 144 envs slots are drawn by atomic ticket: same set of slots, unspecified order within the step.) */
int cusrl_episode_stats(const float *reward, const uint8_t *done, float *episode_rew, float *episode_len,
                        float *ring_rew, float *ring_len, uint64_t *num_episodes, double *step_reward_sum,
                        int64_t N, int64_t D, int64_t R, int parity, void *stream);

/* The whole per-env-step epilogue of the rollout loop in ONE launch (cusrl/template/actor_critic.py:277,
 * cusrl/template/trainer.py:300-313, cusrl/template/environment.py:356-362):
 *   done_out[n] = terminated[n] | truncated[n];   episode statistics exactly as cusrl_episode_stats with that flag;
 *   indices_out[0 .. count) = the finished envs in ascending order (`get_done_indices`), *count_out = their number.
 * count_out is written with a system-scope store and may be pinned host memory: the host launches this right after
 * env.step, runs agent.step (hooks, buffer push) meanwhile, and finds the count waiting instead of blocking on a
 * device->host copy.  Needs N <= cusrl_step_epilogue_max_envs(). */
int cusrl_step_epilogue(const float *reward, const uint8_t *terminated, const uint8_t *truncated, uint8_t *done_out,
                        float *episode_rew, float *episode_len, float *ring_rew, float *ring_len, uint64_t *num_episodes,
                        double *step_reward_sum, int64_t *indices_out, int32_t *count_out, int64_t N, int64_t D, int64_t R,
                        int parity, void *stream);
int64_t cusrl_step_epilogue_max_envs(void);
/* cusrl_step_epilogue AND cusrl_buffer_push of the same env step as ONE launch (actor_critic.py:273-282 + trainer.py:296-321):
 * the epilogue blocks store `done` both to done_out and straight into the buffer's slab of fields[done_field] (whose src
 * is ignored); every other field is appended as by cusrl_buffer_push.  For steps whose post_step hooks do no device
 * work between the two (nothing may read the flag or edit the reward in between). */
int cusrl_step_epilogue_push(const float *reward, const uint8_t *terminated, const uint8_t *truncated, uint8_t *done_out,
                             float *episode_rew, float *episode_len, float *ring_rew, float *ring_len, uint64_t *num_episodes,
                             double *step_reward_sum, int64_t *indices_out, int32_t *count_out, int64_t N, int64_t D, int64_t R,
                             int parity, const cusrl_field_t *fields, int n_fields, int done_field, int64_t cursor,
                             void *stream);

/* cusrl_step_epilogue for the PLAY loop (cusrl/template/player.py:228-247; additive entry of ABI 7): everything
 * cusrl_step_epilogue does — the same device code, same results — and in the same launch
 *   episode_count[n] += (terminated[n] | truncated[n])           (player.py:269, int64 [N], device, in place)
 *   *unfinished_out = #{n : episode_count[n] < target_episodes}   (player.py:246 — 0 ends the loop)
 * unfinished_out: one int32 on the device or in pinned host memory, written once with a system-scope release store.
 * workspace: cusrl_play_epilogue_workspace_words() uint32 words on the device, zeroed ONCE by the caller when allocated: the
 * launch leaves them zero again (the block that draws the last ticket takes the integer total and resets both words), so
 * consecutive launches on one stream need no preparation — no memset, no second kernel, no synchronisation.
 * CUSRL_E_INVALID, nothing launched: a NULL pointer, N, D or R < 1, parity outside {0, 1}, target_episodes < 1;
 * CUSRL_E_UNSUPPORTED, nothing launched: N > cusrl_step_epilogue_max_envs() (there is no ticket-slot form of it). */
int cusrl_play_epilogue(const float *reward, const uint8_t *terminated, const uint8_t *truncated, uint8_t *done_out,
                        float *episode_rew, float *episode_len, float *ring_rew, float *ring_len, uint64_t *num_episodes,
                        double *step_reward_sum, int64_t *indices_out, int32_t *count_out, int64_t N, int64_t D, int64_t R,
                        int parity, int64_t *episode_count, int64_t target_episodes, int32_t *unfinished_out,
                        uint32_t *workspace, void *stream);
int64_t cusrl_play_epilogue_workspace_words(void);

/* ---- post-update policy statistics — cusrl/hook/on_policy/stats.py:28-40 for Normal policies ----
 * out[0] = mean_b KL(N(old_mean, old_std) || N(new_mean, new_std)) summed over the A action dims (kl_divergence),
 * out[1] = mean of advantage * exp(log N(action; new_mean, new_std) - old_logp)  (importance_weighted_advantage),
 * out[2] = mean of new_std (action_std).  [B, A] matrices, old_logp [B], advantage [B, D];
 * partials: double[cusrl_policy_stats_num_partials(B)][3] workspace.  Fixed summation order (deterministic). */
int cusrl_policy_stats(const float *old_mean, const float *old_std, const float *new_mean, const float *new_std,
                       const float *action, const float *old_logp, const float *advantage, int64_t B, int64_t A,
                       int64_t D, double *partials, float *out, void *stream);
int64_t cusrl_policy_stats_num_partials(int64_t B);
/* The same hook for one-hot categorical policies (cusrl/nn/module/distribution.py:332-366; torch's
 * _kl_categorical_categorical): out[0] = mean_b KL(softmax(old_logits) || softmax(new_logits)),
 * out[1] = mean of advantage * exp(log_softmax(new_logits)[taken] - old_logp), out[2] = 0 (no action std). */
int cusrl_categorical_policy_stats(const float *old_logits, const float *new_logits, const float *action,
                                   const float *old_logp, const float *advantage, int64_t B, int64_t A, int64_t D,
                                   double *partials, float *out, void *stream);

/* ---- differentiable policy terms — OnPolicyPreparation.objective, cusrl/hook/on_policy/common.py:29-43 ----
 * logp = sum_a log N(action | mean, std) (cusrl/nn/module/distribution.py:207-209), entropy (distribution.py:211-213),
 * logp_ratio = logp - old_logp, ratio = exp(logp_ratio); outputs [B].  The stock `ppo` composition gets these (and their
 * gradients) from cusrl_ppo_loss_fwd_bwd; this pair serves compositions in which a further hook defines `objective` and
 * may read or differentiate them (one launch forward, one backward instead of the reference's ~15 torch ops + autograd).
 * std: [B, A] (std_rows = B) or ONE [A] vector shared by all rows (std_rows = 1).
 * Backward: g_* = gradients wrt the four outputs, each [B] or NULL; `ratio` = the forward's output (needed with g_ratio).
 * d_mean [B, A]; d_std [B, A], or [A] for a std vector (column sums in fixed order through d_std_partials:
 * float[cusrl_policy_terms_std_partial_rows(B)][A], A <= 64). */
int cusrl_policy_terms_fwd(const float *mean, const float *std, int64_t std_rows, const float *action,
                           const float *old_logp, int64_t B, int64_t A, float *logp_out, float *entropy_out,
                           float *logp_ratio_out, float *ratio_out, void *stream);
int cusrl_policy_terms_bwd(const float *mean, const float *std, int64_t std_rows, const float *action, const float *ratio,
                           const float *g_logp, const float *g_entropy, const float *g_logp_ratio, const float *g_ratio,
                           int64_t B, int64_t A, float *d_mean, float *d_std, float *d_std_partials, void *stream);
int64_t cusrl_policy_terms_std_partial_rows(int64_t B);
/* The same pair for one-hot categorical policies (distribution.py:354-362): logits / one-hot action [B, A]. */
int cusrl_categorical_terms_fwd(const float *logits, const float *action, const float *old_logp, int64_t B, int64_t A,
                                float *logp_out, float *entropy_out, float *logp_ratio_out, float *ratio_out, void *stream);
int cusrl_categorical_terms_bwd(const float *logits, const float *action, const float *ratio, const float *g_logp,
                                const float *g_entropy, const float *g_logp_ratio, const float *g_ratio, int64_t B,
                                int64_t A, float *d_logits, void *stream);

/* ---- MLP backward epilogues (callers of the path: torch.nn.Linear / ReLU backward of the actor-critic) ----
 * Bias gradient = column sums of grad [rows, H]; with `output` != NULL the ReLU backward mask is applied first
 * (grad_in = grad * (output > 0), written to grad_in) and the column sums are taken of the masked gradient, i.e.
 * threshold_backward + sum(0) of autograd in one pass.  partials: float[cusrl_colsum_num_partials(rows, H)][H]
 * workspace; colsum: float[H] (fixed summation order: deterministic), or NULL to get the partial rows only (H % 4 == 0
 * layouts): their column sums are then taken by cusrl_assemble_gradients. */
int cusrl_relu_bwd_colsum(const float *grad, const float *output, float *grad_in, float *partials, float *colsum,
                          int64_t rows, int64_t H, void *stream);
int64_t cusrl_colsum_num_partials(int64_t rows, int64_t H);

/* ---- backward of the FIRST layer of an MLP (ABI 6): y = relu(x W^T + b) whose input needs no gradient — the observation layer
 * of the actor / critic backbones (cusrl/nn/module/mlp.py:89-90; what autograd runs there: threshold_backward, sum(0), the
 * weight-gradient GEMM).  ONE pass over grad_out [rows, H], output [rows, H] (the ReLU's output: grad is masked by output > 0;
 * NULL: no activation) and input [rows, K] produces dW [H, K] = masked^T x and db [H] = column sums of masked — nothing is
 * written back per row (no masked-gradient matrix: dX is not needed).  The products run on v_mfma_f32_16x16x4_f32 (exact f32,
 * the column of ones of db included); the kernel is bound by the 4 (2 H + K) bytes per row it streams.
 * Result: grads float[H * K + H] = dW (row-major) | db — what cusrl_assemble_gradients copies into the two parameters' slots
 * (offset 0 / numel H*K and offset H*K / numel H).  Two launches on `stream`: the pass (per block one [64, K + 1] piece of a
 * partial row) and a small fixed-order sum of the partial rows (a kernel boundary is the cheap cross-XCD fence here).
 * partials: float[cusrl_input_layer_row_blocks(rows, H)][H * K + H] workspace.
 * Supported (cusrl_input_layer_supported): K % 4 == 0, K <= 60, H % 64 == 0, H <= 4096; all pointers 16-byte aligned.
 * Deterministic (fixed summation order). */
int cusrl_input_layer_bwd(const float *grad_out, const float *output, const float *input, int64_t rows, int64_t in_features,
                          int64_t out_features, float *partials, float *grads, void *stream);
int cusrl_input_layer_supported(int64_t in_features, int64_t out_features);
int64_t cusrl_input_layer_row_blocks(int64_t rows, int64_t out_features);

/* ---- backward of a narrow linear layer (policy-mean / value heads; torch.nn.Linear backward with out_features <= 16)
 * One pass over the minibatch produces all three gradients of y = x W^T + b:
 *   grad_input [rows, K] = grad_out W   (skipped when NULL),   dW [O, K] = grad_out^T x,   db [O] = sum_rows grad_out.
 * relu_input != 0: x is the output of a ReLU (x > 0 <=> the ReLU passed); grad_input is then written already
 * masked — the ReLU's backward — and its column sums, the producer layer's bias gradient, are returned too.
 * packed: float[(O + 1) * K + 16] = dW (row-major) | column sums of the masked grad_input (zeros when
 * relu_input == 0) | db, zero padded (NULL: partial rows only, reduced later by cusrl_assemble_gradients);
 * partials: float[cusrl_narrow_linear_num_partials(rows)][(O + 1) * K + 16].
 * Supported shapes (cusrl_narrow_linear_supported): 1 <= O <= 16, K in {32, 64, ..., 1024} a power of two; all
 * pointers 16-byte aligned.  Fixed summation order (deterministic). */
int cusrl_narrow_linear_bwd(const float *grad_out, const float *input, const float *weight, float *grad_input,
                            float *partials, float *packed, int64_t rows, int64_t in_features, int64_t out_features,
                            int relu_input, void *stream);
int64_t cusrl_narrow_linear_num_partials(int64_t rows);
int cusrl_narrow_linear_supported(int64_t in_features, int64_t out_features);
/* Forward of a ONE-output linear layer — the value head (cusrl/nn/module/critic.py:87-88), a discriminator's logit
 * (cusrl/hook/auxiliary/amp.py:138-147): output[b] = input[b, :] . weight + bias[0] (bias may be NULL), one launch instead
 * of torch's broadcast-bias copy + skinny GEMM.  out_features must be 1 (wider heads keep the library GEMM and its bias
 * epilogue), in_features as for cusrl_narrow_linear_supported; input / weight 16-byte aligned. */
int cusrl_narrow_linear_fwd(const float *input, const float *weight, const float *bias, float *output, int64_t rows,
                            int64_t in_features, int64_t out_features, void *stream);

/* ---- inference pass of a two-hidden-layer ReLU MLP + head, one launch (csrc/mlp_forward.hip) ----
 * output[b, :] = w3 relu(w2 relu(w1 input[b, :] + b1) + b2) + b3 — the Linear / ReLU stack of cusrl/nn/module/mlp.py:74-93
 * behind the policy-mean head (cusrl/nn/module/actor.py:69-92, distribution.py:256-262) or the value head
 * (cusrl/nn/module/critic.py:87-88), evaluated WITHOUT autograd: acting (ActorCritic.act, actor_critic.py:226-244), the value
 * targets (hook/on_policy/value.py:58-79), the post-update statistics (hook/on_policy/stats.py:29-40).  Replaces three library
 * GEMMs (+ the sampling launch): every intermediate stays on chip, a workgroup keeps its weight slices in registers and walks
 * 16-row tiles.  fp32 MFMA accumulation; agrees with the library GEMMs to a few ulp of the accumulated magnitude.
 * Weights are torch.nn.Linear's: w1 [hidden1, in], w2 [hidden2, hidden1], w3 [out, hidden2], row-major; b3 may be NULL.
 * Sampling epilogue (eps != NULL; std [out] vector, eps [rows, out]): action = mean + eps * std, logp[b] = sum_a log N(action |
 * mean, std) with the expressions and the summation order of cusrl_normal_sample_logp, std_out (optional) = std repeated per
 * row; `output` (optional then) receives the mean.  Without eps: std / action / logp / std_out must be NULL and output given.
 * Supported (cusrl_mlp2_forward_supported): in % 4 == 0, 4 <= in <= 64; hidden1 in {128, 256}; hidden2 in {64, 128};
 * 1 <= out <= 16; input / weights / biases 16-byte aligned (output too when out % 4 == 0). */
int cusrl_mlp2_forward(const float *input, int64_t rows, int64_t in_features, const float *w1, const float *b1, int64_t hidden1,
                       const float *w2, const float *b2, int64_t hidden2, const float *w3, const float *b3, int64_t out_features,
                       float *output, const float *std, const float *eps, float *action, float *logp, float *std_out,
                       void *stream);
int cusrl_mlp2_forward_supported(int64_t in_features, int64_t hidden1, int64_t hidden2, int64_t out_features);

/* ---- gradient-norm clipping (hook/on_policy/gradient_clipping.py:67-83 -> torch.nn.utils.clip_grad_norm_) ----
 * norm_out[0] = ||grad||_2 (pre-clip, the `grad_norm/default` metric); grad *= min(max_norm / (norm + 1e-6), 1).
 * max_norm < 0: measure only.  grad: float[n], 16-byte aligned (the flat gradient buffer every .grad aliases);
 * partials: double[cusrl_clip_grad_norm_num_partials(n)] workspace.  Fixed summation order (deterministic). */
int cusrl_clip_grad_norm(float *grad, int64_t n, float max_norm, double *partials, float *norm_out, void *stream);
int64_t cusrl_clip_grad_norm_num_partials(int64_t n);

/* ---- flat gradient assembly (the buffer behind actor_critic.py:311-314: backward, all-reduce, clip, step) ----
 * flat[offset .. offset + numel) = sum over `splits` stacked slabs of src [splits][numel]; splits = 1 copies a
 * plain gradient, splits = 0 writes zeros (src ignored).  The split-batch weight-gradient GEMMs leave their
 * [S, out, in] partial products here instead of running one sum(0) each; the column-sum kernels (bias gradients,
 * cusrl_relu_bwd_colsum / cusrl_narrow_linear_bwd called without their output pointer) leave their per-block partial
 * rows here instead of running a finalize launch each (a column window of a wider partial row is addressed through
 * `src` + `row_stride`).  One launch per 24 pieces.  Fixed order.
 * sumsq_partials (optional): double[cusrl_assemble_gradients_blocks(pieces, num_pieces)] — every block also stores the sum
 * of squares of the gradient elements it wrote; summed, that is the squared gradient norm of clip_grad_norm_
 * (gradient_clipping.py:74) and cusrl_adam_step takes the rows as its clip_partials, so a single-process optimizer step
 * needs no separate squared-sum pass (with several ranks the all-reduce changes the gradients in between). */
typedef struct {
    const void *src;
    int64_t offset;     /* element offset of the parameter's slot in `flat` */
    int64_t numel;
    int64_t splits;
    int64_t row_stride; /* elements between consecutive slabs; 0 = numel (densely stacked slabs) */
} cusrl_grad_piece_t;
int cusrl_assemble_gradients(const cusrl_grad_piece_t *pieces, int64_t num_pieces, float *flat, double *sumsq_partials,
                             void *stream);
int64_t cusrl_assemble_gradients_blocks(const cusrl_grad_piece_t *pieces, int64_t num_pieces);

/* Block partials of sum(grad^2) only (the first half of cusrl_clip_grad_norm): the caller hands them to
 * cusrl_adam_step, which applies the clipping coefficient while it streams the gradient. */
int cusrl_grad_sumsq(const float *grad, int64_t n, double *partials, void *stream);

/* ---- optimizer step on flat buffers (torch.optim.Adam / AdamW, the optimizer of cusrl/preset/ppo.py) ----
 * One launch: step += 1; g = grad * clip (clip = min(max_norm / (||grad|| + 1e-6), 1) from `clip_partials`, or 1
 * when NULL; max_norm < 0: norm only); AdamW: param *= 1 - lr wd, Adam: g += wd param;
 * exp_avg += (g - exp_avg)(1 - beta1); exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2;
 * param -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)   (torch's fused kernel).
 * Hyper-parameters are doubles like torch's: 1 - beta and the bias corrections are formed in double, then rounded.
 * param / grad / exp_avg / exp_avg_sq: float[n], 16-byte aligned; step, lr: device float[1] (hipGraph replays see
 * schedule changes); norm_out: device float[1] or NULL (receives ||grad||, the `grad_norm` metric);
 * norm_accumulator (ABI 6): device float[1] or NULL — ||grad|| is ADDED to it (the running sum a captured step keeps of the
 * metric over its replays, cusrl_accumulate_scalars' job without its launch);
 * ticket: device uint32[1], zero-initialised once by the caller and owned by this entry point afterwards. */
int cusrl_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, const float *lr,
                    int64_t n, double beta1, double beta2, double eps, double weight_decay, int decoupled_weight_decay,
                    int maximize, const double *clip_partials, int64_t num_clip_partials, float max_norm,
                    float *norm_out, float *norm_accumulator, uint32_t *ticket, void *stream);

/* cusrl_adam_step over ONE WINDOW of the flat buffers (round 6): the optimizer step of the parameters of one network, issued on
 * the stream that produced their gradients — the critic's on the critic's branch of a captured minibatch step, the others' on
 * the main stream — so that the two branches of the step never join (actor_critic.py:311-320 runs clip + step once, behind one
 * backward).  The clipping coefficient is the GLOBAL one (gradient_clipping.py:74): the squared norm is the sum of
 * clip_partials_a[0 .. num_a) followed by clip_partials_b[0 .. num_b) — the partial rows of the two windows' gradient
 * assemblies, in the order ONE assembly of all parameters would have left them; both launches of a step are handed the same
 * two arrays and compute the same norm to the bit.  param / grad / exp_avg / exp_avg_sq point at the window's first element
 * (16-byte aligned), n is its length; every window has its own `step` counter and `ticket`; step_mirror (optional): a second
 * device float[1] that receives the new step count too (the other window's counter, when a launch covers both windows). */
int cusrl_adam_step_window(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, const float *lr,
                           int64_t n, double beta1, double beta2, double eps, double weight_decay, int decoupled_weight_decay,
                           int maximize, const double *clip_partials_a, int64_t num_a, const double *clip_partials_b,
                           int64_t num_b, float max_norm, float *norm_out, float *norm_accumulator, float *step_mirror,
                           uint32_t *ticket, void *stream);

/* cusrl_adam_step_window that measures the gradient norm ITSELF (ABI 6, second part of round 6): the step of a job with several
 * ranks, where the gradient all-reduce (cusrl/utils/distributed.py:145-172, actor_critic.py:314) sits between the gradient assembly
 * — whose free partial sums are of the un-averaged gradients — and the clipping (gradient_clipping.py:74), so that the squared
 * norm used to be a launch of its own (cusrl_grad_sumsq) on the serial tail of every minibatch step.  One launch: every block sums
 * the squares of its share of norm_grad[0 .. norm_n) (the WHOLE flat gradient buffer, also when the launch steps one window of
 * it), publishes its partial sum in `workspace`, waits for the launch's other blocks, and derives the coefficient from all
 * partial sums in fixed order; then the step of cusrl_adam_step_window over param / grad / exp_avg / exp_avg_sq [0 .. n).  The
 * grid depends on norm_n and the device alone (at most half a block per CU, <= 256: the blocks of a launch meet inside it, and two
 * launches may do so side by side), so the launches of a
 * step's windows find the same norm to the bit.  workspace: cusrl_adam_step_normed_workspace_bytes() device bytes, 8-byte
 * aligned, filled with 0xFF bytes ONCE by the caller and owned by the entry point afterwards (self-re-arming: safe to replay
 * from a hipGraph); two launches that may run side by side need a workspace each.  norm_grad: 16-byte aligned.  Everything else
 * as cusrl_adam_step_window; max_norm < 0: measure only. */
int cusrl_adam_step_normed(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *step, const float *lr,
                           int64_t n, double beta1, double beta2, double eps, double weight_decay, int decoupled_weight_decay,
                           int maximize, const float *norm_grad, int64_t norm_n, void *workspace, float max_norm, float *norm_out,
                           float *norm_accumulator, float *step_mirror, uint32_t *ticket, void *stream);
int64_t cusrl_adam_step_normed_workspace_bytes(void);

/* ---- running observation statistics ----
 * cusrl/nn/utils/normalization.py:15-50 `mean_var_count` of x [rows, C] restricted to rows with mask != 0 (mask may
 * be NULL = all rows; replaces the host-synchronising boolean-mask select of hook/mdp/observation.py:206-208):
 * batch_mean[C], batch_var[C] (population variance, correction = 0), batch_count (device double[1]);
 * an empty selection yields mean 0, var 1, count 0 like the reference.  Any C < 2^30 (C >= 256: a second partials
 * kernel whose lanes walk a row in windows of 256 channels); the sums are shifted by row 0's value of each channel, so
 * the variance does not cancel when |mean| >> std and a constant channel gives var 0 exactly.
 * partials: double[cusrl_masked_stats_num_partials(rows, C)][C + 1][2] workspace. */
int cusrl_masked_col_stats(const float *x, const uint8_t *mask, int64_t rows, int64_t C, double *partials,
                           float *batch_mean, float *batch_var, double *batch_count, void *stream);
int64_t cusrl_masked_stats_num_partials(int64_t rows, int64_t C);

/* cusrl/nn/utils/normalization.py:80-93 `merge_mean_var_` + cusrl/nn/layer/rms.py:163-167: merge batch statistics into
 * the running mean / var (weights count : batch_count), std = sqrt(var + eps), count += batch_count (capped at
 * max_count when max_count > 0); a zero batch_count leaves everything unchanged.  count, batch_count: device double[1]. */
int cusrl_rms_merge(float *mean, float *var, float *std, double *count, const float *batch_mean,
                    const float *batch_var, const double *batch_count, float eps, double max_count, int64_t C,
                    void *stream);

/* cusrl/nn/layer/rms.py:198-203 `normalize`: out = clamp((x - mean) / std, -clamp, clamp) (clamp <= 0: no clamp). */
int cusrl_rms_normalize(const float *x, const float *mean, const float *std, float clamp, float *out, int64_t rows,
                        int64_t C, void *stream);

/* ---- recurrent BPTT data movement ----
 * Done-split sequence layout of a temporal batch — cusrl/nn/utils/recurrent.py:63-92 (`compute_sequence_lengths`),
 * :215-252 (`split_and_pad_sequences`), :160-199 (`scatter_memory`).  done is [L, N] bytes (the last step always ends
 * a sequence).  Sequences are numbered env-major (all segments of env 0 in time order, then env 1, ...).
 *  phase 1  cusrl_sequence_count: sequences per env -> exclusive prefix within each block of 256 envs
 *           (env_prefix[N] int32), block totals (block_totals[cusrl_sequence_blocks(N)] int32) and the total number
 *           of sequences Ns (num_sequences, device int32[1]) — the host reads Ns to size the padded tensors;
 *  phase 2  cusrl_sequence_layout: dest[t*N + n] = pos * Ns + seq (int64: row of slot (t, n) inside the padded
 *           [L, Ns] layout), first_seq[n] = index of env n's first sequence, and mask[pos * Ns + seq] = 1 for valid
 *           padded positions (mask [L, Ns] bytes must be zeroed by the caller); optionally (NULL to skip)
 *           seq_lengths[seq] = number of valid steps of every sequence (int64[Ns], `compute_sequence_lengths`) and
 *           last_seq[n] = index of the sequence still running at the end of env n's column (int64[N]).
 * Packing / unpacking any [L, N, ...] tensor is then cusrl_scatter_rows / cusrl_gather_rows with `dest`.
 * cusrl_gather_memory — cusrl/nn/utils/recurrent.py:124-157 (`gather_memory`, the inverse of scatter_memory used by
 * the packed-sequence forward, cusrl/nn/module/rnn.py:273-291): out[n] = memory[last_seq[n]], zeroed where
 * done_last[n] (the env finished exactly at the last step); rows of row_bytes bytes. */
int cusrl_sequence_count(const uint8_t *done, int64_t L, int64_t N, int32_t *env_prefix, int32_t *block_totals,
                         int32_t *num_sequences, void *stream);
int64_t cusrl_sequence_blocks(int64_t N);
int cusrl_sequence_layout(const uint8_t *done, int64_t L, int64_t N, const int32_t *env_prefix,
                          const int32_t *block_totals, int64_t Ns, int64_t *dest, int64_t *first_seq, uint8_t *mask,
                          int64_t *seq_lengths, int64_t *last_seq, void *stream);
int cusrl_gather_memory(const void *memory, const int64_t *last_seq, const uint8_t *done_last, void *out, int64_t N,
                        int64_t row_bytes, void *stream);

/* ---- intrinsic-reward epilogues ----
 * RND, cusrl/hook/auxiliary/rnd.py:71-74: reward[i] += scale * mean_k (target[i,k] - prediction[i,k])^2 for i < rows
 * (reward has one channel); bonus_out (optional, [rows]) receives the added term for the `rnd_reward` metric. */
int cusrl_rnd_reward(const float *target, const float *prediction, float *reward, float *bonus_out, float scale,
                     int64_t rows, int64_t K, void *stream);
/* AMP, cusrl/hook/auxiliary/amp.py:134-136: reward[i] += scale * -log(max(1 - 1/(1 + exp(-logit[i])), 1e-4));
 * bonus_out as above (`amp_reward`). */
int cusrl_amp_style_reward(const float *logit, float *reward, float *bonus_out, float scale, int64_t rows, void *stream);
/* The style reward together with the mean the metric `amp_reward` records (amp.py:134-136 + agent.record): one
 * single-workgroup launch for rows <= 2^20 (an env step), instead of the reward launch + a reduction. mean_out: float[1]. */
int cusrl_amp_style_reward_mean(const float *logit, float *reward, float *bonus_out, float scale, int64_t rows,
                                float *mean_out, void *stream);

/* ---- AdversarialMotionPrior.post_step up to the discriminator — cusrl/hook/auxiliary/amp.py:112-128 ----
 * agent rows  = cat(state[n, columns], next_state[n, columns])  (columns: K int32 entries, NULL = 0..K-1; state rows are
 *               `state_pitch` floats apart), or `agent_raw` [N, C] when the env provides `amp_obs` (state = NULL);
 * expert rows = dataset[indices[n]] (indices: the int64 draws of torch.randint, so the random stream is the
 *               reference's), or `expert_raw` [N, C] when a demonstration sampler provides them;
 * then transition_rms.update(agent), transition_rms.update(expert) (population statistics, Chan merge with weights
 * count : N, count capped at max_count if > 0 — the arithmetic of cusrl_masked_col_stats + cusrl_rms_merge) and both
 * normalised + clamped (clamp <= 0: none) with the statistics after BOTH updates, into agent_out / expert_out [N, C].
 * C = 2K <= 128, N * C <= cusrl_amp_prepare_max_elements(): TWO launches (assemble + block partial sums; merge +
 * normalise, every block folding the <= 64 partial rows itself) instead of the reference's cat + index + 2 x
 * var_mean/merge + 2 x normalise (~25 torch launches; 10 launches of the per-op kernels above).
 * workspace: double[cusrl_amp_prepare_workspace(N, C)]. */
int cusrl_amp_prepare(const float *state, const float *next_state, int64_t state_pitch, const int32_t *columns, int64_t K,
                      const float *agent_raw, const float *dataset, const int64_t *indices, const float *expert_raw,
                      int64_t N, int64_t C, float *mean, float *var, float *std, double *count, float eps,
                      double max_count, float clamp, float *agent_out, float *expert_out, double *workspace, void *stream);
int64_t cusrl_amp_prepare_max_elements(void);
int64_t cusrl_amp_prepare_workspace(int64_t N, int64_t C);

/* ---- the synthetic benchmark env of BASELINE.json config 2 (cusrl_amd/testing/environment.py; the reference ships
 * no such env — its step is this package's definition of the workload): next_observation ~ N(0, 1) [N, obs_dim],
 * reward ~ N(0, 1) [N, reward_dim], terminated / truncated ~ Bernoulli(p) [N] bytes, reset_rows ~ N(0, 1) [N, obs_dim] (one
 * fresh row per env for the resets), from Philox4x32-10 keyed on (seed, step number, stream, element) in ONE launch.
 * counter: uint64[2] device words {step number, arrival ticket}, zero-initialised by the caller; the launch advances the
 * step number itself (its last block), so a hipGraph replay draws fresh numbers. */
int cusrl_synthetic_env_step(uint64_t seed, uint64_t *counter, int64_t N, int64_t obs_dim, int64_t reward_dim,
                             float p_terminate, float p_truncate, float *next_observation, float *reward,
                             uint8_t *terminated, uint8_t *truncated, float *reset_rows, void *stream);

/* accumulator[i] += *values[i] for i < n <= 32 (values: HOST array of device pointers to fp32 scalars): the per-step
 * running sums of the metrics a captured minibatch / env step records (cusrl/utils/metrics.py:17-28 keeps running means
 * with four torch launches per metric and step).  One launch. */
int cusrl_accumulate_scalars(const float *const *values, int n, float *accumulator, void *stream);

/* ---- RewardShaping.post_step — cusrl/hook/mdp/reward.py:43-47 ----
 * reward = clamp(reward * scale + shift, lower, upper) in place (the product and the sum rounded separately like the two
 * torch ops; has_lower / has_upper = 0: that bound is None). */
int cusrl_reward_shaping(float *reward, float scale, float shift, float lower, float upper, int has_lower, int has_upper,
                         int64_t n, void *stream);

/* ---- ObservationNanToNum.pre_act / post_step — cusrl/hook/mdp/observation.py:42-56 ----
 * tensor.nan_to_num_(nan, posinf, neginf) in place on up to TWO contiguous fp32 arrays (the observation and the state of one
 * hook call) in ONE launch; b == NULL or nb == 0: only a.  Classified on the bit pattern: every NaN (any sign, any payload)
 * becomes `nan`, +Inf `posinf`, -Inf `neginf`; every finite value keeps its bits (-0.0, denormals, +-FLT_MAX).  Only 4-byte
 * alignment is required of a and b (offset views): scalar head up to a 16-byte boundary, 16-byte body, scalar tail, per array.
 * A lane stores only where it replaced something: clean input is read, never written.  Both pointers travel by value: no
 * device-side table, no staging copy, no memset — a plain kernel node under capture.  na + nb == 0: returns 0, no launch. */
int cusrl_nan_to_num2(float *a, int64_t na, float *b, int64_t nb, float nan, float posinf, float neginf, void *stream);

/* ---- nn.MSELoss(prediction, target) forward AND backward — RandomNetworkDistillation.objective, rnd.py:78-81 ----
 * loss_out[0] = mean((prediction - target)^2) over n elements (fp64 block partials, fixed order),
 * d_prediction = 2 (prediction - target) / n.  partials: double[cusrl_mse_loss_num_partials(n)]. */
int cusrl_mse_loss_fwd_bwd(const float *prediction, const float *target, int64_t n, float *loss_out, float *d_prediction,
                           double *partials, void *stream);
int64_t cusrl_mse_loss_num_partials(int64_t n);
/* loss_out[0] = loss_scale * sum(x^2), grad_out = grad_scale * x — the gradient penalty of AMP's discriminator objective
 * (mean_n ||dD/dx_n||^2, cusrl/nn/layer/loss.py:10-56) and what it sends back into the input gradient; same workspace. */
int cusrl_sumsq_fwd_bwd(const float *x, int64_t n, double loss_scale, double grad_scale, float *loss_out, float *grad_out,
                        double *partials, void *stream);
/* AMP's discrimination loss over the joint batch logit[2 * rows] (first half agent = target 0, second half expert =
 * target 1): loss_out[0] = weight * mean BCE-with-logits = (BCE(D(agent), 0) + BCE(D(expert), 1)) / 2 * loss_weight
 * (amp.py:143-147), d_logit = weight * (sigmoid(logit) - target) / (2 rows).  One launch instead of ~10 torch ops. */
int cusrl_bce_pair_fwd_bwd(const float *logit, int64_t rows, float weight, float *loss_out, float *d_logit, void *stream);

/* ---- weight * nn.MSELoss(prediction, target[..., columns]) forward AND backward with the target read in place ----
 * StateEstimation.objective (estimation.py:126-131), ReturnPrediction / StatePrediction / NextStatePrediction.objective
 * (representation.py:40-45, 108-113, 167-173), PolicyDistillationLoss.objective (distillation.py:44-47).
 * prediction [rows, K] contiguous; row r of the target starts at target + r * target_pitch (elements): a buffer leaf or a
 * row view of one, never copied.  columns: K int32 device entries, column k of the prediction is compared with target column
 * columns[k] (any order, repeats allowed); NULL: columns 0..K-1.  The CALLER guarantees 0 <= columns[k] < target_pitch (the
 * table lives on the device: the kernel does not check it); with columns == NULL, target_pitch >= K is checked here.
 *   loss_out[0]        = weight / (rows K) * sum_{r,k} (prediction[r,k] - target[r, columns[k]])^2
 *   d_prediction[r,k]  = 2 weight / (rows K) * (prediction[r,k] - target[r, columns[k]])
 * fp64 block partials in fixed order (bit-reproducible, no atomics, no memset); partials: double[max(1,
 * cusrl_column_mse_num_partials(rows, K))].  One block finalises itself; beyond that a one-block finalize follows.
 * rows * K > INT32_MAX: CUSRL_E_UNSUPPORTED (cusrl_column_mse_num_partials then returns 0). */
int cusrl_column_mse_fwd_bwd(const float *prediction, const float *target, int64_t target_pitch, const int32_t *columns,
                             int64_t rows, int64_t K, float weight, float *loss_out, float *d_prediction, double *partials,
                             void *stream);
int64_t cusrl_column_mse_num_partials(int64_t rows, int64_t K);

/* ---- NormalNllLoss forward AND backward — cusrl/nn/layer/loss.py:62-141 ----
 * nll[r,k] = 0.5 (log_var + (target[r,k] - mean[r,k])^2 / var) (+ log sqrt(2 pi) when full = 1), where dist[r,k], clamped from
 * below at `bound`, is log_var (mode 0), log_std (1), var (2) or std (3); `bound` is given in that domain (log eps, log eps / 2,
 * eps, sqrt eps).  loss_out[0] = mean (reduction 1) or sum (reduction 2) of nll over rows * K elements; d_mean and d_dist are
 * its gradients, d_dist zero where dist < bound (torch's clamp_min backward).  A NaN in dist stays a NaN.
 * Row r of mean / dist / target starts at the pointer + r * its pitch (elements), K elements wide; row r of BOTH gradients at
 * d_mean / d_dist + r * grad_pitch.  A chunked [rows, 2K] input is mean = input, dist = input + K, both pitches 2K, and one
 * [rows, 2K] gradient, d_mean = grad, d_dist = grad + K, grad_pitch = 2K; a target that is a column view of a wider leaf is
 * read in place.  Every pitch >= K.  float4 accesses when K and every pitch are multiples of 4 and every pointer is 16-byte
 * aligned, scalar ones otherwise.  Per element in fp32, fp64 block partials in fixed order (bit-reproducible, no atomics, no
 * memset); partials: double[max(1, cusrl_normal_nll_num_partials(rows, K))], the launch rule of cusrl_column_mse_fwd_bwd.
 * rows * K > INT32_MAX: CUSRL_E_UNSUPPORTED (cusrl_normal_nll_num_partials then returns 0). */
int cusrl_normal_nll_fwd_bwd(const float *mean, int64_t mean_pitch, const float *dist, int64_t dist_pitch, const float *target,
                             int64_t target_pitch, int64_t rows, int64_t K, int mode, int full, float bound, int reduction,
                             float *loss_out, float *d_mean, float *d_dist, int64_t grad_pitch, double *partials, void *stream);
int64_t cusrl_normal_nll_num_partials(int64_t rows, int64_t K);

/* ---- ActionSmoothnessLoss.objective forward AND backward — cusrl/hook/auxiliary/smoothness.py:59-102 ----
 * mean [T, B, A] fp32 (the action mean of a temporal minibatch), done [T, B] 1-byte flags; an episode ends at a set flag,
 * that step included (cusrl/nn/utils/recurrent.py:63-92, 215-252); done[T-1] is never read as a boundary.
 *   first order,  1 <= t < T: pair (t-1, t) of env b valid iff !done[t-1, b];                d1 = mean[t] - mean[t-1]
 *   second order, 2 <= t < T: triple valid iff !done[t-2, b] && !done[t-1, b];               d2 = -mean[t-2] + 2 mean[t-1] - mean[t]
 *   losses_out[k-1] = sum_valid sum_a w_k[a] |d_k| / (n_k A);  counts_out[k-1] = n_k, the exact number of valid pairs / triples
 *   gradient of term k: +-w_1[a] sign(d1) / (n_1 A) on rows t, t-1;  (-1, +2, -1) w_2[a] sign(d2) / (n_2 A) on rows t-2, t-1, t
 * with sign(0) = 0.  n_k = 0: losses_out[k-1] = NaN (the mean of an empty selection) and the term's gradient is all zeros.
 * w1 / w2: DEVICE fp32 [A] vectors, read by the launch (a changed weight needs no new capture); NULL: that term is not
 * evaluated, its loss slot is 0; both NULL: CUSRL_E_INVALID.  d_mean holds one [T, B, A] plane PER NON-NULL WEIGHT, the first
 * order's first: the terms' gradients stay apart so that each can be scaled by its own incoming gradient.  Every element of
 * those planes is written exactly once (no zero-fill by the caller, no atomics).
 * One thread walks one (b, a) column along t; fp32 per element, fp64 block sums finished in one fixed order
 * (bit-reproducible).  Launches on `stream`: a count pass over `done`, the walk, and a one-block finalize beyond one block
 * of 256 columns.  workspace: cusrl_action_smoothness_workspace(T, B, A) 8-byte words, not initialised by the caller.
 * T < 3: CUSRL_E_INVALID;  T * B * A > INT32_MAX: CUSRL_E_UNSUPPORTED (the workspace query then returns 0). */
int cusrl_action_smoothness_fwd_bwd(const float *mean, const uint8_t *done, const float *w1, const float *w2, int64_t T,
                                    int64_t B, int64_t A, float *losses_out, int64_t *counts_out, float *d_mean,
                                    void *workspace, void *stream);
int64_t cusrl_action_smoothness_workspace(int64_t T, int64_t B, int64_t A);


/* ---- Mirror symmetry — cusrl/hook/auxiliary/symmetry.py:30-62,155-356, cusrl/hook/mdp/observation.py:213-217 (ABI 7) ----
 * A mirror table (int32, device) describes MirrorDef(destination_indices, flipped_indices), out[j] = in[dest[j]] * (-1 if j is
 * flipped else 1), out width C_out = len(dest), in width C_in:
 *   table[0 .. C_out)                      code of output column j: dest[j] | (flipped ? 1u << 31 : 0)
 *   table[C_out .. C_out + C_in + 1)       offsets into the inverse list, per input column (CSR)
 *   table[C_out + C_in + 1 .. 2 C_out + C_in + 1)  inverse list: the codes (output column | flip bit) that read input column i,
 *                                          in increasing output column
 * A negation is a sign flip: bit-exact against `x * -1` for every non-NaN x, signed zeros included.
 *
 * One field of cusrl_mirror_rows: rows r in [0, rows) of src [R, src_width] (row stride src_stride elements) go to
 * dst[r * dst_stride + dst_offset + j], j in [0, width): a copy (table == NULL, width == src_width) or the mirror through
 * `table` (width = C_out, src_width = C_in).  dst_stride / dst_offset let one launch write the [R, 2, C] rows of
 * SymmetricDataAugmentation (original half copied, mirrored half through the table) and the repeated narrow leaves
 * ([R, 2, 1] advantage: two copies).  Bytes moved: rows * 4 (src_width read + width written) per field. */
typedef struct {
    const float *src;
    int64_t src_stride;
    float *dst;
    int64_t dst_stride;
    int64_t dst_offset;
    const int32_t *table;
    int32_t width;
    int32_t src_width;
} cusrl_mirror_field_t;

/* All fields in ONE launch (`fields` is a HOST array, passed by value to the kernel).  rows == 0 launches nothing. */
int cusrl_mirror_rows(const cusrl_mirror_field_t *fields, int n_fields, int64_t rows, void *stream);

/* Gradient of the mirror: grad_in[r, i] = sum over the output columns j that read i, in increasing j, of
 * sign_j * grad_out[r, j] (fp32, fixed order: a non-bijective map gives the same bits every time); a column nobody reads gets 0.
 * grad_out [rows, C_out] (row stride go_stride), grad_in [rows, C_in] (row stride gi_stride). */
int cusrl_mirror_rows_bwd(const float *grad_out, int64_t go_stride, float *grad_in, int64_t gi_stride, const int32_t *table,
                          int64_t c_in, int64_t c_out, int64_t rows, void *stream);

/* MirrorSymmetryLoss.objective (symmetry.py:204-231) forward AND backward in one pass, C_in == C_out == A:
 *   loss_out[0] = weight * mean((mu - M(mu_m))^2) over [B, A]
 *   loss_out[1] = weight * mean((sigma - |M(sigma_m)|)^2) when sigma != NULL (else 0)
 * mu = the current action mean, mu_m = the mean the actor gives for the mirrored observations, both [B, A] contiguous.
 * sigma / sigma_m: [B, A], or with std_vector != 0 the [A] vector the actor repeats over the rows (the term is then the
 * mean over A, which is the mean of the repeated matrix).  Gradients of loss_out[0] + loss_out[1]: d_mu, d_mu_m [B, A]
 * (d_mu_m already taken back through the mirror, fixed-order sums), d_sigma, d_sigma_m (the shape of sigma; abs' gradient is
 * torch.sign, 0 at 0).  fp64 block partials; partials: double[2 * cusrl_mirror_mse_num_partials(B * A)].  Beyond one
 * block a one-block finalize follows.  Nothing is read back to the host. */
int cusrl_mirror_mse_fwd_bwd(const float *mu, const float *mu_m, const float *sigma, const float *sigma_m, int std_vector,
                             const int32_t *table, int64_t B, int64_t A, double weight, float *loss_out, float *d_mu,
                             float *d_mu_m, float *d_sigma, float *d_sigma_m, double *partials, void *stream);
int64_t cusrl_mirror_mse_num_partials(int64_t n);

/* The symmetric statistics of ObservationNormalization._update_rms_impl (observation.py:213-217), in place on fp32 mean / var
 * [C] (C_in == C_out == C <= CUSRL_MAX_SYMMETRIZE_CHANNELS), one rounding per operation in the reference's order:
 *   var = (var + |M(var)|) / 2 + (mean - M(mean))^2 / 4,  then  mean = (mean + M(mean)) / 2.  One workgroup. */
int cusrl_symmetrize_mean_var(float *mean, float *var, const int32_t *table, int64_t C, void *stream);

/* The head of a symmetric actor (SymmetricActor, symmetry.py:396-487; additive entries of ABI 7).  The wrapped actor ran ONCE
 * over the stacked rows: mean2 [2B, A] contiguous, rows [0, B) for the observations and rows [B, 2B) for the mirrored
 * observations; std2 is [2B, A] in the same layout (AdaptiveNormalDist) or, with std_vector != 0, the [A] vector NormalDist
 * repeats, which is one row that is both halves.  `table`: the action mirror's table above for C_in == C_out == A;
 * M = "gather by destination_indices, then flip the listed outputs".
 * SHAPE LIMITS of all three: 1 <= A <= CUSRL_MAX_SYMMETRIC_HEAD_ACTIONS and 0 <= B with 2 B A <= INT32_MAX; outside them
 * CUSRL_E_UNSUPPORTED (the host then evaluates the torch expression).  B == 0 launches nothing.
 *
 * cusrl_symmetric_head_fwd, ONE launch:  mean_out[b] = (mean_o[b] + M(mean_m[b])) / 2,  std_out[b] = (std_o[b] + |M(std_m[b])|) / 2,
 * both [B, A]; one fp32 add, exact mirror and halving: bit-identical to the torch expression on the same operands.
 *
 * cusrl_symmetric_head_sample, ONE launch: the same combine, action = mean + std * eps (eps [B, A] from the caller, one fp32
 * multiply and one add) and logp [B, 1] = the Normal log-probability of `action` summed over A (accumulated in fp64).
 *
 * cusrl_symmetric_head_bwd, ONE launch (+ the finalize below): from g_mean / g_std [B, A] (either may be NULL: that gradient
 * is neither read nor written) the gradients of the stacked operands, d_mean2 [2B, A] and d_std2 ([2B, A], or [A] for a vector):
 *   d_o[b, i] = g[b, i] / 2
 *   d_m[b, i] = sum over the output columns j that read i, in increasing j, of sign_j * g[b, j] / 2   (0 when nobody reads i)
 * and for the std every term times sgn(M(std_m)[b, j]), sgn(0) = 0 (torch's abs).  A std vector's gradient is the sum over b
 * of d_o + d_m per column: fp64 partial sums per block in a fixed order, no atomics.  d_bias (optional, needs g_mean): [A], the
 * gradient of the head's bias b when mean2 = raw2 + b and the head itself treats b as a constant — the same column sums for the
 * mean, the two halves added ROW BY ROW, so that a column that mirrors onto itself with a flip gets exactly 0 as in the
 * reference's two passes.  partials: double[cusrl_symmetric_head_num_partials(B, A)] (only read and written with column sums);
 * beyond one block of rows per column a finalize launch of one block per column follows.  std2 is only read when g_std != NULL. */
int cusrl_symmetric_head_fwd(const float *mean2, const float *std2, int std_vector, const int32_t *table, int64_t B, int64_t A,
                             float *mean_out, float *std_out, void *stream);
int cusrl_symmetric_head_sample(const float *mean2, const float *std2, int std_vector, const float *eps, const int32_t *table,
                                int64_t B, int64_t A, float *action, float *logp, float *mean_out, float *std_out, void *stream);
int cusrl_symmetric_head_bwd(const float *g_mean, const float *g_std, const float *std2, int std_vector, const int32_t *table,
                             int64_t B, int64_t A, float *d_mean2, float *d_std2, float *d_bias, double *partials,
                             void *stream);
int64_t cusrl_symmetric_head_num_partials(int64_t B, int64_t A);

/* ---- residual add + LayerNorm — the row-wise work of cusrl/nn/module/simba.py:28-73 (`input + block(input)`, nn.LayerNorm)
 * (additive entries of ABI 7; csrc/layer_norm.hip).  Every residual add of a pre-LayerNorm backbone is followed by a LayerNorm
 * (the next block's, or the final one), so the two are one pass over the row.  x, residual, sum_out, y, dy, ds, s, d_s: [B, H]
 * contiguous fp32; gamma, beta, d_gamma, d_beta: [H]; mean, rstd: fp32 [B].  1 <= H <= CUSRL_MAX_LAYER_NORM_WIDTH (a row is at
 * most 16 values per lane of the wavefront that owns it), any B >= 0 (B == 0 launches nothing); CUSRL_E_UNSUPPORTED outside.
 * Pointers need 4-byte alignment only: 16-byte aligned operands with H % 4 == 0 move as 16-byte accesses, anything else as
 * 4-byte accesses, with the same lane-to-column assignment and therefore the same bits.  No atomics: the same bits every run.
 *
 * cusrl_add_layer_norm_fwd, ONE launch, one wavefront per row, the row read once:
 *   s = x + residual (one fp32 add, torch's bits), stored to sum_out;  residual == NULL: s = x, sum_out is not written;
 *   y = (s - mean) * rstd * gamma + beta with torch's statistics: mean and the biased variance of the row accumulated in
 *   float64 in two passes over the register-resident row, rstd = 1 / sqrt(var + eps), each rounded to fp32 once;
 *   mean / rstd (both or neither): the statistics for the backward, NULL in passes nobody differentiates.
 *
 * cusrl_add_layer_norm_bwd, ONE launch (+ a one-block finalize when more than one block ran):
 *   d_s = rstd * (g - mean_H(g) - xhat * mean_H(g * xhat)) + ds,  g = dy * gamma,  xhat = (s - mean) * rstd;
 *   ds (optional): the gradient that reaches s directly (the residual path behind this LayerNorm).  d_s is the gradient of
 *   x and of residual alike.  d_gamma = sum_rows dy * xhat, d_beta = sum_rows dy: float64 column sums per block, laid down in
 *   `partials` (double[cusrl_add_layer_norm_num_partials(B, H)], 0 when one block does it all: may be NULL then) and summed in
 *   block order by the finalize; the grid is capped (256 blocks) so that this stays one block's work. */
#define CUSRL_MAX_LAYER_NORM_WIDTH 1024
int cusrl_add_layer_norm_fwd(const float *x, const float *residual, const float *gamma, const float *beta, float eps,
                             float *sum_out, float *y, float *mean, float *rstd, int64_t B, int64_t H, void *stream);
int cusrl_add_layer_norm_bwd(const float *dy, const float *ds, const float *s, const float *mean, const float *rstd,
                             const float *gamma, float *d_s, float *d_gamma, float *d_beta, double *partials, int64_t B,
                             int64_t H, void *stream);
int64_t cusrl_add_layer_norm_num_partials(int64_t B, int64_t H);

/* ---- per-column affine map with fixed statistics — `Normalization.forward` cusrl/nn/module/normalization.py:52 and
 * `Denormalization.forward` :89, the layers at the two ends of a `Sequential` backbone (additive entries of ABI 7;
 * csrc/column_affine.hip).  x, out, dy, dx: [rows, C] contiguous fp32; mean, std: [C].  ONE launch each; 4-byte aligned
 * pointers work (16-byte lanes when C % 4 == 0 and every pointer is 16-byte aligned, 4-byte lanes otherwise: the same bits).
 * out may be x and dx may be dy.  rows == 0 launches nothing and writes nothing.  CUSRL_E_INVALID: a NULL pointer, rows < 0,
 * C < 1, inverse outside {0, 1}; CUSRL_E_UNSUPPORTED: C > INT32_MAX or rows * C beyond int64.
 *
 * cusrl_column_affine_fwd — each step one correctly rounded fp32 operation, i.e. torch's bits for the reference's expression:
 *   inverse == 0 (normalization.py:52): out[r, c] = (x[r, c] - mean[c]) / std[c]   a subtraction, then a DIVISION (no reciprocal)
 *   inverse == 1 (normalization.py:89): out[r, c] = x[r, c] * std[c] + mean[c]     a multiplication, then an addition (no fma)
 * cusrl_column_affine_bwd — what torch's autograd gives for those expressions; mean and std are not trainable in the
 * reference (`requires_grad=False`), so there is no column reduction:
 *   inverse == 0 (normalization.py:52): dx = dy / std          inverse == 1 (normalization.py:89): dx = dy * std */
int cusrl_column_affine_fwd(const float *x, const float *mean, const float *std, float *out, int64_t rows, int64_t C,
                            int inverse, void *stream);
int cusrl_column_affine_bwd(const float *dy, const float *std, float *dx, int64_t rows, int64_t C, int inverse, void *stream);

/* ---- gates and GLU activations — the element-wise work between the GEMMs of cusrl/nn/layer/gate.py:36-136 and
 * cusrl/nn/layer/activation.py:7-26 (additive entries of ABI 7; csrc/gate.hip).  Every operand is [rows, C] contiguous fp32
 * (the GLU input and its gradient [rows, 2 H]).  ONE launch each; the launch shape of cusrl_column_affine_*: 4-byte aligned
 * pointers work (16-byte lanes when C % 4 == 0 — H % 4 == 0 for the GLU — and every non-NULL pointer is 16-byte aligned,
 * 4-byte lanes otherwise: the same bits), grid capped with a stride over the rest, 64-bit element indices.  rows == 0 launches
 * nothing and writes nothing.  No output may alias an input or another output.  CUSRL_E_INVALID: a NULL pointer among the
 * operands the kind uses (listed below), rows < 0, C < 1, an unknown kind; CUSRL_E_UNSUPPORTED: C > INT32_MAX or the element
 * count beyond int64.  An operand the kind does not use is never read or written and may be NULL.
 *
 * s(v) = 1 / (1 + expf(-v)), t(v) = tanhf(v), one rounded fp32 operation per step (no fma).  p and q are PRE-activations, bias
 * included (the outputs of the gate's linear layers); p2 / q2 (each NULL or present) are second addends, P = p + p2 and
 * Q = q + q2 in that order, so that `r_y(y) + r_x(x)` (gate.py:130-134) needs no add launch of its own.
 *
 *   kind            cusrl_gate_fwd: out =               uses        cusrl_gate_bwd, from dout (g = s(P), h = t(Q))       reads / writes
 *   GATE_INPUT      g x + y                 (:47-48)    x y p       dx = dout g, dp = dout x g (1 - g)                   x p / dx dp
 *   GATE_OUTPUT     x + g y                 (:63-64)    x y p       dy = dout g, dp = dout y g (1 - g)                   y p / dy dp
 *   GATE_HIGHWAY    g x + (1 - g) y         (:80-81)    x y p       dx = dout g, dy = dout (1 - g), dp = dout (x - y) g (1 - g)   x y p / dx dy dp
 *   GATE_SIGMOID_TANH  x + g h              (:97-99)    x p q       dp = dout h g (1 - g), dq = dout g (1 - h h)         p q / dp dq
 *   GATE_GRU_RESET  g x                     (:130,134)  x p         dx = dout g, dp = dout x g (1 - g)                   x p / dx dp
 *   GATE_GRU_OUT    (1 - g) x + g h         (:132-136)  x p q       dx = dout (1 - g), dp = dout (h - x) g (1 - g), dq = dout g (1 - h h)   x p q / dx dp dq
 * The gradient of an operand that enters `out` as itself (y of INPUT; x of OUTPUT and SIGMOID_TANH) is dout and is not written;
 * dp is the gradient of p and of p2 alike, dq of q and q2.  The backward recomputes g and h from the pre-activations: no
 * activation is saved.  Its 1 - g, g (1 - g) and 1 - h h are evaluated without the cancellation of the fp32 differences, as
 * e / (1 + e), e / (1 + e)^2 with e = expf(-|P|) and 4 u / (1 + u)^2 with u = expf(-2 |Q|), so that a gradient tensor keeps
 * 1e-5 of its largest entry even when that entry sits at |P| = 8.  A saturated pre-activation gives g in {0, 1} or h in
 * {-1, 1} exactly, a finite `out`, and g (1 - g) or 1 - h h EXACTLY zero there (the fp32 forward is constant); nothing divides
 * by a quantity that can vanish.
 *
 * cusrl_glu_fwd: out[r, c] = a act(b) with a = input[r, c], b = input[r, H + c], the halves read in place;
 *   GLU_GEGLU (:13-15): act(b) = b Phi(b), Phi(b) = erfcf(-b / sqrt 2) / 2 — the exact (erf) GELU, torch's default;
 *   GLU_SWIGLU (:24-26): act(b) = b s(b).
 * cusrl_glu_bwd writes both halves of dinput [rows, 2 H]: dinput[r, c] = dout act(b), dinput[r, H + c] = dout a act'(b);
 *   GELU' = Phi(b) + b phi(b), phi(b) = expf(-b b / 2) / sqrt(2 pi);  SiLU' = s + b s (1 - s). */
#define CUSRL_GATE_INPUT 0
#define CUSRL_GATE_OUTPUT 1
#define CUSRL_GATE_HIGHWAY 2
#define CUSRL_GATE_SIGMOID_TANH 3
#define CUSRL_GATE_GRU_RESET 4
#define CUSRL_GATE_GRU_OUT 5
#define CUSRL_GLU_GEGLU 0
#define CUSRL_GLU_SWIGLU 1
int cusrl_gate_fwd(int kind, const float *x, const float *y, const float *p, const float *p2, const float *q, const float *q2,
                   float *out, int64_t rows, int64_t C, void *stream);
int cusrl_gate_bwd(int kind, const float *x, const float *y, const float *p, const float *p2, const float *q, const float *q2,
                   const float *dout, float *dx, float *dy, float *dp, float *dq, int64_t rows, int64_t C, void *stream);
int cusrl_glu_fwd(int kind, const float *input, float *out, int64_t rows, int64_t H, void *stream);
int cusrl_glu_bwd(int kind, const float *input, const float *dout, float *dinput, int64_t rows, int64_t H, void *stream);

/* ---- scaled dot-product attention and the rotary embedding — what cusrl/nn/layer/mha.py:133-140 hands to
 * F.scaled_dot_product_attention, and cusrl/nn/layer/encoding.py:107-125 (additive entries of ABI 7; csrc/attention.hip).
 * fp32 throughout; the [N, H, Lq, Lk] scores are never written to memory.
 *
 * Layout: q [N, Lq, H, D], k and v [N, Lk, H, D] with element (n, l, h, d) at base + n * stride_n + l * stride_l + h * D + d
 * (strides in elements, per tensor): the slices of a packed [N, L, 3, H, D] or [N, L, 2, H, D] projection and a
 * batch_first=False transposition are read where they are.  dout is read the same way.  out, dq [N, Lq, H, D] and dk, dv
 * [N, Lk, H, D] are written contiguous; lse is [N, H, Lq].  A lane moves 16 bytes where D % 4 == 0 and every strided base is
 * 16-byte aligned with strides that are multiples of 4, and 4 bytes otherwise: the same arithmetic per element, the same bits.
 *
 * Masks: `causal` (top-left aligned: key j is visible to query i iff j <= i, whatever Lq and Lk), OR-ed with at most one of
 * keep_mask (uint8, nonzero = attend) and bias (fp32, added to the scaled score; -inf = a masked key), either read at
 * n * mask_stride_n + h * mask_stride_h + i * mask_stride_q + j * mask_stride_k (element strides; 0 for a broadcast dimension).
 *
 * cusrl_sdpa_fwd, ONE launch:  s_ij = scale * sum_d q_id k_jd (+ bias_ij), -inf where masked;
 *   out_i = sum_j softmax_j(s_i.) v_j  by online softmax over key tiles;  lse_i = ln sum_j exp(s_ij) (the row maximum included).
 * cusrl_sdpa_bwd, TWO launches on the stream (query-major, then key-major), from q, k, v, out, lse, dout:
 *   p_ij = exp(s_ij - lse_i),  delta_i = sum_d dout_id out_id,  ds_ij = p_ij (sum_d dout_id v_jd - delta_i) scale;
 *   dq_i = sum_j ds_ij k_j (the query-major pass, which also writes delta into `workspace`);
 *   dk_j = sum_i ds_ij q_i,  dv_j = sum_i p_ij dout_i (the key-major pass).
 *   workspace: float[cusrl_sdpa_bwd_workspace(N, H, Lq, Lk, D)] (-1 for sizes the entries refuse).
 * Every output element has one owning lane that adds its terms in index order: no atomics, the same bits on every call.
 * A query row with every key masked: out_i = 0, lse_i = -inf, p_i. = 0 exactly, so it adds exactly zero to dq, dk and dv;
 * exp(-inf - (-inf)) is never evaluated and nothing is NaN.
 *
 * 1 <= D <= CUSRL_MAX_SDPA_HEAD_DIM; H, Lq, Lk >= 1 otherwise unbounded (64-bit indices, the key tiles loop); N == 0 is a
 * successful no-op.  CUSRL_E_INVALID, nothing launched: a NULL operand the call needs (the masks are optional), a negative
 * size, H, Lq or Lk < 1, D out of range, keep_mask and bias together.  CUSRL_E_UNSUPPORTED: an extent beyond int64.
 *
 * cusrl_rope_apply, ONE launch: x [N, L, H, D] read at n * x_stride_n + l * x_stride_l + h * D + d, out [N, L, H, D]
 * contiguous, cos_rows / sin_rows [L, D / 2] contiguous (the cache rows offset .. offset + L), D even.  With x = (x1, x2) the
 * two halves of the last dimension and c, s the row l of cos_rows, sin_rows:
 *   transpose == 0 (encoding.py:112-125, x cos + rotate_half(x) sin):  out = (x1 c + (-x2) s,  x2 c + x1 s)
 *   transpose == 1 (its backward, dx = dout cos - rotate_half(dout sin)):  out = (x1 c + x2 s,  x2 c - x1 s)
 * CUSRL_E_INVALID: a NULL pointer, N < 0, L or H < 1, D < 2 or odd, transpose outside {0, 1}. */
#define CUSRL_MAX_SDPA_HEAD_DIM 128
int cusrl_sdpa_fwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n, int64_t k_stride_l,
                   const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *keep_mask, const float *bias,
                   int64_t mask_stride_n, int64_t mask_stride_h, int64_t mask_stride_q, int64_t mask_stride_k, int causal,
                   float scale, float *out, float *lse, int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D, void *stream);
int cusrl_sdpa_bwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n, int64_t k_stride_l,
                   const float *v, int64_t v_stride_n, int64_t v_stride_l, const float *out, const float *lse, const float *dout,
                   int64_t dout_stride_n, int64_t dout_stride_l, const uint8_t *keep_mask, const float *bias,
                   int64_t mask_stride_n, int64_t mask_stride_h, int64_t mask_stride_q, int64_t mask_stride_k, int causal,
                   float scale, float *dq, float *dk, float *dv, float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t Lk,
                   int64_t D, void *stream);
int64_t cusrl_sdpa_bwd_workspace(int64_t N, int64_t H, int64_t Lq, int64_t Lk, int64_t D);
int cusrl_rope_apply(const float *x, int64_t x_stride_n, int64_t x_stride_l, const float *cos_rows, const float *sin_rows,
                     float *out, int64_t N, int64_t L, int64_t H, int64_t D, int transpose, void *stream);

/* ---- causal sliding-window ("band") attention — the attention core of cusrl/nn/module/causal_attn.py:135-258, whose mask and
 * score rule are cusrl/nn/utils/attention.py:117-124 and 158-159 (additive entries of ABI 7; csrc/attention.hip).  fp32.
 *
 * q [N, Lq, H, D]; k and v [N, Lk, H, D] with Lk = Lq + W, the first W keys being the cache.  Layout, strides and the 16-byte /
 * 4-byte load rule are those of cusrl_sdpa_* above.  Key j is visible to query i iff all of
 *   i <= j <= i + W;
 *   key_valid[n * Lk + j] != 0                      (key_valid: uint8 [N, Lk] contiguous, or NULL: every key exists);
 *   q_segment[n * Lq + i] == seg_kv(n, j)           (q_segment: int32 [N, Lq] contiguous, or NULL: one segment), where
 *                                                   seg_kv(n, j) = 0 for j < W and q_segment[n * Lq + j - W] otherwise.
 * s_ij = scale * sum_d q_id k_jd - alibi_slopes[h] * (float)(i + W - j)   (alibi_slopes: fp32 [H], or NULL: no bias), -inf
 * where key j is not visible.  out, lse, p, delta, ds, dq, dk, dv: the formulas of cusrl_sdpa_fwd / cusrl_sdpa_bwd.
 *
 * cusrl_band_sdpa_fwd, ONE launch; only the band is streamed: a workgroup's 16 queries q0 .. q0 + 15 read the key tiles from
 *   q0 up to min(Lk, q0 + 16 + W).  Lq == 1 (the step of a rollout) takes a kernel of its own: one 16-lane group per (n, h)
 *   reads the W + 1 keys straight from global memory, online softmax in chunks of 16 keys.
 * cusrl_band_sdpa_bwd, TWO launches (query-major: dq and delta into `workspace`; key-major: dk, dv).  dk and dv are
 *   [N, Lk - key_grad_from, H, D] contiguous, row j - key_grad_from holding key j; keys in front of key_grad_from are not
 *   visited (0 <= key_grad_from <= W: a cache whose projection is detached passes W).  A workgroup's 16 keys j0 .. j0 + 15 read
 *   the query tiles from max(0, j0 - W) up to min(Lq, j0 + 16).
 *   workspace: float[cusrl_band_sdpa_bwd_workspace(N, H, Lq, W, D)] (-1 for sizes the entries refuse).
 * One owning lane per output element, terms added in index order, no atomics, the same bits on every call.  A query with no
 * visible key: out = 0, lse = -inf, exactly zero added to every gradient.
 *
 * N == 0 is a successful no-op.  CUSRL_E_INVALID, nothing launched: a NULL operand the call needs (key_valid, q_segment and
 * alibi_slopes are optional), a negative size, H, Lq or W < 1, D outside 1 .. CUSRL_MAX_SDPA_HEAD_DIM, key_grad_from outside
 * 0 .. W.  CUSRL_E_UNSUPPORTED: an extent beyond int64. */
int cusrl_band_sdpa_fwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                        int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                        const int32_t *q_segment, const float *alibi_slopes, float scale, float *out, float *lse, int64_t N,
                        int64_t H, int64_t Lq, int64_t W, int64_t D, void *stream);
int cusrl_band_sdpa_bwd(const float *q, int64_t q_stride_n, int64_t q_stride_l, const float *k, int64_t k_stride_n,
                        int64_t k_stride_l, const float *v, int64_t v_stride_n, int64_t v_stride_l, const uint8_t *key_valid,
                        const int32_t *q_segment, const float *alibi_slopes, float scale, const float *out, const float *lse,
                        const float *dout, int64_t dout_stride_n, int64_t dout_stride_l, int64_t key_grad_from, float *dq,
                        float *dk, float *dv, float *workspace, int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D,
                        void *stream);
int64_t cusrl_band_sdpa_bwd_workspace(int64_t N, int64_t H, int64_t Lq, int64_t W, int64_t D);

/* ---- depthwise 2-D convolution — the spatial half of cusrl/nn/layer/separable_conv.py:52-64, an nn.Conv2d with
 * groups == in_channels == out_channels and zero padding (additive entries of ABI 7; csrc/conv.hip).  fp32, contiguous:
 *   x, dx [N, C, H, W];  w, dw [C, KH, KW] (the memory of torch's [C, 1, KH, KW]);  bias, dbias [C] (NULL: no bias);
 *   out, dout [N, C, Ho, Wo] with Ho = (H + 2 PH - DH (KH - 1) - 1) / SH + 1 (rounded down) and Wo likewise: torch's formula.
 * Geometry (KH, KW, SH, SW, PH, PW, DH, DW): kernel, stride, zero padding (the same on both sides of an axis), dilation.
 *
 * cusrl_dwconv2d_fwd, ONE launch:
 *   out[n,c,oy,ox] = bias[c] + sum_ky sum_kx w[c,ky,kx] x[n,c, oy SH - PH + ky DH, ox SW - PW + kx DW],
 *   a tap outside the image contributing nothing; fp32, the terms added in (ky, kx) order, no fma.
 * cusrl_dwconv2d_bwd_input, ONE launch, a gather: dx[n,c,iy,ix] = sum over the (ky, kx, oy, ox) with oy SH - PH + ky DH == iy
 *   and ox SW - PW + kx DW == ix of w[c,ky,kx] dout[n,c,oy,ox], in (ky, kx) order.  One owning thread per element, no atomics;
 *   a row or column no window reads (a stride remainder) is the empty sum, exactly 0.0f.
 * cusrl_dwconv2d_bwd_params, at most TWO launches: dw[c,ky,kx] = sum_{n,oy,ox} dout[n,c,oy,ox] x[n,c,iy,ix] (taps inside the
 *   image only) and, unless dbias is NULL, dbias[c] = sum_{n,oy,ox} dout[n,c,oy,ox].  float64 sums in a fixed order — a thread
 *   walks its (n, oy, ox) in ascending order, lanes, waves and blocks are added in index order — rounded to fp32 once: the same
 *   bits on every call.  Up to 64 blocks per channel write a row of CUSRL_MAX_DWCONV_TAPS + 1 sums into
 *   double partials[cusrl_dwconv2d_num_partials(N, C, Ho, Wo)] and one finalize launch adds the rows; where one block per
 *   channel covers everything (N Ho Wo <= 1024) it writes dw and dbias itself, num_partials is 0 and partials may be NULL.
 *   (-1: sizes the entries refuse.)
 * No floating-point atomics anywhere.  Every access is 4 bytes wide: any 4-byte aligned pointer works and gives the same bits.
 * Element indices are 64-bit wherever a count does not fit 32.  No output may alias an input.
 *
 * N == 0 is a successful no-op.  Validation runs on the host before anything is launched.  CUSRL_E_INVALID: a NULL pointer the
 * call uses (bias / dbias are optional; partials where num_partials > 0), N < 0, C, H, W, K*, S* or D* < 1, P* < 0, a geometry
 * whose Ho or Wo is below 1.  CUSRL_E_UNSUPPORTED: KH KW > CUSRL_MAX_DWCONV_TAPS (7 x 7), an extent or element count beyond
 * int64, more than INT32_MAX / 3200 channels. */
#define CUSRL_MAX_DWCONV_TAPS 49
int cusrl_dwconv2d_fwd(const float *x, const float *w, const float *bias, float *out, int64_t N, int64_t C, int64_t H, int64_t W,
                       int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW, int64_t DH, int64_t DW, void *stream);
int cusrl_dwconv2d_bwd_input(const float *dout, const float *w, float *dx, int64_t N, int64_t C, int64_t H, int64_t W, int64_t KH,
                             int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW, int64_t DH, int64_t DW, void *stream);
int cusrl_dwconv2d_bwd_params(const float *x, const float *dout, float *dw, float *dbias, double *partials, int64_t N, int64_t C,
                              int64_t H, int64_t W, int64_t KH, int64_t KW, int64_t SH, int64_t SW, int64_t PH, int64_t PW,
                              int64_t DH, int64_t DW, void *stream);
int64_t cusrl_dwconv2d_num_partials(int64_t N, int64_t C, int64_t Ho, int64_t Wo);

/* ---- std bijectors — the bounded sigmoid and the bounded softplus behind a policy's standard deviation,
 * cusrl/nn/layer/bijector.py:76-126 (additive entries of ABI 7; csrc/bijector.hip).  x, y, dy, dx: contiguous fp32 [n].  ONE
 * launch each; the launch shape of cusrl_column_affine_*: 4-byte aligned pointers work (16-byte lanes when n % 4 == 0 and every
 * pointer is 16-byte aligned, 4-byte lanes otherwise: the same bits), grid capped with a stride over the rest, 64-bit element
 * indices.  y may be x and dx may be dy.  Every step is one rounded fp32 operation (no fma) with the accurate expf / log1pf;
 * s(v) = 1 / (1 + expf(-v)).  The backward recomputes from x: no output is saved.  The float parameters are the fp32 roundings
 * of the module's Python floats, which is what torch makes of them.
 *
 *   kind                 p0, p1, p2                       cusrl_bijector_fwd: y =                    cusrl_bijector_bwd: dx =
 *   BIJECTOR_SIGMOID     min, range, (unused)             min + range s(x)                  (:86)    dy range (1 - s(x)) s(x)
 *   BIJECTOR_SOFTPLUS    scale, min_input, max_input      (z > 20 ? z : log1pf(expf(z))) / scale     dy (z > 20 ? 1 : s(z)) where
 *                                                         with z = clamp(x, min_input, max_input) scale     min_input <= x <= max_input (edges
 *                                                         (:110-111; 20 is torch's softplus threshold)       inclusive), exactly 0.0f elsewhere
 * A NaN x gives a NaN y and, for the softplus, dx = 0.0f (torch's clamp backward); NaN and +-Inf in x or dy otherwise come out
 * where torch's expression puts them.
 *
 * n == 0 launches nothing and writes nothing.  CUSRL_E_INVALID, nothing launched: a NULL pointer, n < 0, an unknown kind, and for
 * the softplus scale <= 0 or min_input > max_input (a NaN among them included).  CUSRL_E_UNSUPPORTED: more lanes than a grid
 * of 32-bit extent has threads (n / 4, or n on the 4-byte path, above INT32_MAX * 256). */
#define CUSRL_BIJECTOR_SIGMOID 0
#define CUSRL_BIJECTOR_SOFTPLUS 1
int cusrl_bijector_fwd(int kind, const float *x, float *y, int64_t n, float p0, float p1, float p2, void *stream);
int cusrl_bijector_bwd(int kind, const float *x, const float *dy, float *dx, int64_t n, float p0, float p1, float p2, void *stream);

/* ---- bias + activation behind a bias-free GEMM — the per-step query of a frozen expert policy (cusrl_amd/nn/expert.py, the
 * teacher of cusrl/hook/auxiliary/distillation.py:50-97; additive entry of ABI 7; csrc/bias_act.hip) ----
 * ONE launch:  out[r, h] = act(x[r, h] + bias[h]),  x and out [rows, H] contiguous fp32, bias [H]; out may be x.  The addition
 * is one rounded fp32 operation, then
 *   ACT_IDENTITY   v
 *   ACT_RELU       v > 0 ? v : 0                     (a NaN stays a NaN)
 *   ACT_ELU        v > 0 ? v : alpha * expm1f(v)     (torch's formula; `alpha` is read by this code only)
 *   ACT_TANH       tanhf(v)                          (+-1 for a large |v|: nothing overflows)
 * NaN propagates; -0.0 and +-Inf come out as the formula gives them.  4-byte aligned pointers work: 16-byte accesses when
 * H % 4 == 0 and all three pointers are 16-byte aligned, 4-byte accesses otherwise, the same bits either way.  A thread keeps its
 * slice of the bias in registers while it walks rows.  No host synchronisation: the launch may be captured.
 * CUSRL_E_INVALID, nothing launched: a NULL pointer, rows < 1 or H < 1.  CUSRL_E_UNSUPPORTED, nothing launched: an unknown
 * activation code, rows * H beyond int64, or a row of more than 65535 * 256 column lanes. */
#define CUSRL_ACT_IDENTITY 0
#define CUSRL_ACT_RELU 1
#define CUSRL_ACT_ELU 2
#define CUSRL_ACT_TANH 3
int cusrl_bias_act(const float *x, const float *bias, float *out, int64_t rows, int64_t H, int activation, float alpha,
                   void *stream);

/* ---- the two elementwise ends of a deployed policy's step (cusrl_amd/nn/deployed.py, the runner of a file written by
 * ActorCritic.export — cusrl/template/actor_critic.py:332-418; additive entries of ABI 7; csrc/deploy.hip) ----
 * cusrl_deploy_prologue, ONE launch in front of the first GEMM:
 *   out[b, k] = clamp((nan_to_num(obs[b, k]) - mean[k]) / std[k], -clamp, clamp)       obs, out [B, K] contiguous fp32
 * Each part is optional.  `replace` is a HOST pointer to the three floats {nan, posinf, neginf}, read before the call returns
 * (NULL: no sanitiser); the classification is the bit pattern's, as cusrl_nan_to_num2 does it.  mean, std [K] (both NULL: no
 * normaliser).  clamp <= 0 (or a NaN): no clamp.  The result has the bits of cusrl_nan_to_num2 followed by cusrl_rms_normalize on
 * the same operands: the same classification, subtraction, correctly rounded division and fminf(fmaxf()) in the same order.
 * out may be obs.  4-byte aligned pointers work: 16-byte accesses when K % 4 == 0 and every pointer given is 16-byte aligned,
 * 4-byte accesses otherwise, the same bits either way.
 * cusrl_deploy_epilogue, ONE launch behind the head's bias-free GEMM, in place on its output y [B, A]:
 *   y[b, a] = clip((y[b, a] + bias[a]) * scale[a] + shift[a], lo[a], hi[a])            bias, scale, shift, lo, hi [A]
 * One add, one multiply and one add (two roundings, never an FMA), then v < lo ? lo : v and v > hi ? hi : v (a NaN stays a
 * NaN, as torch.clamp leaves it).  bias NULL: no bias; scale and shift both NULL: no affine; lo and hi both NULL: no clip.
 * done != NULL (B one-byte flags): the same launch writes zeros over the rows b of memory [B, M] with done[b] != 0 and touches
 * no other row (16-byte stores when M % 4 == 0 and memory is 16-byte aligned, 4-byte stores otherwise).  With nothing to do
 * (every part NULL) nothing is launched.
 * Both: B == 0 launches nothing.  No host synchronisation: the launches may be captured.  CUSRL_E_INVALID, nothing launched:
 * B < 0, K or A < 1, M < 0, a NULL obs / out / y with B > 0, one of a pair (mean and std, scale and shift, lo and hi) without the
 * other, done without a memory of M >= 1, an obs or out that is not 4-byte aligned.  CUSRL_E_UNSUPPORTED: K or A above
 * INT32_MAX, an element count beyond int64.
 * The `_cpu` entries restate the two kernels on the host, element by element with the same expressions (every pointer a HOST
 * pointer, no stream): what the GPU tests compare the kernels' bits against. */
int cusrl_deploy_prologue(const float *obs, const float *replace /* host, 3 floats */, const float *mean, const float *std,
                          float clamp, float *out, int64_t B, int64_t K, void *stream);
int cusrl_deploy_prologue_cpu(const float *obs, const float *replace, const float *mean, const float *std, float clamp, float *out,
                              int64_t B, int64_t K);
int cusrl_deploy_epilogue(float *y, const float *bias, const float *scale, const float *shift, const float *lo, const float *hi,
                          int64_t B, int64_t A, const uint8_t *done, float *memory, int64_t M, void *stream);
int cusrl_deploy_epilogue_cpu(float *y, const float *bias, const float *scale, const float *shift, const float *lo, const float *hi,
                              int64_t B, int64_t A, const uint8_t *done, float *memory, int64_t M);

/* ---- classic-control tasks as device-resident environments (cusrl_amd/environment/; the reference takes these tasks from
 * gymnasium through cusrl/environment/gym.py, one host round trip per step; additive entries of ABI 7; csrc/environment.hip) ----
 * Per env e: a contiguous fp32 row state[e, S], an int32 steps[e] (steps taken in the running episode) and an int64 episode[e]
 * (how often the env has been reset).  All arithmetic fp32, one rounding per written operation, in the written order; sinf /
 * cosf are the platform's.  An action row of a discrete task is read as logits / one-hot: the FIRST maximal column is taken.
 *
 *   CLASSIC_CARTPOLE     S = 4 (x, x', th, th'), action [N, 2], observation = state, F = column 1 ? +10 : -10
 *       temp = (F + 0.05 th'^2 sin th) / 1.1;   th'' = (9.8 sin th - cos th temp) / (0.5 (4/3 - 0.1 cos^2 th / 1.1))
 *       x''  = temp - 0.05 th'' cos th / 1.1;   x += 0.02 x', x' += 0.02 x'', th += 0.02 th', th' += 0.02 th'' (old derivatives)
 *       reward 1;  terminated = |x| > 2.4 or |th| > 12 * 2 pi / 360;  default max_steps 500
 *       reset: four draws U[-0.05, 0.05]
 *   CLASSIC_PENDULUM     S = 2 (th, th'), action [N, 1], observation [cos th, sin th, th'], u = clamp(a, -2, 2)
 *       reward = -(wrap(th)^2 + 0.1 th'^2 + 0.001 u^2) of the OLD state, wrap(th) = floor-mod(th + pi, 2 pi) - pi
 *       th' = clamp(th' + (15 sin th + 3 u) 0.05, -8, 8), then th += 0.05 th';  never terminated;  default max_steps 200
 *       reset: th ~ U[-pi, pi], th' ~ U[-1, 1]
 *   CLASSIC_MOUNTAINCAR  S = 2 (p, v), action [N, 3] -> a in {0, 1, 2}, observation = state
 *       v = clamp(v + (a - 1) 0.001 - 0.0025 cos(3 p), -0.07, 0.07), p = clamp(p + v, -1.2, 0.6), v = 0 if p == -1.2 and v < 0
 *       reward -1;  terminated = p >= 0.5 and v >= 0;  default max_steps 200
 *       reset: p ~ U[-0.6, -0.4], v = 0
 *   CLASSIC_ACROBOT      S = 4 (th1, th2, w1, w2), action [N, 3] -> torque a = column - 1 in {-1, 0, +1},
 *                        observation [cos th1, sin th1, cos th2, sin th2, w1, w2] (O = 6)
 *       constants m1 = m2 = 1, l1 = 1, lc1 = lc2 = 0.5, I1 = I2 = 1, g = 9.8, dt = 0.2; folded, with sin x for cos(x - pi/2), the
 *       derivative f(th1, th2, w1, w2; a) = (w1, w2, w1', w2') is, each line left to right:
 *         d1 = 3.5 + cos th2;   d2 = 1.25 + 0.5 cos th2;   phi2 = 4.9 sin(th1 + th2)
 *         phi1 = (-0.5 (w2 w2)) sin th2 - (w2 w1) sin th2 + 14.7 sin th1 + phi2
 *         w2' = (a + (d2 / d1) phi1 - (0.5 (w1 w1)) sin th2 - phi2) / (1.25 - (d2 d2) / d1);   w1' = -((d2 w2' + phi1) / d1)
 *       one classical Runge-Kutta step, the torque held: k1 = f(s), k2 = f(s + 0.1 k1), k3 = f(s + 0.1 k2), k4 = f(s + 0.2 k3),
 *       s = s + (0.2f / 6.0f) (k1 + 2 k2 + 2 k3 + k4), the sum left to right; then th1, th2 wrapped into [-pi, pi] WITHOUT a loop:
 *       x > pi: x - 2 pi ceil((x - pi) / (2 pi));  x < -pi: x + 2 pi ceil((-pi - x) / (2 pi))  (a NaN stays, an Inf becomes a NaN:
 *       a non-finite angle comes out non-finite and the call returns);  w1 = clamp(w1, -4 pi, 4 pi), w2 = clamp(w2, -9 pi, 9 pi)
 *       terminated = -cos th1 - cos(th1 + th2) > 1 (of the new state);  reward = terminated ? 0 : -1;  default max_steps 500
 *       reset: four draws U[-0.1, 0.1]
 *   CLASSIC_MOUNTAINCARCONTINUOUS  S = 2 (p, v), action [N, 1], observation = state, force = clamp(a, -1, 1)
 *       v = clamp(v + (force 0.0015 - 0.0025 cos(3 p)), -0.07, 0.07), p = clamp(p + v, -1.2, 0.6), v = 0 if p == -1.2 and v < 0
 *       terminated = p >= 0.45 and v >= 0;  reward = (terminated ? 100 : 0) - 0.1 (a a) with the RAW action;  default max_steps 999
 *       reset: p ~ U[-0.6, -0.4], v = 0 (the draw MountainCar takes)
 *   truncated = steps[e] (after the step) >= max_steps and not terminated.
 *
 * cusrl_classic_step, ONE launch, one thread per env: advances state and steps IN PLACE and writes next_observation [N, O] (the
 * terminal observation for a finished env), reward [N, 1] and the one-byte flags terminated / truncated [N, 1]; touches nothing
 * else.  A thread reads and writes only its own env's rows.  4-byte aligned pointers work (a state row moves as one access
 * where `state` is aligned to a row, as S scalars otherwise: the same bits; Acrobot's 6-wide observation row as three 8-byte
 * stores where next_observation is 8-byte aligned too, as 6 scalars otherwise).  No loop's trip count depends on data.
 *
 * cusrl_classic_reset, ONE launch, one thread per index slot k < rows.  live = count ? *count : rows, read on the device.
 *   k < live:   env e = indices[k] is re-initialised: its draws are Philox4x32-10 with counter (e, episode[e]) and key `seed`,
 *               uniforms u = (word >> 8) 2^-24 + 2^-25 mapped as lo + (hi - lo) u — a pure function of (seed, e, episode[e]),
 *               whatever the launch shape and order; then episode[e] += 1 and steps[e] = 0, or with randomize_progress != 0 the
 *               integer floor(max_steps * word / 2^32) of a second Philox call; row k of observation_out is the fresh observation.
 *   k >= live:  row k is the CURRENT observation of env indices[k]; that env's state, steps and episode are not written.
 * indices: int64 [rows], ids in [0, N) (an id outside is skipped, its row written as zeros); distinct within the first `live`
 * (the trainer's step epilogue guarantees it).  Should an id at or above `live` repeat one below it, that row holds the env's
 * observation from before or after this launch's reset — the caller drops such rows.
 *
 * N == 0 (step) / rows == 0 (reset) launch nothing.  CUSRL_E_INVALID, nothing launched: an unknown kind, a negative size,
 * max_steps outside 1 .. INT32_MAX, a NULL or misaligned pointer among those the call uses (count may be NULL).
 * CUSRL_E_UNSUPPORTED: more envs or slots than INT32_MAX * 64.
 * The `_cpu` entries run the same __host__ __device__ bodies on the host (every pointer a HOST pointer, no stream): the host
 * form of the environments and what the GPU tests compare against. */
#define CUSRL_CLASSIC_CARTPOLE 0
#define CUSRL_CLASSIC_PENDULUM 1
#define CUSRL_CLASSIC_MOUNTAINCAR 2
#define CUSRL_CLASSIC_ACROBOT 3
#define CUSRL_CLASSIC_MOUNTAINCARCONTINUOUS 4
int cusrl_classic_step(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps, float *next_observation,
                       float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N, void *stream);
int cusrl_classic_step_cpu(int kind, const float *action, float *state, int32_t *steps, int64_t max_steps, float *next_observation,
                           float *reward, uint8_t *terminated, uint8_t *truncated, int64_t N);
int cusrl_classic_reset(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps,
                        int64_t *episode, float *observation_out, int64_t rows, int randomize_progress, int64_t max_steps, int64_t N,
                        void *stream);
int cusrl_classic_reset_cpu(int kind, uint64_t seed, const int64_t *indices, const int32_t *count, float *state, int32_t *steps,
                            int64_t *episode, float *observation_out, int64_t rows, int randomize_progress, int64_t max_steps,
                            int64_t N);

/* ---- RewardNormalization.post_step (cusrl_amd/hook/mdp/reward.py): rewards divided by the running standard deviation of the
 * discounted return, as gymnasium's NormalizeReward and SB3's VecNormalize(norm_reward=True) do; the reference has no such hook
 * (its users scale IsaacLab rewards by hand); additive entries of ABI 7; csrc/reward_norm.hip ----
 * Operands: reward [N, R] and G [N, R] contiguous fp32 (G: the discounted return per env and reward column), terminated and
 * truncated [N] one-byte flags (done = terminated | truncated), stats [3, R] contiguous float64: row 0 the running mean, row 1
 * the running variance, row 2 the running count of G, per column (a fresh triple is 0, 1, 1e-4).  ONE launch, in this order:
 *   1. G[i, c] = G[i, c] * gamma + reward[i, c]                          fp32, the product and the sum rounded separately
 *   2. update != 0, per column c, all in float64:
 *        pivot = G[0, c] (the new one);  s = sum_i (G[i, c] - pivot);  q = sum_i (G[i, c] - pivot)^2;  d = s / N
 *        batch_mean = pivot + d;  batch_var = q / N - d d, a negative one 0  (population variance; a NaN stays a NaN)
 *        w_sum = count + N;  w_new = N / w_sum;  w_old = count / w_sum;  delta = batch_mean - mean
 *        mean = mean + delta w_new;  var = var + ((batch_var - var) w_new + (delta delta) (w_old w_new));  count = w_sum
 *      (the weighted parallel-variance merge of cusrl_amd/nn/rms.py merge_mean_var_).  update == 0: stats is only read.
 *   3. scale = (float) sqrt(var[c] + epsilon), the float64 root rounded to fp32 once;  reward[i, c] = reward[i, c] / scale, one
 *      correctly rounded fp32 division per element (never a multiplication by a reciprocal).  The mean is NOT subtracted.
 *   4. has_clip != 0: v < -clip ? -clip : v, then v > clip ? clip : v (a NaN stays a NaN)
 *   5. G[i, c] = 0 where done[i]
 * Nothing is filtered: a NaN or Inf reward enters G and, with update != 0, its column's statistics — every reward of that column
 * is then non-finite from this call on — and the call returns.  No loop's trip count depends on data.
 * Launch shape and summation order: one block of 1024 threads per column.  Rows go in chunks of 4 consecutive rows; thread t
 * owns the chunks t, t + 1024, t + 2048, ... and adds their rows to its own (s, q) in ascending row order; the 64 lanes of a wave
 * are summed by the halving tree (lane l += lane l + 32, then 16, 8, 4, 2, 1), the 16 wave totals in wave order starting from 0.
 * The order is a function of N alone: the same operands give the same bits every call.  With R == 1, reward and G 16-byte aligned
 * and both flag arrays 4-byte aligned a whole chunk moves as one 16-byte access per array (the flags as 4 bytes), as scalars
 * otherwise: the same bits.  No atomics, no hand-off between blocks, plain vector stores; no host synchronisation, so the launch
 * may be captured.  N == 0 launches nothing.  CUSRL_E_INVALID, nothing launched: N < 0, R < 1, a NULL pointer with N > 0, a
 * reward or G that is not 4-byte aligned, a stats that is not 8-byte aligned, has_clip != 0 with a clip that is negative or a
 * NaN.  CUSRL_E_UNSUPPORTED: R above 65535, N * R beyond int64.
 * cusrl_reward_normalize_cpu runs the same __host__ __device__ element, merge and scale bodies on the host and visits the rows
 * in the order above (every pointer a HOST pointer, no stream): the hook's host form and what the GPU tests compare against. */
int cusrl_reward_normalize(float *reward, float *G, const uint8_t *terminated, const uint8_t *truncated, double *stats, float gamma,
                           double epsilon, float clip, int has_clip, int update, int64_t N, int64_t R, void *stream);
int cusrl_reward_normalize_cpu(float *reward, float *G, const uint8_t *terminated, const uint8_t *truncated, double *stats,
                               float gamma, double epsilon, float clip, int has_clip, int update, int64_t N, int64_t R);

/* ---- frame stacking: the observation history of cusrl_amd.nn.ObservationStacker and cusrl_amd.environment.FrameStack
 * (gymnasium's FrameStackObservation(env, stack_size, padding_type); the reference has no such wrapper; additive entries of
 * ABI 7; csrc/frame_stack.hip) ----
 * Operands: the history H [N, S, K], persistent contiguous fp32, slot 0 the oldest observation and slot S - 1 the newest; a
 * stacked observation is the same memory order, [N, S * K]: out[n, s * K + k].  The source rows are [.., K0] contiguous fp32.
 * columns: int32 [K] device vector of distinct indices into K0, the columns that are kept, in their order (NULL: K == K0, every
 * column in place; an entry outside [0, K0) reads nothing and stacks +0.0).  padding: how a fresh history is filled from its
 * first observation v — CUSRL_FRAME_STACK_PAD_RESET: every slot is v; CUSRL_FRAME_STACK_PAD_ZERO: slots 0 .. S - 2 are +0.0 and
 * slot S - 1 is v.  Both launches only MOVE 32-bit words: NaN payloads, -0.0 and +-Inf pass bit for bit, no arithmetic is done.
 *
 * cusrl_frame_stack_push, ONE launch: for every row n, H[n, s] = H[n, s + 1] for s < S - 1, then H[n, S - 1] = obs[n, columns];
 * out [N, S * K] is the new H, a buffer of its own (out overlapping H is refused).  fresh != NULL (N one-byte flags): a row
 * whose flag is set is not shifted but refilled from obs[n] by the padding rule, and the launch clears that flag; the other
 * flags are not written.  One lane owns one column (n, k) through all S slots and walks them in ascending order, reading slot
 * s + 1 before it writes slot s: no lane reads a word another lane writes, whatever S is.  A block takes whole rows; the lanes of
 * a row read its flag in front of the block's barrier and the flag is cleared behind it, by that block alone.
 *
 * cusrl_frame_stack_reset, ONE launch, one lane per (slot j, column k): live = count ? *count : L, read on the device (clamped
 * to 0 .. L; count NULL: every slot is valid — the host path and the all-env reset).  indices: int64 [L] env ids; reset_obs
 * [L, K0], row j belonging to env indices[j]; out [L, S * K].
 *   j < live:   H[indices[j]] is refilled from reset_obs[j, columns] by the padding rule; out[j] is the refilled row.  The ids of
 *               the first `live` slots are distinct (the trainer's step epilogue guarantees it).
 *   j >= live:  a stale but valid env id whose row the caller drops: H is NOT written, out[j] is what H[indices[j]] holds.
 * A stale slot may name the same env as a valid one: stale lanes never write H, so the history is what the valid slot wrote, and
 * the stale out row — the env's history from before or after this launch's refill, word by word — is dropped by the caller.
 * An id outside [0, N) is skipped: no history is touched and its out row is +0.0.
 *
 * Both: 4-byte aligned pointers work; with columns == NULL, K % 4 == 0 and H, the source and out 16-byte aligned a lane moves
 * four adjacent columns as one 16-byte word, otherwise one column: the same bits either way.  Grid-stride loops over at most 2048
 * blocks of 256 threads.  The source must not overlap H or out.  Plain vector stores, no atomics, no host synchronisation: the
 * launches may be captured.  N == 0 (push) / L == 0 (reset) launch nothing.  CUSRL_E_INVALID, nothing launched: a negative N
 * or L, S, K or K0 below 1, columns == NULL with K != K0, an unknown padding code, a NULL or misaligned pointer among those the
 * call uses (columns, fresh and count may be NULL), out overlapping H.  CUSRL_E_UNSUPPORTED: S, K or K0 above INT32_MAX, a
 * byte count beyond int64.
 * The `_cpu` entries restate the two kernels on the host, word by word (every pointer a HOST pointer, no stream; slots in
 * ascending j): the host form of the two classes and what the GPU tests compare the kernels' bits against. */
#define CUSRL_FRAME_STACK_PAD_RESET 0
#define CUSRL_FRAME_STACK_PAD_ZERO 1
int cusrl_frame_stack_push(float *H, const float *obs, const int32_t *columns, uint8_t *fresh, float *out, int64_t N, int64_t S,
                           int64_t K, int64_t K0, int padding, void *stream);
int cusrl_frame_stack_push_cpu(float *H, const float *obs, const int32_t *columns, uint8_t *fresh, float *out, int64_t N, int64_t S,
                               int64_t K, int64_t K0, int padding);
int cusrl_frame_stack_reset(float *H, const int64_t *indices, const int32_t *count, const float *reset_obs, const int32_t *columns,
                            float *out, int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0, int padding, void *stream);
int cusrl_frame_stack_reset_cpu(float *H, const int64_t *indices, const int32_t *count, const float *reset_obs, const int32_t *columns,
                                float *out, int64_t L, int64_t N, int64_t S, int64_t K, int64_t K0, int padding);


/* ---- a6 / a14 data-parallel exchange over RCCL / xGMI — cusrl/utils/distributed.py:58-63, 101-110, 145-183 ----
 * One process per GPU (cusrl/utils/config.py:31-44); a communicator spans all ranks of the job and binds to the
 * device that is current when it is created.  Rank 0 draws the 128-byte id (cusrl_comm_unique_id), the host hands it
 * to the other ranks by any means (the Python host uses its torch.distributed store), every rank calls
 * cusrl_comm_create.  The three collectives only ENQUEUE work on `stream` (no host synchronisation, no allocation), so
 * they may be issued during hipGraph capture and then replay as nodes of the captured minibatch step:
 *   cusrl_allreduce_mean  buffer[i] = mean over ranks of buffer[i], in place, fp32 — `reduce_gradients` on the flat
 *                         gradient buffer (distributed.py:145-172; caller template/actor_critic.py:314);
 *   cusrl_allgather       output[r * bytes : (r + 1) * bytes] = rank r's input — `gather_stack` of cat(mean, var) for
 *                         `reduce_mean_var_` (distributed.py:101-110, 175-183), merged by cusrl_merge_mean_var;
 *   cusrl_broadcast       rank `root`'s buffer to every rank, in place — `broadcast_parameters` (distributed.py:58-63).
 * RCCL is resolved at run time from the copy already loaded into the process (PyTorch-ROCm's), else the system one;
 * cusrl_comm_available() == 0 when neither exists.  A failed RCCL call returns CUSRL_E_COMM and leaves its
 * ncclResult_t text in cusrl_comm_last_error() (host string, valid until the thread's next cusrl_comm_* call). */
typedef struct cusrl_comm cusrl_comm_t;
int cusrl_comm_available(void);
const char *cusrl_comm_last_error(void);
int cusrl_comm_unique_id(void *id_out /* host, 128 bytes */);
int cusrl_comm_create(const void *id /* host, 128 bytes */, int world_size, int rank, cusrl_comm_t **comm_out);
int cusrl_comm_destroy(cusrl_comm_t *comm);
/* Abandon a communicator whose enqueued collectives may never complete (a peer rank failed before issuing its half):
 * ncclCommAbort — stops in-flight kernels instead of waiting for them — then frees the handle. */
int cusrl_comm_abort(cusrl_comm_t *comm);
int cusrl_comm_world_size(const cusrl_comm_t *comm);
int cusrl_allreduce_mean(float *buffer, int64_t count, cusrl_comm_t *comm, void *stream);
int cusrl_allgather(const void *input, void *output, int64_t bytes_per_rank, cusrl_comm_t *comm, void *stream);
int cusrl_broadcast(void *buffer, int64_t bytes, int root, cusrl_comm_t *comm, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CUSRL_HIP_H */
