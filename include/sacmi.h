/*
 * sacmi.h — C ABI of the MI355X-native SAC gradient-step library (libsacmi.so).
 *
 * This is the drop-in boundary for the reference's hot path
 * (FilippoCrc/Humanoid-walking-with-SAC, snapshot 2025-02-22):
 *
 *   sac_imp.SAC.__init__            sac_imp.py:9-52        -> sacmi_create
 *   sac_imp.SAC.update_parameters   sac_imp.py:74-144      -> sacmi_step / sacmi_step_async
 *   trainer updates_per_step loop   trainer.py:203-204     -> sacmi_step_many_async
 *   sac_imp.SAC._soft_update_...    sac_imp.py:146-152     -> (inside sacmi_step)
 *   sac_imp.SAC.select_action       sac_imp.py:54-72       -> sacmi_act
 *   nn.Module.state_dict / load     sac_imp.py:154-233     -> sacmi_get_tensor / sacmi_set_tensor
 *   ReplayBuffer.push / __len__     replay_buffer.py:10-11,21-22   -> sacmi_push / sacmi_len
 *   ReplayBuffer.sample (indices)   replay_buffer.py:13-19 -> sacmi_sample_indices (+ inside step)
 *   ReplayBuffer.buffer (read)      sac_imp.py:199          -> sacmi_get_rows
 *   PrioritizedReplayBuffer.sample  replay_buffer.py:48-82 -> sacmi_per_sample
 *   PrioritizedReplayBuffer.update_priorities  replay_buffer.py:84-87 -> sacmi_per_update
 *   random.getstate/setstate, np.random.get_state/set_state -> sacmi_rng_get_mt / sacmi_rng_set_mt
 *
 * Conventions
 *   - Every call returns int status: 0 = OK, otherwise an SACMI_E* code; the message
 *     is in sacmi_last_error() (thread-local).  The Python host maps codes to the
 *     reference's exceptions (ValueError for SACMI_EVALUE, RuntimeError otherwise).
 *   - One context per GPU.  All device work of a context is ordered on its HIP stream
 *     (its own, or one supplied by sacmi_set_stream).  A context is not thread-safe.
 *   - The library owns all device memory; every host pointer argument is copied in
 *     or out before the call returns (except sacmi_step_async, which writes nothing
 *     to host memory).
 *   - Plain C types only: no torch / HIP types cross this boundary.
 */
#ifndef SACMI_H_
#define SACMI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI 3 (round 6): sacmi_step_chained removed (the persistent-chain kernels are gone);
 * sacmi_grad_buffer(0)'s view documents its trailing error-flag words (kDpFlagN). */
#define SACMI_ABI_VERSION 3

enum sacmi_status {
  SACMI_OK = 0,
  SACMI_EVALUE = 1,    /* bad argument (maps to ValueError)          */
  SACMI_ESTATE = 2,    /* call not valid in the current state        */
  SACMI_EDEVICE = 3,   /* HIP runtime error / no device              */
  SACMI_ENAN = 4,      /* non-finite value surfaced (maps to ValueError, as Normal(validate_args)) */
};

enum sacmi_replay_kind { SACMI_REPLAY_UNIFORM = 0, SACMI_REPLAY_PER = 1 };

/* arithmetic of the MLP GEMMs: fp32 (exact f32 MFMA, the reference's precision) or bf16
 * (bf16 MFMA operands, fp32 accumulation; fp32 master weights, Adam, losses and row
 * algebra) — BASELINE configs[4] */
enum sacmi_compute_dtype { SACMI_COMPUTE_FP32 = 0, SACMI_COMPUTE_BF16 = 1 };

typedef struct sacmi_config {
  int32_t state_dim;          /* S  (sac_imp.py:11)                               */
  int32_t action_dim;         /* A  (sac_imp.py:12)                               */
  int32_t hidden_dim;         /* H  (sac_imp.py:13, default 256)                  */
  int32_t max_batch;          /* largest batch_size passed to step / act          */
  double gamma;               /* 0.99  (sac_imp.py:14)                            */
  double tau;                 /* 0.005 (sac_imp.py:15)                            */
  double lr;                  /* 3e-4  (sac_imp.py:16)                            */
  double alpha;               /* 0.2   (sac_imp.py:17) alpha used until the 1st update */
  int32_t auto_entropy;       /* automatic_entropy_tuning (sac_imp.py:18)          */
  int32_t replay_kind;        /* sacmi_replay_kind                                 */
  double action_low;          /* action_bounds (networks_model1.py:52-55)         */
  double action_high;
  int64_t capacity;           /* ReplayBuffer(capacity=1e6) (replay_buffer.py:7)  */
  double per_alpha;           /* 0.6   (replay_buffer.py:26)                      */
  double per_beta_start;      /* 0.4                                             */
  double per_beta_frames;     /* 1e5                                             */
  uint64_t seed;              /* Philox seed for the policy noise (perf mode)     */
  int32_t n_hidden;           /* hidden layers per net: 2 = networks_model1 (the  */
                              /* reference's SAC, sac_imp.py:4), 3 = networks_model2 */
                              /* (networks_model2.py:18-99); 0 means 2            */
  int32_t compute_dtype;      /* sacmi_compute_dtype                              */
} sacmi_config;

typedef struct sacmi_ctx sacmi_ctx;

/* Tensor ids for get/set.  Layout of every tensor is the reference nn.Linear /
 * optimizer layout: weight [out, in] row-major, bias [out]. */
enum sacmi_net { SACMI_POLICY = 0, SACMI_Q1 = 1, SACMI_Q2 = 2, SACMI_Q1_TARGET = 3,
                 SACMI_Q2_TARGET = 4 };
enum sacmi_slot { SACMI_SLOT_PARAM = 0, SACMI_SLOT_GRAD = 1, SACMI_SLOT_ADAM_M = 2,
                  SACMI_SLOT_ADAM_V = 3 };
/* layer index inside a net (n_hidden = 2): policy {0: fc1, 1: fc2, 2: mean, 3: log_std};
 * q {0: fc1, 1: fc2, 2: fc3}.  n_hidden = 3 (networks_model2): policy {0: fc1, 1: fc2,
 * 2: fc3, 3: mean, 4: log_std}; q {0: fc1, 1: fc2, 2: fc3, 3: fc4}.
 * part: 0 = weight, 1 = bias. */

/* scalar ids for get/set_scalar */
enum sacmi_scalar {
  SACMI_S_LOG_ALPHA = 0,       /* log_alpha (sac_imp.py:48)                          */
  SACMI_S_ALPHA = 1,           /* current alpha (0.2 float before the 1st update)    */
  SACMI_S_ALPHA_IS_TENSOR = 2, /* 1 once alpha = log_alpha.exp() (sac_imp.py:135)   */
  SACMI_S_STEP_POLICY = 3,     /* Adam 'step' of each optimizer                     */
  SACMI_S_STEP_Q1 = 4,
  SACMI_S_STEP_Q2 = 5,
  SACMI_S_STEP_ALPHA = 6,
  SACMI_S_ADAM_M_LOG_ALPHA = 7,
  SACMI_S_ADAM_V_LOG_ALPHA = 8,
  SACMI_S_GRAD_LOG_ALPHA = 9,
  SACMI_S_PER_FRAME = 10,      /* PrioritizedReplayBuffer.frame (replay_buffer.py:31) */
  SACMI_S_NOISE_COUNTER = 11,  /* Philox counter (updates drawn so far)             */
  SACMI_S_KEEP_GRADS = 12,     /* host flag: 1 = single-GPU updates also export the   */
                               /* gradients to the GRAD slot (param.grad after        */
                               /* backward); 0 (default) skips those stores           */
  SACMI_S_GRAPH_COUNT = 13,    /* read-only: instantiated update graphs cached by the  */
                               /* context (one per distinct update configuration)     */
  SACMI_S_COUNT = 14
};

/* ---- lifecycle ---------------------------------------------------------------- */
int sacmi_abi_version(void);
const char* sacmi_last_error(void);
int sacmi_device_count(int* n);
int sacmi_create(const sacmi_config* cfg, int device, sacmi_ctx** out);
int sacmi_destroy(sacmi_ctx* ctx);
/* Order all work on an external HIP stream (e.g. torch's current stream), passed
 * as an opaque pointer; NULL returns to the context's own stream. */
int sacmi_set_stream(sacmi_ctx* ctx, void* hip_stream);
int sacmi_synchronize(sacmi_ctx* ctx);

/* ---- parameters / optimizer state (state_dict bridge) ------------------------ */
int sacmi_tensor_numel(sacmi_ctx* ctx, int net, int layer, int part, int64_t* numel);
int sacmi_set_tensor(sacmi_ctx* ctx, int slot, int net, int layer, int part,
                     const float* host, int64_t numel);
int sacmi_get_tensor(sacmi_ctx* ctx, int slot, int net, int layer, int part,
                     float* host, int64_t numel);
int sacmi_set_scalar(sacmi_ctx* ctx, int which, double value);
int sacmi_get_scalar(sacmi_ctx* ctx, int which, double* value);

/* ---- replay (HBM ring, SoA) ----------------------------------------------------- */
/* Append n transitions (copy-in).  s,s2: [n,S] f32; a: [n,A] f32; r: [n] f32;
 * d: [n] u8.  Oldest rows are evicted past capacity (deque(maxlen)).  For PER the
 * new rows get max(priorities) (or 1.0 when empty), replay_buffer.py:36-46. */
int sacmi_push(sacmi_ctx* ctx, const float* s, const float* a, const float* r,
               const float* s2, const uint8_t* d, int64_t n);
/* The same from packed rows [n][2S + A + 2] f32: s | a | r | s2 | d (d: 0 or 1).  Up to
 * 16 rows a chunk are read by the scatter kernel straight from mapped staging (the
 * trainer's row per env step: no copy command ahead of the next update). */
int sacmi_push_packed(sacmi_ctx* ctx, const float* rows, int64_t n);
int sacmi_len(sacmi_ctx* ctx, int64_t* n);
/* Empty the replay: the assignment `replay_buffer.buffer = rows` of checkpoint loading
 * (sac_imp.py:229-230) replaces the contents, so the rows pushed next start a fresh deque.
 * PER priorities are left as they are (the reference's list assignment does not touch its
 * priority array, replay_buffer.py:28-30). */
int sacmi_replay_clear(sacmi_ctx* ctx);
/* Copy rows at deque positions idx[0..n) out (materialises ReplayBuffer.buffer). */
int sacmi_get_rows(sacmi_ctx* ctx, const int64_t* idx, int64_t n, float* s, float* a,
                   float* r, float* s2, uint8_t* d);

/* Same, addressed by ring slot (PrioritizedReplayBuffer indices are list positions
 * = ring slots, replay_buffer.py:40-44,73). */
int sacmi_get_slots(sacmi_ctx* ctx, const int64_t* slots, int64_t n, float* s, float* a,
                    float* r, float* s2, uint8_t* d);

/* ---- RNG bridges ----------------------------------------------------------------- */
/* stream 0 = CPython `random` (uniform indices), stream 1 = numpy legacy
 * RandomState (PER).  key: 624 words, pos: index 0..624. */
int sacmi_rng_set_mt(sacmi_ctx* ctx, int stream, const uint32_t* key, int32_t pos);
int sacmi_rng_get_mt(sacmi_ctx* ctx, int stream, uint32_t* key, int32_t* pos);

/* Perf-mode policy noise (eps of GaussianPolicy.sample, networks_model1.py:87-90 — the
 * reference draws it from torch's generator): Philox4x32-10 keyed by `seed`, counter
 * `offset` + one per update.  Replaces the seed given at create time; the next update
 * re-captures its graphs. */
int sacmi_rng_seed_device(sacmi_ctx* ctx, uint64_t seed, uint64_t offset);

/* random.sample(buffer, batch) positions, drawn on the GPU from stream 0 (advances it). */
int sacmi_sample_indices(sacmi_ctx* ctx, int32_t batch, int64_t* idx_out);

/* ---- the gradient step ----------------------------------------------------------- */
/* One update_parameters(batch): sample (uniform: device MT stream 0 unless idx is
 * given; PER contexts: the device PER sampler on stream 1, ring-slot indices), gather, target, twin-critic step, actor step, alpha step, Polyak.
 * idx:  NULL -> draw on device; else [batch] deque positions.
 * eps1, eps2: NULL -> on-device Philox noise; else [batch, A] standard normals
 *   (eps1 for policy.sample(next_state), eps2 for policy.sample(state)).
 * losses_out (may be NULL): {q1_loss, q2_loss, policy_loss} — synchronises. */
int sacmi_step(sacmi_ctx* ctx, int32_t batch, const int64_t* idx, const float* eps1,
               const float* eps2, float* losses_out);
/* Non-finite inputs (SACMI_ENAN -> ValueError), where the reference raises:
 *   - a NaN policy mean / log_std fed to Normal(mean, std) (networks_model1.py:87) in
 *     policy.sample(next_state) (sac_imp.py:89: the update takes no step) or in
 *     policy.sample(state) (:116: the critic step is taken, the actor / alpha / Polyak
 *     steps are not); select_action(evaluate=False) likewise (sacmi_act);
 *   - NaN PER probabilities (np.random.choice, replay_buffer.py:64: the frame advances, the
 *     numpy stream does not).
 * The device records it and every later update of the stream takes no step (a
 * multi-update launch stops where the reference's loop raised).  sacmi_step (with
 * losses_out), sacmi_fetch_losses, sacmi_per_sample and sacmi_act report it and forget it. */
/* sacmi_step(ctx, batch, NULL, NULL, NULL, losses_out) in two halves: the launch
 * (device indices + device noise; returns at once) and the wait (synchronises, writes the
 * losses, reports SACMI_ENAN like sacmi_step).  Between them the caller's thread is free
 * — the drop-in advances Python's `random` there by the reference's own random.sample
 * (sac_imp.py:75 -> replay_memory.py sample) while the GPU runs the update.  Every launch
 * is followed by exactly one wait; nothing else may be called on the context between. */
int sacmi_step_launch(sacmi_ctx* ctx, int32_t batch);
int sacmi_step_wait(sacmi_ctx* ctx, float* losses_out);
/* Same work, enqueued only (no host sync, no host writes); losses stay on device
 * in a ring of `ring` slots, fetched by sacmi_fetch_losses.  The host-mapped loss, error and
 * done words are maintained by the synchronous forms only (sacmi_step, sacmi_step_launch /
 * _wait): the async forms' kernels store nothing into host memory. */
int sacmi_step_async(sacmi_ctx* ctx, int32_t batch);
/* n_updates consecutive updates (device indices + device noise) as ONE launch: the
 * `for _ in range(updates_per_step): agent.update_parameters(batch_size)` loop of
 * trainer.py:203-204.  Identical results to n_updates sacmi_step_async calls; every
 * update's losses go to the ring.  1 <= n_updates <= 256. */
int sacmi_step_many_async(sacmi_ctx* ctx, int32_t batch, int32_t n_updates);
int sacmi_fetch_losses(sacmi_ctx* ctx, float* out, int32_t max_steps, int32_t* n_out);

/* ---- per-update training diagnostics ------------------------------------------------- */
/* Off at creation.  On, every update — fused or phase-split, synchronous, async or inside a
 * multi-update launch, staged or device-sampled indices, data parallel (the rank's own
 * minibatch: no collective is added) — appends one row of SACMI_STAT_COUNT fp32 values to a
 * device ring of 4096 rows, reduced on the device from what the update's forward passes left
 * in HBM (one more one-workgroup launch in the actor block, behind the forward of the updated
 * critics and before the alpha step).  Over the B rows i of the update's minibatch:
 *   Q1_MEAN, Q2_MEAN  mean q1(s_i, a_i), mean q2(s_i, a_i) (the critics before their step)
 *   Q_TARGET_MEAN     mean q^_i, q^ = r + (1 - d) gamma (min(q1t, q2t)(s', a') - alpha log pi(a'|s'))
 *                     (sac_imp.py:87-98)
 *   TD_MEAN, TD_MAX   mean / max of 0.5 (|q1 - q^| + |q2 - q^|): unweighted, also under
 *                     prioritized feedback
 *   Q_PI_MEAN         mean min(q1, q2)(s_i, a~_i) with the critics AFTER this update's critic
 *                     step (sac_imp.py:117-119)
 *   ENTROPY           -mean log pi(a~_i | s_i)
 *   ALPHA, LOG_ALPHA  the temperature this update's losses used and log_alpha, both before this
 *                     update's alpha step
 *   ALPHA_LOSS        -log_alpha mean(log pi(a~|s) + target_entropy), target_entropy =
 *                     -action_dim (sac_imp.py:128-131); 0 without automatic entropy tuning
 *   REWARD_MEAN       mean r_i
 *   BATCH             (float)B
 * Per-row values are fp32; the sums accumulate in fp64 in a fixed order (no atomics: two runs
 * from the same state give the same bits) and each mean is rounded once.  An update voided by
 * a non-finite input (SACMI_ENAN; any error bit set when the reduction runs) appends nothing,
 * as it returns no losses.  Off, the update's launches are exactly those of a context that
 * never enabled it (the switch is part of the graph key).  SACMI_STATS=1 in the environment at
 * sacmi_create switches it on from the start.
 * Additive: the ABI version is unchanged. */
enum sacmi_stat { SACMI_STAT_Q1_MEAN = 0, SACMI_STAT_Q2_MEAN = 1, SACMI_STAT_Q_TARGET_MEAN = 2,
                  SACMI_STAT_TD_MEAN = 3, SACMI_STAT_TD_MAX = 4, SACMI_STAT_Q_PI_MEAN = 5,
                  SACMI_STAT_ENTROPY = 6, SACMI_STAT_ALPHA = 7, SACMI_STAT_LOG_ALPHA = 8,
                  SACMI_STAT_ALPHA_LOSS = 9, SACMI_STAT_REWARD_MEAN = 10, SACMI_STAT_BATCH = 11,
                  SACMI_STAT_COUNT = 12 };
int sacmi_set_stats(sacmi_ctx* ctx, int32_t on);
int sacmi_stats(sacmi_ctx* ctx, int32_t* on);
/* Synchronises the stream; copies the most recent min(total, 4096, max_rows) rows, oldest
 * first ([n][SACMI_STAT_COUNT] f32); *total (may be NULL) = rows appended since creation.
 * Read-only: reports and clears no error (sacmi_fetch_losses does that). */
int sacmi_fetch_stats(sacmi_ctx* ctx, float* out, int32_t max_rows, int32_t* n_out, int64_t* total);

/* ---- global-norm gradient clipping and per-update gradient norms ---------------------- */
/* torch.nn.utils.clip_grad_norm_ between backward() and optimizer.step(), for the reference's
 * three network optimizers (q1, q2, policy: sac_imp.py:101-125; log_alpha's own optimizer is
 * never clipped).  Per update and group n, over the REAL elements of the group's gradient
 * (torch's weight and bias elements: the storage's pad columns never count):
 *     sumsq_n = sum (g * grad_scale)^2                        fp64, fixed order, no atomics
 *     norm_n  = (float)sqrt(sumsq_n)
 *     coef_n  = min(1.0f, max_norm_n / (norm_n + 1e-6f))      fp32
 *     Adam steps the group from (g * grad_scale) * coef_n
 * grad_scale is 1 on one GPU and 1/world in the data-parallel all-reduce form, where the
 * reduction runs behind the collective: the norm is that of the mean gradient, the same on
 * every rank.  The sharded data-parallel form would need one more collective and is refused:
 * with clipping on, sacmi_step_dp on a sharded context, sacmi_dp_set_sharded(1) and a
 * communicator initialised under $SACMI_DP_SHARD return SACMI_ESTATE before touching state.
 *
 * 0, 0 = off (default; the update's launches are exactly those of a context that never called
 * this).  A positive value or +inf switches the feature on; with one of the two at 0 that
 * range is measured only (as +inf).  Negative or NaN: SACMI_EVALUE.  critic applies to q1
 * and to q2 separately.  With max_norm = +inf the coefficient is exactly 1 and the update's
 * parameters and moments are bit-identical to an unclipped one.  The thresholds live on the
 * device and are written stream-ordered: changing them re-captures nothing (switching the
 * feature on or off selects another captured graph).  On, the fused update takes its Adam
 * steps in launches of their own behind the weight-gradient levels (same arithmetic, same
 * bits as the fused epilogues); everything else of the update is unchanged.
 *
 * A non-finite norm gets no special case (torch's error_if_nonfinite=False): the coefficient
 * and then the group's parameters go non-finite, and the next update's policy sample reports
 * SACMI_ENAN.
 *
 * SACMI_SLOT_GRAD holds the raw, pre-clip gradient (torch scales .grad in place; here the
 * coefficient is applied inside the Adam step): multiply by the update's SACMI_GCOEF_* for
 * torch's post-clip .grad.
 *
 * Every update that returns losses appends one row {norm q1, q2, pi, coef q1, q2, pi} (fp32) to
 * a device ring of 4096 rows; a voided update (any SACMI_ENAN, the actor-batch one whose critic
 * step stood included) appends none.  SACMI_GRAD_CLIP=<critic>[,<actor>] in the environment at
 * sacmi_create switches it on from the start (one value: both ranges; "inf" accepted).
 * Additive: the ABI version is unchanged. */
int sacmi_set_grad_clip(sacmi_ctx* ctx, double max_norm_critic, double max_norm_actor);
int sacmi_grad_clip(sacmi_ctx* ctx, double* max_norm_critic, double* max_norm_actor);
enum sacmi_gnorm { SACMI_GNORM_Q1 = 0, SACMI_GNORM_Q2 = 1, SACMI_GNORM_PI = 2, SACMI_GCOEF_Q1 = 3,
                   SACMI_GCOEF_Q2 = 4, SACMI_GCOEF_PI = 5, SACMI_GNORM_COUNT = 6 };
/* as sacmi_fetch_stats: synchronises, most recent min(total, 4096, max_rows) rows oldest first */
int sacmi_fetch_grad_norms(sacmi_ctx* ctx, float* out, int32_t max_rows, int32_t* n_out, int64_t* total);

/* ---- running observation normalisation ------------------------------------------------ */
/* The running mean / variance normaliser with clipping of the mainstream SAC stacks, with their
 * semantics: the ring stores RAW observations; they are normalised where they are consumed — at
 * sample time in the update's gather and at act time in sacmi_act — with the statistics current
 * then.  The reference has none (replay_buffer.py:73).
 *
 * Running moments, per context, on the device, all fp64: count, mean[S] and M2[S] (the sum of
 * squared deviations of column k from its mean).  They are updated from the state s of every
 * transition a push actually stores (not s2; not the rows a push of more than `capacity` rows
 * skips; sacmi_replay_clear leaves them alone) and from the rows handed to
 * sacmi_obs_norm_update.  Each chunk of at most 1024 rows that reaches the device is merged
 * into them (per-row Welford steps, Chan's merge; never E[x^2] - mean^2) in a fixed order
 * without atomics: the same pushes from the same state give the same bits.
 *
 * Derived fp32 vectors, recomputed on the device whenever the moments or eps change:
 *     nmean[k] = (float)mean[k]
 *     nrstd[k] = (float)(1.0 / sqrt(M2[k] / count + eps))     population variance, fp64
 * count == 0 is the identity (mean 0, scale 1).  (eps = 0 on a constant column gives an
 * infinite scale and NaN rows: keep eps > 0.)
 *
 * The normalisation, one device function for every consumer, in fp32:
 *     t = (x - nmean[k]) * nrstd[k]
 *     y = t < -clip ? -clip : (t > clip ? clip : t)            a NaN stays a NaN
 * applied to s and s2 of every gathered row and to the states of sacmi_act; the actions,
 * rewards and done flags are untouched.  Under bf16 activations y is rounded to bf16 once,
 * after normalising.  A NaN observation still surfaces as SACMI_ENAN from the policy sample.
 *
 * mode 0: off (default; the update's launches are exactly those of a context that never called
 * this).  1: on, pushes update the moments.  2: on, frozen: pushes leave the moments alone
 * (sacmi_obs_norm_update still counts).  eps >= 0 and finite, clip > 0 or +inf (no clipping),
 * else SACMI_EVALUE.  On / off selects another captured graph; 1 <-> 2, the moments, eps and clip
 * are stream-ordered device state: changing them re-captures nothing.  Switching off keeps the
 * moments.
 *
 * On, the minibatch is gathered by a launch of its own in every update: no gather rides along
 * in another update's launches and no batch is drawn ahead (sacmi_step_ride_possible reports
 * 0), and while mode is 1 every pushed row takes the chunked device path (the push mailbox is
 * bypassed).  sacmi_step_phase, sacmi_step_phase_ex and sacmi_step_dp return SACMI_ESTATE
 * before touching state: each rank's shard would grow statistics of its own, and a collective
 * over the moments is not built.
 *
 * SACMI_OBS_NORM=1 in the environment at sacmi_create selects mode 1 with eps 1e-8 and clip 10.
 * Additive: the ABI version is unchanged. */
int sacmi_set_obs_norm(sacmi_ctx* ctx, int32_t mode, double eps, double clip);
int sacmi_obs_norm(sacmi_ctx* ctx, int32_t* mode, double* eps, double* clip);
/* states [n][S] f32 into the moments; any mode but off (SACMI_ESTATE), "frozen" included */
int sacmi_obs_norm_update(sacmi_ctx* ctx, const float* states, int64_t n);
/* Synchronises the stream.  mean, m2: [S] f64, S = state_dim (else SACMI_EVALUE). */
int sacmi_obs_norm_get_moments(sacmi_ctx* ctx, double* count, double* mean, double* m2, int32_t S);
/* count < 0, m2 < 0, a non-finite value or a wrong S: SACMI_EVALUE.  Works in every mode. */
int sacmi_obs_norm_set_moments(sacmi_ctx* ctx, double count, const double* mean, const double* m2,
                               int32_t S);
/* nmean, nrstd [S] f32 as the gather reads them (synchronises) */
int sacmi_obs_norm_get_vectors(sacmi_ctx* ctx, float* nmean, float* nrstd, int32_t S);

/* ---- n-step returns in the replay gather ------------------------------------------------ */
/* Multi-step targets, made where the minibatch is gathered, from the ring as it is at sample
 * time: nothing is stored per row, pushes are not delayed, and the return follows the ring's
 * current contents.  The reference bootstraps one step ahead (sac_imp.py:86-93).
 *
 * n = steps, 1 <= n <= 32 (else SACMI_EVALUE); n = 1 is off (default; the update's launches are
 * exactly those of a context that never called this).  g[j] = (float)(gamma ** j), j = 0..31,
 * computed on the host in fp64 and rounded once (g[0] = 1).
 *
 * For a sampled row at deque position i (prioritized contexts: ring slot p0, i = (p0 - head +
 * capacity) % capacity) the chain is p_j = (p0 + j) % capacity, j = 0, 1, ...  Row p_j stops it
 * if done[p_j] != 0, or its episode-end flag is set (below), or j == min(n - 1, len - 1 - i):
 * the chain never passes the newest row, so it never wraps onto the oldest.  m = the smallest
 * stopping j.  Then, in fp32 with every operation rounded on its own (no contraction),
 *     R  = r_0;  for j = 1..m in that order:  R = R + g[j] * r_j
 *     d' = done[p_m] != 0 ? 1 : (m == 0 ? 0 : 1 - g[m])
 * and the gathered row is s, a from p0, r[b] = R, s2 from p_m, d[b] = d'.  A row with m == 0
 * is bit for bit the one-step row.  A chain ended by a flag with done == 0 bootstraps from that
 * row's s2 (a time-limit truncation).  A NaN reward propagates into R as it would into r.
 *
 * Nothing downstream of the gather changes: the row algebra computes fl(fl(1 - d') * gamma) *
 * min(q1t, q2t) as before, which DEFINES the effective bootstrap coefficient.  For g[m] >= 0.5
 * both subtractions are exact and it is fl(g[m] * (float)gamma); below that it is within about
 * 2 ulp of gamma^(m+1) (documented, not a defect).  The diagnostics and the prioritized
 * feedback's TD errors are then the n-step ones.
 *
 * Episode boundaries: the ring keeps one flag byte per slot.  While n >= 2 EVERY stored row
 * writes its flag, 0 or 1 (sacmi_push / sacmi_push_packed write 0), so an evicted row's flag is
 * overwritten with its slot; switching on from off clears all flags (stream-ordered).
 * sacmi_push_ep / sacmi_push_packed_ep are sacmi_push / sacmi_push_packed with end: [n] u8 or
 * NULL (all 0); sacmi_mark_episode_end sets the flag of the newest stored row (a trainer that
 * learns of a time-limit cut only after the push).  All three return SACMI_ESTATE while off
 * (unless the return statistics of sacmi_set_reward_norm take the flags, modes 1 and 2);
 * sacmi_mark_episode_end also with an empty replay.  A terminal row needs no flag.
 *
 * On / off selects another captured graph; the value of n and the table are stream-ordered
 * device state: changing n among values >= 2 re-captures nothing.  On, the minibatch is
 * gathered by a launch of its own in every update (k_gather_nstep): no gather rides along and no
 * batch is drawn ahead (sacmi_step_ride_possible reports 0; sacmi_step_phase_ex with ride_next
 * returns SACMI_ESTATE), and every pushed row takes the chunked device path (the push mailbox is
 * bypassed).  The phase-split and data-parallel updates stay allowed: the chain is local to a
 * rank's own ring.  Composes with observation normalisation (s from p0 and s2 from p_m are
 * normalised), staged indices, prioritized replay and its feedback mode.
 *
 * SACMI_NSTEP=<n> in the environment at sacmi_create switches it on from the start.
 * Additive: the ABI version is unchanged. */
int sacmi_set_nstep(sacmi_ctx* ctx, int32_t n);
int sacmi_nstep(sacmi_ctx* ctx, int32_t* n);
int sacmi_push_ep(sacmi_ctx* ctx, const float* s, const float* a, const float* r,
                  const float* s2, const uint8_t* d, const uint8_t* end, int64_t n);
int sacmi_push_packed_ep(sacmi_ctx* ctx, const float* rows, const uint8_t* end, int64_t n);
int sacmi_mark_episode_end(sacmi_ctx* ctx);
/* The flags of rows idx[n] (deque positions, or ring slots with by_slot), for checkpoints;
 * all 0 while off.  Synchronises. */
int sacmi_get_episode_ends(sacmi_ctx* ctx, const int64_t* idx, int64_t n, int32_t by_slot, uint8_t* out);
/* Test hooks: r[batch], d[batch] of minibatch set 0 as the last update's gather left them (as
 * sacmi_read_batch); raw fp32 values into the ring's done array at ring slots. */
int sacmi_read_batch_rd(sacmi_ctx* ctx, int32_t batch, float* r, float* d);
int sacmi_debug_set_done(sacmi_ctx* ctx, const int64_t* slots, const float* values, int64_t n);

/* ---- reward scaling and running return normalisation ---------------------------------- */
/* A constant reward scale (the SAC paper's one sensitive hyperparameter) and the running return
 * normaliser of the mainstream stacks (the norm_reward of a VecNormalize wrapper): the reward is
 * divided by the running standard deviation of the discounted return, then clipped.  As with
 * the observations, the ring stores RAW rewards; they are normalised where they are consumed,
 * at sample time, with the statistics current then.  The reference has neither.
 *
 * State, per context, on the device, all fp64: ret, the running discounted return of the
 * episode being pushed, and count, mean, M2 (the sum of squared deviations from the mean) of
 * the ret values seen.  With g64 = (double)cfg.gamma, for every transition a push actually
 * stores, in push order (ONE environment stream: consecutive rows are consecutive steps),
 *     ret = fl64(fl64(ret * g64) + (double)r_i)         two roundings, never contracted
 *     (count, mean, M2) take ret                         Welford steps, Chan's merge
 *     if d_i != 0 or end_i: ret = 0
 * end_i is the row's episode-end flag (below).  A push of more than `capacity` rows counts only
 * the rows it stores, and ret is reset to 0 before the first of them.  sacmi_replay_clear
 * leaves the state alone.  Each chunk of at most 1024 rows that reaches the device is merged in
 * a fixed order without atomics, every word with one writer (never E[x^2] - mean^2): the same
 * pushes from the same state give the same bits.
 *
 * Factor, one fp32 value, recomputed on the device whenever the state, scale or eps changes:
 *     k = (float)(scale / sqrt(M2 / count + eps))       fp64, rounded once; modes 1 and 2, count > 0
 *     k = (float)scale                                  mode 3, or count == 0
 * (eps = 0 with all returns equal gives an infinite k: keep eps > 0.)
 *
 * Normalisation, one device function, in fp32:
 *     t = r * k                                         one rounding
 *     y = t < -clip ? -clip : (t > clip ? clip : t)     compares: a NaN stays a NaN
 * applied to the gathered reward of every minibatch row, by one small launch of its own in every
 * update behind whatever produced the minibatch (k_reward_norm, out of place).  With n-step
 * returns on it is applied to the collapsed return R: the clip then bounds R * k, not each
 * step's reward.  States, actions and d are untouched.  Everything downstream is then in
 * normalised units, exactly as if the user had pushed such rewards: the Q values, the
 * diagnostics' REWARD_MEAN, Q_* and TD_*, the prioritized feedback's priorities and the gradient
 * norms.  A NaN reward stays a NaN in the row; in mode 1 it also enters ret and the moments,
 * after which k is NaN until sacmi_reward_norm_set_state replaces them.
 *
 * mode 0: off (default; the update's launches are exactly those of a context that never called
 * this).  1: running: pushes update the state.  2: frozen: pushes leave the whole state alone,
 * ret included.  3: constant scale only: no state is kept, k = (float)scale.  scale > 0 and
 * finite, eps >= 0 and finite, clip > 0 or +inf (no clipping), else SACMI_EVALUE.  On / off
 * selects another captured graph; the mode among 1 / 2 / 3, the state, scale, eps and clip are
 * stream-ordered device or host state: changing them re-captures nothing.  Switching modes
 * leaves the state alone.  Every call here that changes what the normalisation would read gives
 * up a batch drawn ahead.
 *
 * The gathers are unchanged: they ride along and are drawn ahead as without the feature
 * (sacmi_step_ride_possible reports what it reports for a context that never enabled it).
 * While the mode is 1 every pushed row takes the chunked device path (the push mailbox is
 * bypassed; rows already pending are flushed first, uncounted); modes 2 and 3 keep the mailbox.
 *
 * Episode ends: in modes 1 and 2 sacmi_push_ep, sacmi_push_packed_ep and sacmi_mark_episode_end
 * are accepted even while n-step returns are off.  The flags then feed only the return reset:
 * the ring's flag bytes are still not kept and sacmi_get_episode_ends still reports zeros.
 * sacmi_mark_episode_end also sets ret = 0, stream-ordered (modes 1 and 2).  With n-step off
 * and this mode 0 or 3 the three calls return SACMI_ESTATE as before.
 *
 * In any mode but 0, sacmi_step_phase, sacmi_step_phase_ex and sacmi_step_dp (loopback
 * included) return SACMI_ESTATE before touching state: rank-local statistics would need a
 * collective that is not built.  (The constant-scale data-parallel case needs none; it is the
 * follow-up.)
 *
 * SACMI_REWARD_NORM=1 in the environment at sacmi_create selects mode 1 with scale 1, eps 1e-8
 * and clip 10; SACMI_REWARD_SCALE=<x> sets the scale, and on its own selects mode 3 with clip
 * +inf.  Additive: the ABI version is unchanged. */
int sacmi_set_reward_norm(sacmi_ctx* ctx, int32_t mode, double scale, double eps, double clip);
int sacmi_reward_norm(sacmi_ctx* ctx, int32_t* mode, double* scale, double* eps, double* clip);
/* Synchronises the stream.  All zero on a context that never switched the feature on. */
int sacmi_reward_norm_get_state(sacmi_ctx* ctx, double* count, double* mean, double* m2, double* ret);
/* count < 0, m2 < 0 or a non-finite value: SACMI_EVALUE.  Works in every mode. */
int sacmi_reward_norm_set_state(sacmi_ctx* ctx, double count, double mean, double m2, double ret);
/* the factor k as k_reward_norm reads it (synchronises) */
int sacmi_reward_norm_get_factor(sacmi_ctx* ctx, float* k);
/* Test hook: the normalised r[batch] of minibatch set 0 as the last update left it;
 * sacmi_read_batch_rd keeps returning the raw gathered r. */
int sacmi_read_batch_rn(sacmi_ctx* ctx, int32_t batch, float* rn);

/* Data-parallel split of the step (one process per GPU).  phase 0: sample, gather,
 * forward, critic backward -> critic gradient buffer; phase 1: critic Adam + Polyak,
 * actor forward/backward -> actor gradient buffer; phase 2: actor Adam + alpha;
 * phase 3: phase 2 of the previous update then phase 0 of the next, in one launch
 * (no collective sits between them).
 * Between phases the caller all-reduces (sum) the buffer named by
 * sacmi_grad_buffer(which=0 critic, 1 actor); grad_scale (1/world) is applied by the
 * Adam kernels. */
int sacmi_step_phase(sacmi_ctx* ctx, int32_t batch, int32_t phase, float grad_scale);
/* The same with the minibatch buffer sets spelled out, for a fixed sequence of split
 * updates (e.g. one captured into a graph by the caller): parity (0/1) = the buffer set
 * of the update whose phase 0 (phase 3: the NEXT update) / phase 1 runs; have_batch =
 * its indices and rows were produced by the previous update (phases 0, 3); ride_next =
 * the phase-1 launches also sample and gather the next update into set parity^1
 * (uniform replay only, sacmi_step_ride_possible).  The caller guarantees that nothing
 * changes the replay buffer or the sampling stream between a ride and its use. */
int sacmi_step_phase_ex(sacmi_ctx* ctx, int32_t batch, int32_t phase, float grad_scale,
                        int32_t parity, int32_t have_batch, int32_t ride_next);
int sacmi_step_ride_possible(sacmi_ctx* ctx, int32_t batch, int32_t* out);
/* 1 when updates of this batch store their activations as bf16 (compute_dtype bf16 at the
 * batch-4096 class: hidden layers, minibatch rows and sampled actions; the policy heads
 * then read a bf16-rounded input), else 0. */
int sacmi_step_act16(sacmi_ctx* ctx, int32_t batch, int32_t* out);
/* Test hook: the hidden activations (post-ReLU) the last update of `batch` rows left in
 * HBM, hidden layer `layer` (0-based) of pass
 *   0  the critics on (s, a)            -> [2][batch][hidden]  (q1, then q2)
 *   1  the target critics on (s', a')   -> [2][batch][hidden]
 *   2  the updated critics on (s, a~)   -> [2][batch][hidden]
 *   3  the policy on [s' ; s]           -> [2 * batch][hidden]
 * (numel = 2 * batch * hidden).  Their signs are the ReLU masks the update's backward used:
 * the parity tests recompute the fp64 gradient under the GPU's own masks.  bf16-stored
 * activations (sacmi_step_act16) come back widened to fp32 (bits << 16: the exact stored
 * values), in the same layout. */
int sacmi_read_activation(sacmi_ctx* ctx, int32_t pass, int32_t layer, int32_t batch, float* out,
                          int64_t numel);
/* Test hook (read-only: synchronises the stream and copies, launches nothing): an fp32
 * backward buffer as the last update of `batch` rows left it in HBM.  `layer` is the hidden
 * layer (0-based) of the per-layer buffers, 0 for the others.
 *   DHC   [batch][2 * hidden]  dL/dh of the critics on (s, a), q1 | q2 side by side; for the
 *         last hidden layer the coefficient-free rows u = [h > 0] w_head the row-prologue
 *         level (L5) stored for that layer's weight gradient (dh = u * dq)
 *   DHA   the same of the updated critics on (s, a~) (the last hidden layer's is never written)
 *   DHP   [batch][hidden]      dL/dh of the policy's actor rows
 *   DQ    [2][batch]           dL/dq_i = 2 (q_i - q^) / batch
 *   DQ4   [2 * batch][4]       the same, one value per 16-byte row (pads 0)
 *   DHEAD [batch][2 * action_dim]  dL/d(mean | log_std)
 *   DOTP  [6][batch][(hidden + 31) / 32]  the critic head dot partials per 32-column block
 *         (block 0 carries the head bias): slots 0/1 q1/q2 on (s, a), 2/3 the targets, 4/5
 *         the updated critics on (s, a~); a row's head value is their fp32 sum in block order
 * Additive: the ABI version is unchanged. */
enum sacmi_backward_buf { SACMI_BWD_DHC = 0, SACMI_BWD_DHA = 1, SACMI_BWD_DHP = 2, SACMI_BWD_DQ = 3,
                          SACMI_BWD_DQ4 = 4, SACMI_BWD_DHEAD = 5, SACMI_BWD_DOTP = 6 };
int sacmi_read_backward(sacmi_ctx* ctx, int32_t which, int32_t layer, int32_t batch, float* out,
                        int64_t numel);
/* Test hook (read-only: synchronises the stream and copies, launches nothing, and leaves the
 * context's own bookkeeping alone): the five host-mapped words of the synchronous step —
 * out[0..2] the bits of {q1_loss, q2_loss, policy_loss}, out[3] the error bits, out[4] the done
 * counter.  They are maintained by the synchronous forms only (sacmi_step, sacmi_step_launch /
 * _wait): sacmi_step_async, sacmi_step_many_async and the one-rank sacmi_step_dp store none of
 * them.  Additive: the ABI version is unchanged. */
int sacmi_debug_host_words(sacmi_ctx* ctx, uint32_t out[5]);
/* Test hook: the minibatch of the last device-sampled update of `batch` rows that used batch
 * set 0 (every single update, and the first of a multi-update graph): its replay indices
 * (idx[batch]: deque positions, or ring slots for PER) and the policy noise it drew
 * (eps[2 * batch * action_dim]: rows [0, batch) for policy.sample(next_state), rows [batch,
 * 2 batch) for policy.sample(state), sac_imp.py:89,116). */
int sacmi_read_batch(sacmi_ctx* ctx, int32_t batch, int64_t* idx, float* eps, int64_t eps_numel);
/* The gradient range a phase-split update's collective covers, in the gradient arena:
 * which = 0 the critic range [q1 | q2] FOLLOWED BY 4 error-flag floats (kDpFlagN: flag 0 =
 * this update saw a skip-all non-finite input, flag 1 = an actor-batch one, 2-3 zero) — they
 * travel with the critic all-reduce so that every rank voids the same steps; a grad norm or
 * clip over this view must exclude the last 4 floats.  which = 1 the actor range [policy |
 * log_alpha]. */
int sacmi_grad_buffer(sacmi_ctx* ctx, int which, void** device_ptr, int64_t* numel);
/* Gradient arena size (floats) and adoption of a caller-allocated device buffer of
 * that size (e.g. a torch tensor), so collectives run on it in place.  Must be on the
 * context's device and stay alive for the context's lifetime. */
int sacmi_grad_arena_numel(sacmi_ctx* ctx, int64_t* numel);
int sacmi_attach_grad_arena(sacmi_ctx* ctx, void* device_ptr, int64_t numel);

/* ---- native data parallel (RCCL over xGMI, no host framework) ------------------------ */
/* The same split update with the two gradient all-reduces issued by the library itself
 * (SURVEY §8(b) sacmi_allreduce_init; sac_imp.py:101-125 is the single-process update it
 * distributes).  One process per GPU: rank 0 creates the RCCL unique id
 * (sacmi_allreduce_unique_id, SACMI_RCCL_ID_BYTES bytes) and hands it to every rank by any
 * host channel; each rank then calls sacmi_allreduce_init on its context.  RCCL is loaded
 * at run time (dlopen: the process's already-loaded librccl if any, else
 * $SACMI_RCCL_PATH, else librccl.so.1): libsacmi itself has no link dependency on it. */
#define SACMI_RCCL_ID_BYTES 128
int sacmi_allreduce_unique_id(void* id_out, int32_t nbytes);
int sacmi_allreduce_init(sacmi_ctx* ctx, const void* id, int32_t nbytes, int32_t rank,
                         int32_t world);
/* n_updates complete data-parallel updates (every rank the same n): per update phase 0
 * (phase 3 after the first), all-reduce(sum) of the critic gradients, phase 1,
 * all-reduce of [actor gradients | dL/dlog_alpha], the last phase 2 at the end; updates
 * 2..n take their minibatch from the previous update's ride-along sampling/gather when
 * the replay allows it.  Captured into one hipGraph per (batch, n_updates); losses land in
 * the loss ring (sacmi_fetch_losses).  Each rank samples its own replay shard.
 * Sharded form (opt-in, 2 <= world <= 64: $SACMI_DP_SHARD=1 at sacmi_allreduce_init or
 * sacmi_dp_set_sharded): each all-reduce + Adam becomes reduce-scatter -> Adam on
 * this rank's 1/world chunk of the range -> all-gather of the parameters (ZeRO-1: the Adam
 * moments stay valid on the rank's own chunks; sacmi_dp_sync_state gathers them).
 * world == 1: the fused update (nothing to reduce; $SACMI_DP_PHASES_AT_WORLD1 forces the
 * phase sequence). */
int sacmi_step_dp(sacmi_ctx* ctx, int32_t batch, int32_t n_updates);
/* Sharded (1) or all-reduce (0) form of sacmi_step_dp; the same on every rank.  Leaving
 * the sharded form is a collective (every rank): it gathers the Adam moments first, as
 * sacmi_dp_sync_state does, since the all-reduce form steps every element from them. */
int sacmi_dp_set_sharded(sacmi_ctx* ctx, int32_t on);
int sacmi_dp_sharded(sacmi_ctx* ctx, int32_t* on);
/* Collective (every rank): all-gather the sharded Adam moments so that every rank holds
 * them whole (before sacmi_get_tensor of SACMI_SLOT_ADAM_M / _V, a checkpoint).  No-op
 * when not sharded. */
int sacmi_dp_sync_state(sacmi_ctx* ctx);
/* Test hook for the sequence above on ONE context, no RCCL: every all-reduce becomes an
 * in-place x world over the same gradient range — what `world` ranks holding identical
 * shards would reduce to — while the Adam kernels apply 1/world as in a real run.  For a
 * power-of-two world both scalings are exact, so sacmi_step_dp must equal the fused
 * updates bit for bit: every gradient element, dL/dlog_alpha included, must sit inside an
 * all-reduced range and 1/world must be applied exactly once. */
int sacmi_dp_loopback_init(sacmi_ctx* ctx, int32_t world);
/* (Sharded form under loopback: the gradients x world in place, Adam on every rank's chunk
 * in turn — rank 0's launch alone finalising the losses — and the gather an identity.) */

/* ---- prioritized replay ------------------------------------------------------------ */
/* PrioritizedReplayBuffer.sample(batch) indices + IS weights; u: NULL -> draw from
 * MT stream 1 on device, else [min(batch,len)] uniforms in [0,1).  Advances frame. */
int sacmi_per_sample(sacmi_ctx* ctx, int32_t batch, const double* u, int64_t* idx_out,
                     float* weights_out);
/* priorities[idx[i]] = values[i] in order i = 0..n-1 (last duplicate wins), where the
 * caller passes the reference's stored value float32(float(p) + 1e-6)
 * (replay_buffer.py:87; the +1e-6 is a double add, done host-side). */
int sacmi_per_update(sacmi_ctx* ctx, const int64_t* idx, const float* values, int64_t n);
int sacmi_per_get_priorities(sacmi_ctx* ctx, float* out, int64_t n);
/* Feedback mode of a prioritized context (off at creation; SACMI_ESTATE on a uniform one).
 * On, every device-sampled update is the loop a user would write against the buffer API:
 *     s, a, r, s2, d, idx, w = buffer.sample(B)
 *     q_i_loss = mean(w * (q_i(s, a) - q^) ** 2)           i = 1, 2
 *     td       = 0.5 * (|q1 - q^| + |q2 - q^|)             fp32, per row
 *     buffer.update_priorities(idx, td)                    stored: float32(float64(td) + 1e-6)
 * with the write-back on the device, inside the update (last duplicate wins; the actor and
 * alpha blocks are not weighted; the q losses returned are the weighted ones).  An update
 * voided by a non-finite sample (SACMI_ENAN) writes no priority; a non-finite td is written
 * as it is, and the next draw reports "probabilities contain NaN" (inside a multi-update launch
 * that draw runs beside the update that produced the td, whose remaining steps may or may
 * not stand: n updates in one launch equal n launches bit for bit for finite td only).  With
 * feedback on, an update with staged indices, the phase-split updates and sacmi_step_dp return
 * SACMI_ESTATE before they touch any state.
 * Additive: the ABI version is unchanged. */
int sacmi_per_set_feedback(sacmi_ctx* ctx, int32_t on);
int sacmi_per_feedback(sacmi_ctx* ctx, int32_t* on);
/* Test hook (feedback mode), for the last device-sampled update of `batch` rows on batch set
 * 0 (as sacmi_read_batch): the importance-sampling weights it used, the td it computed and
 * the priorities it stored, [batch] each (any may be NULL). */
int sacmi_read_per_feedback(sacmi_ctx* ctx, int32_t batch, float* weights, float* td,
                            float* stored);
int sacmi_per_set_priorities(sacmi_ctx* ctx, const float* in, int64_t n);

/* ---- action selection (sac_imp.py:54-72) ----------------------------------------- */
/* n states [n,S] -> actions [n,A]; deterministic: tanh(mean)*scale+bias;
 * else policy.sample with eps [n,A] (NULL -> Philox). */
int sacmi_act(sacmi_ctx* ctx, const float* s, int32_t n, int32_t deterministic,
              const float* eps, float* a_out);

/* ---- diagnostics ------------------------------------------------------------------ */
/* Run `iters` eager (non-graph) updates with a HIP event recorded on the context's
 * stream between consecutive kernel launches; returns, per launch site, its name
 * (32 bytes each, NUL-padded), the mean duration in ms and the algorithmic FLOPs of
 * one launch (GEMM sites; 0 elsewhere).  The model state advances as in sacmi_step. */
int sacmi_profile_step(sacmi_ctx* ctx, int32_t batch, int32_t iters, char* names_out,
                       float* ms_out, double* flops_out, int32_t max_sites, int32_t* n_sites);
/* Per launch site of the single-GPU update: that site's kernels alone, `reps` times
 * back to back inside one hipGraph, timed with HIP events on the context's stream;
 * us_out = mean microseconds per launch of the site (the duration the kernel has in
 * the step's graph, boundary included); flops_out / bytes_out (may be NULL) = the
 * algorithmic FLOPs / bytes of one launch (GEMM sites; 0 elsewhere).  Diagnostic:
 * every replay advances the model state again (Adam sites take `reps` extra steps). */
int sacmi_profile_sites(sacmi_ctx* ctx, int32_t batch, int32_t reps, char* names_out,
                        float* us_out, double* flops_out, double* bytes_out, int32_t max_sites,
                        int32_t* n_sites);

/* Launch timeline of the real update: n_updates consecutive updates exactly as
 * sacmi_step_many_async runs them (device sampling + noise, ride-along sampling, one
 * hipGraph), captured with every kernel stamping its first workgroup's entry and its last
 * workgroup's exit on the GPU's 100 MHz real-time clock.  Replayed once to warm up, then
 * once measured; returns per kernel launch, in launch order: the launch site's name (32
 * bytes, NUL-padded), the kernel kind (TlKind in csrc/sacmi_internal.h), its grid, the
 * site index (sites count across updates), start / end in microseconds from the first
 * kernel's start, the site's algorithmic FLOPs / bytes (GEMM sites, on the site's first
 * kernel; may be NULL); graph_us = HIP-event time of the measured replay.  Diagnostic: the model
 * state advances by 2 * n_updates updates. */
int sacmi_profile_timeline(sacmi_ctx* ctx, int32_t batch, int32_t n_updates, int32_t max_kernels,
                           char* names_out, int32_t* kind_out, int32_t* grid_out, int32_t* site_out,
                           double* start_us, double* end_us, double* flops_out, double* bytes_out,
                           int32_t* n_kernels, double* graph_us);

/* The timeline of ONE real launch: sacmi_step_many_async(batch, n_updates) as it would run
 * now, captured with the stamps and launched once (no warm-up replay).  It takes a batch the
 * previous launch drew ahead (then it has no sampler / gather launch of its own) and draws the
 * next launch's, exactly as that call does: the state advances by n_updates updates, bit for
 * bit as sacmi_step_many_async's.  Outputs as sacmi_profile_timeline. */
int sacmi_profile_launch_timeline(sacmi_ctx* ctx, int32_t batch, int32_t n_updates, int32_t max_kernels,
                                  char* names_out, int32_t* kind_out, int32_t* grid_out, int32_t* site_out,
                                  double* start_us, double* end_us, double* flops_out, double* bytes_out,
                                  int32_t* n_kernels, double* graph_us);

/* sacmi_profile_timeline over the data-parallel sequence sacmi_step_dp replays (phases +
 * the two RCCL all-reduces of every update; needs sacmi_allreduce_init, and every rank of
 * the communicator must make the same call, since the captured graph holds the
 * collectives).  The all-reduces launch no stamping kernel: their time is the gap before
 * the next kernel's start. */
int sacmi_profile_timeline_dp(sacmi_ctx* ctx, int32_t batch, int32_t n_updates, int32_t max_kernels,
                              char* names_out, int32_t* kind_out, int32_t* grid_out, int32_t* site_out,
                              double* start_us, double* end_us, double* flops_out, double* bytes_out,
                              int32_t* n_kernels, double* graph_us);

/* Host-only self test of the launch validator every GEMM level passes before it is
 * enqueued (operand spans against the registered device allocations, incl. the bf16
 * weight shadows and the split-K workspace): runs a fixed set of accept / reject cases
 * on host arrays; n_passed == n_cases when the validator decides each one correctly.
 * Needs no device. */
int sacmi_selftest_span_checker(int32_t* n_cases, int32_t* n_passed);

#ifdef __cplusplus
}
#endif
#endif /* SACMI_H_ */
