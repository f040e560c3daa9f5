/*
 * orl_engine.h — C ABI of the MI355X-native offline-RL update engine.
 *
 * This is the drop-in boundary for the policy.learn() hot path of the
 * reference (zhaoyizhou1123/OfflineRL-Kit).  The reference has no FFI layer:
 * its boundary is the duck-typed Python interface
 *     BasePolicy.learn(batch) -> Dict[str,float]   (offlinerlkit/policy/base_policy.py:8-26)
 *     ReplayBuffer.sample(batch_size) -> Dict      (offlinerlkit/buffer/buffer.py:96-106)
 *     MFPolicyTrainer.train()                      (offlinerlkit/policy_trainer/mf_policy_trainer.py:41-90)
 * Each entry point below names the reference code it replaces.  Signatures
 * are plain C: pointers, sizes, no torch types.  The Python mirror
 * (offlinerl-kit_amd/offlinerlkit) binds them with ctypes; INTEGRATION.md shows
 * the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returning int returns 0 on success, non-zero on error;
 *     the message is available from orl_last_error() (thread-local).
 *   - one engine = one device + one HIP stream; an engine is not thread-safe.
 *   - an engine carries `n_runs` independent runs (seeds) that are updated
 *     together by every kernel launch (run-batched, like an ensemble).  All
 *     host-side arrays have a leading run dimension [n_runs][...].
 *   - all floating point is fp32.  `precision` selects the MFMA scheme used by
 *     the GEMMs only: 0 = exact fp32 MFMA (v_mfma_f32_16x16x4_f32),
 *     1 = split operands: every operand as hi + lo 16-bit planes (IEEE half:
 *     22 significand bits per operand, power-of-two operand scales folded back
 *     into the fp32 accumulators), 3 MFMAs per product, fp32 accumulate;
 *     orl_split_bits() reports the operand width of the loaded build (22; 16
 *     for the bf16-plane variant build).  In this mode hidden activations
 *     and inputs must stay below 65504 in magnitude (fp16 range) and weights
 *     below 1023 (they enter the products times 2^6): see orl_health.
 *     2 = three fp16 planes per operand (hi + mid + lo = 33 significand bits:
 *     an fp32 operand is represented exactly) and the six products down to
 *     2^-33 with fp32 accumulation -- the arithmetic class of the fp32 MFMA at
 *     more than its rate -- in the launches that have such a flavour: the
 *     weight-stationary forward / dgrad / wgrad launches of nets with
 *     256-wide hidden layers from 4096 batched rows (CQL's dominant launches
 *     at two and three hidden layers, the 256-row phases of CQL / IQL /
 *     TD3+BC / SAC at many runs, the forwards and dgrads of EDAC's ensemble
 *     critics); every other launch (tiled and few-row passes) runs the
 *     precision-0 kernels.  The fp16 operand range of
 *     precision 1 applies to those launches.
 *   - orl_step / orl_learn_n additionally return ORL_RC_UNHEALTHY (1) when the
 *     step(s) ran but a run's health flag is raised (non-finite loss or
 *     gradient, an operand beyond the split-precision range): results are
 *     delivered, orl_last_error() describes the runs, orl_health() has the flags.
 */
#ifndef ORL_ENGINE_H
#define ORL_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORL_ALGO_CQL 0   /* policy/model_free/cql.py:87-207   */
#define ORL_ALGO_IQL 1   /* policy/model_free/iql.py:86-139   */
#define ORL_ALGO_TD3BC 2 /* policy/model_free/td3bc.py:83-124 */
#define ORL_ALGO_EDAC 3  /* policy/model_free/edac.py:88-166  */
#define ORL_ALGO_SAC 4   /* policy/model_free/sac.py:88-140 (MOPOPolicy.learn on the real+model batch, model_based/mopo.py:81-84) */
#define ORL_ALGO_MCQ 5   /* policy/model_free/mcq.py:48-126 (SAC critics / actor + the VAE behaviour policy of nets/vae.py) */
#define ORL_ALGO_MOBILE 6 /* policy/model_based/mobile.py:130-196 (SAC schedule + the model-Bellman-inconsistency penalty; needs orl_engine_set_next_samples) */
#define ORL_ALGO_RCSL 7   /* policy/rcsl/rcsl.py:123-151: one net (ORL_NET_ACTOR) = MLP(obs_dim + 1, hidden, act_dim) of modules/rcsl_module.py, MSE on the
                           * dataset action, Adam with actor_lr / ORL_OPT_ACTOR; metric "loss".  The return-to-go travels where the other algorithms
                           * carry the reward: orl_batch.rewards and the `rew` column of an orl_buffer */
#define ORL_ALGO_RCSL_GAUSS 8 /* policy/rcsl/rcsl_gauss.py:123-154: ORL_NET_ACTOR = MLP(obs_dim + 1, hidden, act_dim) -> z, then DiagGaussian(act_dim, act_dim,
                           * unbounded, conditioned_sigma) of modules/dist_module.py:45-93: mu = W_mu z + b_mu, s = clamp(W_sigma z + b_sigma, -5, 2),
                           * loss = mean((mu - a)^2 exp(-s)) + mean(s), Adam with actor_lr / ORL_OPT_ACTOR; metric "loss".  Inputs, buffers, orl_learn_epoch
                           * and every refusal as for ORL_ALGO_RCSL */
#define ORL_ALGO_AUTOREG 9 /* policy/others/autoregressive.py:9-124: p(a | s) = prod_j N(a_j | s, a_<j).  ORL_NET_ACTOR = [Linear, LeakyReLU(0.01)] x (L + 1):
                           * Linear(obs_dim + 2 act_dim, h0), ..., Linear(h_{L-1}, 2), tensors model.{0, 2, ..., 2L}.{weight, bias}; act_dim <= 32.  A batch
                           * row b becomes act_dim input rows j * B + b = [obs | act[k] 1[k < j] | onehot_j] with target act[j]; (mean, logstd) = the two
                           * (activated) outputs, loss = mean Gaussian NLL over the expanded rows, Adam with actor_lr / ORL_OPT_ACTOR; metric "loss".
                           * Buffers, orl_learn_n, orl_learn_epoch and the refusals as for ORL_ALGO_RCSL, but no return-to-go is read:
                           * orl_batch.rewards may be NULL and a buffer's `rew` column is not range-checked.  Sampling: orl_autoreg_sample */

/* per-run health flags (orl_health).  The reference raises nothing when a run diverges (its losses simply turn nan); here a diverging run
 * can additionally be MASKED by the arithmetic -- the ReLU of the matrix kernels works on the integer view of the activations and maps a NaN
 * whose sign bit is set to +0, and at precision 1 an operand beyond the fp16-plane range multiplies to NaN -- so the engine watches for it. */
#define ORL_HEALTH_NONFINITE_LOSS 1 /* a metric of a step (loss, alpha, Q statistic) was inf / nan */
#define ORL_HEALTH_NONFINITE_GRAD 2 /* a summed parameter gradient was inf / nan when Adam consumed it */
#define ORL_HEALTH_SPLIT_RANGE 4    /* precision 1: an input, stored hidden activation (|x| >= 65504) or weight (|w| >= 65504 / 2^6) is out of the operand range */
#define ORL_RC_UNHEALTHY 1

#define ORL_MAX_HIDDEN 4
#define ORL_MAX_METRICS 8
#define ORL_MAX_NOISE 6

/* network ids (per algorithm; state_dict prefixes of SURVEY.md Appendix B) */
#define ORL_NET_ACTOR 0
#define ORL_NET_CRITIC1 1     /* IQL: critic_q1 ; EDAC: critics (ensemble) */
#define ORL_NET_CRITIC2 2     /* IQL: critic_q2 */
#define ORL_NET_CRITIC1_OLD 3 /* EDAC: critics_old */
#define ORL_NET_CRITIC2_OLD 4
#define ORL_NET_CRITIC_V 5    /* IQL only  */
#define ORL_NET_ACTOR_OLD 6   /* TD3BC only */
#define ORL_NET_VAE_ENC 7     /* MCQ behaviour policy (nets/vae.py): e1, e2, [mean; log_std] */
#define ORL_NET_VAE_DEC 8     /*                                      d1, d2, d3            */
#define ORL_NUM_NETS 9

/* per-run scalars (not nn.Parameters in the reference: run_cql.py:102, cql.py:57) */
#define ORL_SCALAR_LOG_ALPHA 0
#define ORL_SCALAR_CQL_LOG_ALPHA 1
#define ORL_SCALAR_ALPHA 2 /* read-only: the alpha the next learn() will use */
/* optimizer state of the scalars (torch.optim.Adam exp_avg / exp_avg_sq of alpha_optim, cql_alpha_optim) and TD3's
 * _last_actor_loss (td3.py:59): readable / writable so a policy can be re-bound or checkpointed without losing them */
#define ORL_SCALAR_LOG_ALPHA_M 3
#define ORL_SCALAR_LOG_ALPHA_V 4
#define ORL_SCALAR_CQL_LOG_ALPHA_M 5
#define ORL_SCALAR_CQL_LOG_ALPHA_V 6
#define ORL_SCALAR_LAST_ACTOR_LOSS 7

/* optimizer ids for orl_set_lr (run_iql.py:133 mutates actor_optim's lr per epoch) */
#define ORL_OPT_ACTOR 0
#define ORL_OPT_CRITIC 1
#define ORL_OPT_ALPHA 2
#define ORL_OPT_CQL_ALPHA 3
#define ORL_OPT_CRITIC_V 4
#define ORL_OPT_VAE 5      /* MCQ behavior_policy_optim */

typedef struct orl_config {
  int32_t algo;
  int32_t obs_dim, act_dim;
  int32_t n_hidden;
  int32_t hidden[ORL_MAX_HIDDEN];
  int32_t batch_size;
  int32_t n_runs;    /* independent runs carried by this engine (>=1) */
  int32_t device;    /* HIP device ordinal */
  int32_t precision; /* 0 fp32 MFMA; 1 split-fp16 MFMA (hi + lo planes); 2 three fp16 planes (exact fp32 operands, six products) in the many-row critic launches, fp32 MFMA elsewhere */
  uint64_t seed;     /* device Philox seed for orl_learn_n */
  float gamma, tau;
  float actor_lr, critic_lr, alpha_lr;
  float adam_beta1, adam_beta2, adam_eps;
  /* SAC family (sac.py:42-48) */
  int32_t auto_alpha;
  float alpha;
  float target_entropy;
  /* CQL (cql.py:16-60) */
  float cql_weight, temperature;
  int32_t max_q_backup, deterministic_backup, with_lagrange;
  float lagrange_threshold, cql_alpha_lr;
  int32_t num_repeat_actions;
  float act_low, act_high;
  /* IQL (iql.py:16-50) */
  float expectile, iql_temperature, critic_v_lr;
  /* TD3+BC (td3bc.py:17-53) */
  float policy_noise, noise_clip, td3bc_alpha, max_action;
  int32_t update_actor_freq;
  /* EDAC (edac.py:15-52) */
  int32_t num_critics;
  float eta;
  /* COMBO (policy/model_based/combo.py:110-241): the CQL update on a batch whose first `cql_real_rows` rows are real data and the rest
   * model rollouts.  The conservative term repeats rows [cql_cons_row0, cql_cons_row0 + cql_cons_rows) ("model": the model part,
   * "mix": the whole batch) and its -w mean Q term runs over the real rows only.  0 = the whole batch (plain CQL). */
  int32_t cql_cons_row0, cql_cons_rows, cql_real_rows;
  /* MCQ (mcq.py:19-46, run_mcq.py:34-36, 93-101): VAE hidden width / latent size, lambda, behaviour-policy lr; the number of sampled
   * actions is num_repeat_actions, the VAE's max_action is max_action */
  int32_t vae_hidden, vae_latent;
  float mcq_lambda, behavior_lr;
  /* launch geometry of the weight-stationary kernels (csrc/ws_gemm.h), per engine:
   *   ws_one_round  0 (default): as many workgroups per net as fill whole rounds of the CUs; 1: CUs / nets workgroups per net, one round
   *                 (what a process that runs SEVERAL engines per GPU wants: the CUs one engine's launch leaves idle are where the
   *                 other engines' kernels run; bench.py's two-engine default);
   *   ws_cus        CUs one launch spreads over, 8..256 (0 = 256).
   * The environment variables ORL_WS_ONE_ROUND / ORL_WS_CUS, when set, override these fields; they are read once, in orl_engine_create. */
  int32_t ws_one_round, ws_cus;
  /* nn.Dropout(p) behind every hidden ReLU of the ACTOR backbone (nets/mlp.py:16-24; run_iql.py:34,106 builds only the actor backbone with
   * --dropout_rate).  IQL only; 0 = none.  Active in learn() (policy.train() mode, iql.py:122), never in select_action (eval mode).
   * Teacher-forced runs pass the keep masks (0 / 1) of the reference's draws as noise slots 0 .. n_hidden - 1. */
  float actor_dropout;
  /* optional caller-owned parameter arena (device pointer, orl_arena_floats()
   * floats) so that framework tensors can alias engine parameters; NULL = the
   * engine allocates with hipMalloc. */
  float* external_arena;
  /* MOBILE (policy/model_based/mobile.py:19-57, 130-162): num_samples S and the dynamics' elite count E (the penalty pass runs on
   * S * E * batch_size rows), the number of leading batch rows that are real data (their penalty is zeroed, mobile.py:154) and the
   * penalty coefficient; deterministic_backup is CQL's field */
  int32_t mobile_num_samples, mobile_num_elites, mobile_real_rows;
  float penalty_coef;
} orl_config;

/* Replay minibatch: the dict ReplayBuffer.sample returns (buffer.py:96-106).
 * Arrays are [n_runs][batch][dim] row-major; rewards/terminals [n_runs][batch]. */
typedef struct orl_batch {
  const float* observations;
  const float* actions;
  const float* next_observations; /* RCSL: not read, may be NULL */
  const float* rewards;           /* RCSL: the returns-to-go ("rtgs") */
  const float* terminals;         /* RCSL: not read, may be NULL */
  int32_t on_device; /* 0: host pointers (copied in), 1: device pointers */
} orl_batch;

/* Explicit noise for a teacher-forced step, in the reference's draw order.
 * CQL: [0] eps_actor (B,A) N(0,1); [1] eps_next (B,A) or (B*N,A) with
 * max_q_backup; [2] u_rand (B*N,A) U[low,high); [3] eps_pi (B*N,A); [4] eps_next_pi (B*N,A).
 * EDAC: [0] eps_actor, [1] eps_next.  TD3BC: [0] eps_target (B,A).  IQL: none.  SAC: [0] eps_next, [1] eps_actor (B,A).
 * MCQ: [0] eps_vae (B,Z), [1] eps_next (B,A), [2] z_ood (2B*N,Z) N(0,1) (clamped to +-0.5 by the engine like VAE.decode), [3] eps_ood (2B,A),
 * [4] eps_actor (B,A).
 * MOBILE: [0] eps_lcb (S*E*B,A), [1] eps_next (B,A), [2] eps_actor (B,A).
 * Each array has a leading n_runs dimension. */
typedef struct orl_noise {
  const float* slot[ORL_MAX_NOISE];
  int32_t on_device;
} orl_noise;

typedef struct orl_engine orl_engine;

/* -- lifecycle --------------------------------------------------------------- */
const char* orl_last_error(void);
const char* orl_version(void);
int orl_split_bits(void); /* significand bits an operand carries at precision 1 (22: fp16 hi + lo planes; 16: the bf16-plane variant build) */
void orl_config_default(orl_config* cfg, int32_t algo); /* script defaults: run_{cql,iql,td3bc,edac}.py get_args() */
int64_t orl_arena_floats(const orl_config* cfg);        /* size of the parameter arena for external_arena */
int orl_engine_create(const orl_config* cfg, orl_engine** out); /* replaces <Algo>Policy.__init__ + deepcopy of targets (sac.py:29-33) */
void orl_engine_destroy(orl_engine* e);
int orl_engine_sync(orl_engine* e);                     /* hipStreamSynchronize on the engine stream */

/* -- parameters (nn.Module.state_dict() view) -------------- */
int orl_net_present(orl_engine* e, int net);
int64_t orl_net_floats(orl_engine* e, int net);
int orl_net_num_tensors(orl_engine* e, int net);
/* name: reference state_dict key relative to the net prefix (e.g. "backbone.model.0.weight") */
int orl_net_tensor(orl_engine* e, int net, int idx, char* name, int name_cap, int64_t* offset_floats,
                   int32_t* ndim, int64_t shape[4]);
float* orl_net_ptr(orl_engine* e, int run, int net);    /* device pointer to the net's flat fp32 parameters */
int orl_net_set(orl_engine* e, int run, int net, const float* host, int64_t n_floats); /* load_state_dict */
int orl_net_get(orl_engine* e, int run, int net, float* host, int64_t n_floats);       /* state_dict */
int orl_scalar_set(orl_engine* e, int run, int which, float v);
int orl_scalar_get(orl_engine* e, int run, int which, float* v);
int orl_set_lr(orl_engine* e, int opt, float lr);       /* optim.param_groups[0]["lr"] = lr */
int orl_reset_optimizers(orl_engine* e);                /* fresh torch.optim.Adam state (step=0, m=v=0) */
/* torch.optim.Adam state_dict()["state"] of a trainable net's optimizer: exp_avg / exp_avg_sq flat in state_dict order
 * (orl_net_floats values each); the shared step count is orl_step_count / orl_set_step_count (every optimizer of a policy steps
 * once per learn(); TD3BC's actor optimizer steps on every update_actor_freq-th call and derives its own count from it). */
int orl_adam_get(orl_engine* e, int run, int net, float* exp_avg, float* exp_avg_sq, int64_t n_floats);
int orl_adam_set(orl_engine* e, int run, int net, const float* exp_avg, const float* exp_avg_sq, int64_t n_floats);
int orl_set_step_count(orl_engine* e, int64_t steps);   /* resume: Adam's t, TD3BC's _cnt and the device RNG offsets continue from here */

/* -- replay buffer (buffer/buffer.py): its own object, like the reference's ReplayBuffer ------- */
typedef struct orl_buffer orl_buffer;
/* ReplayBuffer.__init__ (:8-32): an empty HBM-resident SoA store on `device` */
int orl_buffer_create(int32_t obs_dim, int32_t act_dim, int32_t device, orl_buffer** out);
void orl_buffer_destroy(orl_buffer* b);
/* load_dataset (:72-86): host arrays -> HBM SoA; obs/next_obs [n][obs_dim], act [n][act_dim], rew/term [n].  A buffer that feeds an RCSL
 * engine carries the return-to-go in `rew`; at precision >= 1 orl_engine_attach_buffer range-checks that column like the observations
 * (it is an MFMA operand there: |rtg| < 65504), and orl_health_check covers it with the net's input. */
int orl_buffer_load(orl_buffer* b, const float* obs, const float* act, const float* next_obs, const float* rew,
                    const float* term, int64_t n);
/* normalize_obs (:88-94): (x - mean) / (std + eps) in place on the device; mean/std(+eps) (obs_dim each) to host */
int orl_buffer_normalize_obs(orl_buffer* b, float eps, float* mean_out, float* std_out);
int64_t orl_buffer_size(orl_buffer* b);
/* sample (:96-106): gather `batch` rows into caller-owned DEVICE arrays (packed [batch][dim], rew/term [batch]).
 * idx: host int64[batch] (the np.random.randint draw of the reference) or NULL = device Philox(seed, call counter). */
int orl_buffer_sample(orl_buffer* b, const int64_t* idx, int32_t batch, uint64_t seed, float* obs_out, float* act_out,
                      float* next_obs_out, float* rew_out, float* term_out);
/* lets orl_learn_n sample this buffer on the device (the buffer must outlive the engine's use of it) */
int orl_engine_attach_buffer(orl_engine* e, orl_buffer* b);
/* -- growable ring: the model-rollout buffer of MOPO / COMBO kept in HBM ------------------------------------------------------
 * ReplayBuffer.__init__ (buffer/buffer.py:8-32): `capacity` rows allocated once, size 0, write position 0.  The device arrays do not
 * move until the next reserve / load.  The current size also lives in a device cell, which the samplers of orl_learn_n read for the
 * model source: a captured graph stays valid while the ring grows. */
int orl_buffer_reserve(orl_buffer* b, int64_t capacity);
/* add_batch (buffer/buffer.py:52-70): rows land at (ptr + i) % capacity, ptr = (ptr + n) % capacity, size = min(size + n, capacity).
 * Packed arrays obs/next_obs [n][obs_dim], act [n][act_dim], rew/term [n]; host pointers, device pointers when on_device.
 * n > capacity is refused.  On return the rows are visible to every stream of the process. */
int orl_buffer_append(orl_buffer* b, const float* obs, const float* act, const float* next_obs, const float* rew, const float* term,
                      int64_t n, int on_device);
/* the loop body of rollout() (policy/model_based/mopo.py:45-79, combo.py:67-108) for one model step; every array pointer is a DEVICE pointer to a
 * packed array.  Evaluates the termination test `term_kind` (0 never done, 1 halfcheetah, 2 hopper, 3 walker2d, 4 ant / antangle,
 * 5 humanoid, 6 pen: utils/termination_fns.py of the reference, its NaN behaviour and hopper's upper-bound-only check included) on
 * next_obs, appends all n transitions with terminals = the test's result (0 / 1), writes the next_obs rows of the transitions that
 * did NOT terminate densely and in their original order to alive_next_obs (room for n rows, not overlapping next_obs), and returns
 * their count and the float64 sum of rew through the two HOST pointers.  A kind that reads an observation column the buffer does not
 * have (pen: column 26; hopper / walker2d: column 1) is refused.
 * Health: rollouts are not range-checked when they are appended (the precision-1 dataset check of orl_engine_attach_buffer is a
 * one-off over a fixed dataset); a model row beyond the operand range shows in the sticky ORL_HEALTH_* flags and the operand scan of
 * orl_health_check like any other operand. */
int orl_buffer_append_rollout(orl_buffer* b, int32_t term_kind, const float* obs, const float* act, const float* next_obs,
                              const float* rew, int64_t n, float* alive_next_obs, int64_t* n_alive, double* rew_sum);
/* orl_buffer_append_rollout for n_runs rings in ONE launch pair (the per-run model rings of a multi-run MOPO / COMBO policy).  The
 * sources are packed DEVICE arrays [n_runs][row_stride][dim] (rew [n_runs][row_stride]) of which run r owns the first n[r] rows
 * (0 <= n[r] <= row_stride, n[r] == 0 is legal); alive_next_obs has the layout of next_obs and receives run r's surviving rows densely,
 * in order, at the head of run r's block -- rows past n_alive[r] are not written.  Ring r advances by n[r]: every ring keeps its own
 * write position, size and device size cell.  n, n_alive and rew_sum are HOST arrays of n_runs entries; the 2 * n_runs results come
 * back in one device-to-host copy.  The rings are distinct, reserved, of one shape and on one device; the refusals of the single-ring
 * call are made per ring and name the run. */
int orl_buffer_append_rollout_runs(orl_buffer* const* rings, int32_t n_runs, int32_t term_kind, const float* obs, const float* act,
                                   const float* next_obs, const float* rew, int64_t row_stride, const int64_t* n, float* alive_next_obs,
                                   int64_t* n_alive, double* rew_sum);
/* rows [row0, row0 + n) of the store back to packed host arrays (sample_all, buffer/buffer.py:108-115, and tests); a ring may be read
 * up to its capacity (rows never written are zero) */
int orl_buffer_read(orl_buffer* b, int64_t row0, int64_t n, float* obs, float* act, float* next_obs, float* rew, float* term);

/* -- trajectory store: the RCSL rollout's bookkeeping (policy/rcsl/rcsl.py:57-120) kept in HBM --------------------------------
 * Rows of up to `capacity_rows` transitions of up to `n_traj` trajectories: obs / next_obs / act (the padded pitches of orl_buffer, pad
 * columns zero), rew and term (0 / 1) float32, the trajectory index int32, the return accumulated BEFORE the transition and the
 * return-to-go float64; per trajectory its return, float64; and the live trajectories -- (index, accumulated return) pairs -- in two
 * arrays that the steps fill alternately.  float64 because the reference keeps `returns` / `acc_returns` in np.zeros arrays and adds
 * the float32 rewards to them: the same promotion and the same single add per step give the same bits. */
typedef struct orl_traj orl_traj;
int orl_traj_create(int32_t obs_dim, int32_t act_dim, int32_t device, int64_t n_traj, int64_t capacity_rows, orl_traj** out);
void orl_traj_destroy(orl_traj* t);
/* a new rollout of n_traj trajectories (at most the count given at creation): no rows, returns 0, live = 0 .. n_traj - 1 with
 * accumulated return 0, reward sum 0 */
int orl_traj_reset(orl_traj* t, int64_t n_traj);
/* the loop body of rollout() (rcsl.py:72-105) for one model step; every array pointer is a DEVICE pointer to a packed array and row i
 * belongs to the i-th live trajectory, so n must equal the live count.  Evaluates the termination test `term_kind` (as in
 * orl_buffer_append_rollout) on next_obs; appends the n transitions with terminals = the test's result, traj_idx = the live index and
 * acc_ret = the live accumulated return; adds rew (promoted to float64) to the trajectory's return -- a trajectory has one live row,
 * so a plain store --; writes the survivors' next_obs rows densely and IN THEIR ORIGINAL ORDER to alive_next_obs (room for n rows, not
 * overlapping next_obs) and their (index, accumulated return + rew) pairs, in the same order, to the other live array; adds the
 * float64 sum of rew, formed in block order, to the running reward sum.  The survivor count comes back through the HOST pointer
 * n_alive: the one device-to-host read of a step (it sizes the next one).
 * Refused before any launch: n != live count, more rows than the capacity left, an unknown kind, a kind that reads an observation
 * column the store does not have (pen: column 26; hopper / walker2d: column 1), alive_next_obs == next_obs. */
int orl_traj_append_step(orl_traj* t, int32_t term_kind, const float* obs, const float* act, const float* next_obs, const float* rew,
                         int64_t n, float* alive_next_obs, int64_t* n_alive);
/* The same step with the rows counted on the device: nothing is read back, so the host need not wait for the step before it enqueues
 * the next.  `bound` is any host-known upper bound on the live count (survivor counts never increase, so an older count is one); it
 * sizes the grid and the arrays the caller provides (obs / act / next_obs / rew: `bound` rows, of which only the first `live` are read;
 * alive_next_obs: room for the survivors).  The kernels take the live count and the row base from device cells and publish the next
 * step's; the cells are kept twice, alternating by step, so no launch reads a cell it writes.  live == 0 writes nothing.  Same
 * kernels, same fixed order and bits as orl_traj_append_step.  The host keeps upper bounds (rows: the sum of the bounds) and refuses,
 * before any launch, a bound that could exceed the capacity, next to orl_traj_append_step's refusals of kinds and overlap; the kernels
 * clamp as well and raise a sticky cell that orl_traj_finish / orl_traj_live report as an error (a bound below the live count does
 * that too; orl_traj_reset clears it).  orl_traj_finish and orl_traj_live refresh the host's rows / live from the cells (one read);
 * orl_traj_append_step and orl_traj_read before such a refresh are refused.  Null stream, like every orl_traj_* call. */
int orl_traj_append_step_counted(orl_traj* t, int32_t term_kind, const float* obs, const float* act, const float* next_obs,
                                 const float* rew, int64_t bound, float* alive_next_obs);
/* the end of rollout() (rcsl.py:107-112): rtg[row] = returns[traj_idx[row]] - acc_ret[row] in float64.  HOST outputs, each may be
 * NULL: the row count, the running reward sum, the n_traj returns.  Calling it twice is harmless; a later append_step needs a new
 * finish before the returns-to-go are read or exported. */
int orl_traj_finish(orl_traj* t, int64_t* rows, double* reward_sum, double* returns_host);
/* rows [row0, row0 + n) back to packed host arrays (obs / next_obs [n][obs_dim], act [n][act_dim], the rest [n]); any pointer may
 * be NULL; rtg after orl_traj_finish only */
int orl_traj_read(orl_traj* t, int64_t row0, int64_t n, float* obs, float* act, float* next_obs, float* rew, float* term,
                  int32_t* traj_idx, double* acc_ret, double* rtg);
/* run_mbrcsl.py's filter and the RCSL dataset in one: after orl_traj_finish, appends the rows of the trajectories with
 * returns > threshold (float64 compare, false on NaN; use_threshold == 0 keeps every row), in their order, behind the rows of the
 * reserved ring `dst`: obs / act / next_obs / term as stored, rew := (float)rtg -- the layout orl_learn_epoch reads.  The ring's size
 * cell is published as by orl_buffer_append.  HOST outputs: the rows appended, the trajectories above the threshold (all of them
 * without one).  The kept rows are counted first, so every refusal happens before a row is written: dst is not a ring, its dims or
 * device differ, or the kept rows exceed capacity - size (an RCSL dataset must not wrap). */
int orl_traj_export(orl_traj* t, int use_threshold, double threshold, orl_buffer* dst, int64_t* rows_kept, int64_t* traj_kept);
/* the real + model batch of MBPolicyTrainer (policy_trainer/mb_policy_trainer.py:78-85; _cat of mopo.py:81-84, combo.py:111-113) inside
 * orl_learn_n: batch rows [0, real_rows) are drawn from the buffer of orl_engine_attach_buffer, rows [real_rows, batch_size) from the
 * ring `model`; every row keeps its Philox counter.  0 < real_rows < batch_size, same dims and device as the engine; NULL detaches.
 * orl_learn_n fails while the ring is empty and, for CQL engines, when real_rows differs from cql_real_rows. */
int orl_engine_attach_model_buffer(orl_engine* e, orl_buffer* model, int32_t real_rows);
/* one model ring PER RUN: the model rows of run r's minibatches are drawn from models[r] only, with that ring's size read from its own
 * device cell.  n must equal the engine's n_runs; real_rows as above; every ring has the engine's dims and device.  orl_learn_n fails
 * while any run's ring is empty (the message names the run); a new reserve of any ring re-captures the graphs.  NULL or n == 0 detaches.
 * Attaching one form (this or orl_engine_attach_model_buffer) replaces the other. */
int orl_engine_attach_model_buffers(orl_engine* e, orl_buffer* const* models, int32_t n, int32_t real_rows);

/* -- the hot path ---------------------------------------------------------------- */
/* policy.learn(batch) with explicit noise: one gradient step for every run.
 * metrics: host [n_runs][ORL_MAX_METRICS] in the reference's result-dict order
 * (orl_metric_name); synchronous, like the reference's .item() calls. */
int orl_step(orl_engine* e, const orl_batch* batch, const orl_noise* noise, float* metrics);
/* MFPolicyTrainer inner loop (mf_policy_trainer.py:52-60): n x {sample -> learn -> logkv_mean},
 * sampling and noise on device; metrics_mean: host [n_runs][ORL_MAX_METRICS] epoch means;
 * elapsed_ms (optional): HIP-event time of the n steps on the engine stream. */
int orl_learn_n(orl_engine* e, int n_steps, float* metrics_mean, float* elapsed_ms);
/* RcslPolicyTrainer's inner loop (rcsl_policy_trainer.py:104-134) over a caller-supplied row order:
 * step s of run r learns rows order[r][s*B + b] of the attached buffer; a negative entry is padding.
 * order: int64 [n_runs][order_len] (a device pointer when on_device), order_len a multiple of batch_size; it is copied into an
 * engine-owned device array.  One shuffled pass of DataLoader(shuffle=True) is a permutation of [0, N) padded with -1 to a multiple of
 * B: a padding row contributes nothing to the loss, its gradient row is zero and the mean divides by valid rows x act_dim, which is the
 * reference's partial last batch.  The position within the epoch lives in a device cell: one captured step graph serves every step of
 * every epoch.  The row's index, padding included, is recorded per step (a padding row reads row 0 of the dataset).
 * metrics_mean: host [n_runs][ORL_MAX_METRICS], the unweighted mean over the order_len / B steps (logkv_mean per batch).
 * Refused before a step is launched: no buffer attached, order_len not a multiple of B, an entry >= the buffer's size (host orders are
 * checked on the host, device orders by one checking launch), a step whose rows are all padding, an engine that is none of RCSL, RCSL_GAUSS, AUTOREG. */
int orl_learn_epoch(orl_engine* e, const int64_t* order, int64_t order_len, int on_device,
                    float* metrics_mean, float* elapsed_ms);
/* AUTOREG: AutoregressivePolicy.forward (autoregressive.py:28-54) for n rows per run: act_dim forward-only passes, between them
 * a_j = mean + exp(logstd) * eps_j goes into the input of the next pass; no host synchronisation but the one at the end.
 * obs [n_runs][n][obs_dim]; eps [n_runs][n][act_dim] standard normals teacher-force the draws (NULL: a device Philox stream keyed by
 * (seed, this entry point's own call counter, run, row, dim)); act_out [n_runs][n][act_dim]; all three are device pointers when on_device.
 * Workspaces are sized for n at the first call and regrown when n grows.  Parameters, optimizer state, the step counter and the
 * noise streams of orl_learn_n are not touched.  Refused on any other engine. */
int orl_autoreg_sample(orl_engine* e, const float* obs, int64_t n, const float* eps, int on_device, float* act_out);
/* MOBILE: the next-state samples of the batch the NEXT orl_step learns, [n_runs][S * E * batch][obs_dim] in the row order of
 * orl_dynsample_next (row (s * E + e) * batch + b).  A device pointer (on_device) is borrowed until that step has run -- nothing is
 * copied, the producer must have finished writing (orl_dynsample_next synchronises its stream) --; a host pointer is copied in.  One
 * orl_step (or one orl_engine_lcb_penalty) consumes the samples; orl_step on a MOBILE engine without pending samples fails before it
 * launches anything, and orl_learn_n fails on a MOBILE engine (the dynamics forward is not on the engine's stream). */
int orl_engine_set_next_samples(orl_engine* e, const float* samples, int on_device);
/* MOBILE's compute_lcb (mobile.py:130-142) alone: the penalty pass of orl_step on the pending samples, WITHOUT the zeroing of the real
 * rows and without touching parameters, optimizer state or the step counter.  eps_lcb [n_runs][S * E * batch][act_dim] teacher-forces
 * the actor's draws (NULL: device Philox); penalty_out [n_runs][batch]; both are device pointers when on_device.  The "penalty" and
 * "lcb_q" taps hold the result afterwards. */
int orl_engine_lcb_penalty(orl_engine* e, const float* eps_lcb, float* penalty_out, int on_device);
/* RAMBO's advantage (policy/model_based/rambo.py:164-181) on an ORL_ALGO_SAC engine, forward only and run-batched: obs / next_obs
 * [n_runs][rows][obs_dim], act [n_runs][rows][act_dim], reward [n_runs][rows] (device pointers when on_device) ->
 *   a' = tanh(mu(s')), logp' = TanhNormal log-prob at the mode (log sigma clamped to [-5, 2]), q' = min(Q1, Q2)(s', a') on the LIVE
 *   critics [- alpha logp' when include_ent; alpha = the device temperature when auto_alpha, the configured one otherwise],
 *   value = r + (1 - term) gamma q' with term = the termination test term_kind (the codes of orl_buffer_append_rollout) on next_obs,
 *   raw = value - min(Q1, Q2)(s, a), advantage = (raw - mean) / (std + 1e-6) with the unbiased std over the rows of the run.
 * advantage [n_runs][rows] and stats [n_runs][2] = {mean of the normalised advantage, raw std} (device pointers when on_device; either
 * may be NULL).  One assemble launch ([s | a] and [s' | a'] are ONE 2 rows-row critic operand), the actor pass, one pass of both
 * critics, one reduction launch of one workgroup per run: fixed summation order, no float atomics.  Workspaces are sized for `rows`
 * at the first call and regrown when rows grows.  Parameters, optimizer state, the step counter and the noise streams of orl_learn_n
 * are not touched.  Taps afterwards ([rows] each): "adv.q_next", "adv.q_base", "adv.logp_next", "adv.term", "adv.raw", "adv.norm".
 * Refused: any other engine, rows < 2 (the unbiased std is NaN) or > 2^22, an unknown term_kind or one that reads an observation
 * column the engine does not have.  Synchronises the engine stream before returning. */
int orl_engine_adv_advantage(orl_engine* e, const float* obs, const float* act, const float* next_obs, const float* reward,
                             int32_t rows, int32_t term_kind, int32_t include_ent, float* advantage, float* stats, int on_device);
/* Sticky per-run health flags (ORL_HEALTH_* bits), flags_out: host uint32[n_runs] (may be NULL); returns the OR over the runs, < 0 on
 * error.  orl_step / orl_learn_n update the flags from what they already read back (metrics; one word per run that k_adam raises on a
 * non-finite gradient) and, at precision 1, scan the step's MFMA operands for the fp16-plane range when a run turned non-finite.
 * orl_health_check runs that range scan on demand (inputs, stored hidden activations and parameters of the LAST step; a pass over
 * the workspaces, not for the inner loop: MFPolicyTrainer calls it once per epoch); orl_health_clear resets the flags (after
 * load_state_dict / a restart of the diverged runs). */
int orl_health(orl_engine* e, uint32_t* flags_out);
int orl_health_check(orl_engine* e, uint32_t* flags_out);
int orl_health_clear(orl_engine* e);
int orl_num_metrics(orl_engine* e);
const char* orl_metric_name(orl_engine* e, int idx);
int64_t orl_step_count(orl_engine* e);

/* -- test / profiling taps --------------------------------------------------------- */
/* copies an intermediate of the LAST step to host: returns number of floats written or <0.
 * names: "q1","q2","target_q","q1a","q2a","logp_a", ... (algorithm specific; RCSL: "pred", "rcsl_x" = [obs | rtg]; RCSL_GAUSS: "z", "mu", "logvar" (post-clamp), "rcsl_x"; AUTOREG: "ar_x" [A * B][obs_dim + 2 A], "ar_out" [A * B][2] (post-activation), "ar_target" [A * B]); every engine also has the minibatch of the last
 * step ("b_obs","b_nobs","b_act","b_rew","b_term": what ReplayBuffer.sample returned / the device sampler drew) and its noise
 * arrays under their orl_noise slot names ("n_eps_actor", ...). */
int64_t orl_debug_read(orl_engine* e, int run, const char* name, float* host, int64_t cap);
/* packed ReLU-mask words (bit b of word w of a row <-> unit 32 w + b is > 0) of a hidden-activation workspace of the LAST step,
 * e.g. "ch0" / "ch1" = the CQL critics' hidden layers: [members][rows][width / 32] words; < 0 when the kernels that ran did not
 * emit bits for it.  What the backward kernels read instead of the activation (autograd's threshold_backward mask). */
int64_t orl_debug_read_bits(orl_engine* e, int run, const char* name, uint32_t* host, int64_t cap_words);
/* gradient of the LAST step w.r.t. the parameters of a trainable net, flat in state_dict order (orl_net_floats values): what
 * autograd leaves in param.grad before optimizer.step() (cql.py:180-190 etc.); the split-K slabs of the backward kernels summed. */
int orl_debug_grads(orl_engine* e, int run, int net, float* host, int64_t n_floats);
/* runs one generic GEMM tile configuration on host data (kernel unit tests): see csrc/gemm.h */
int orl_debug_gemm(int cfg, int mode, int M, int N, int K, const float* A, const float* B, const float* v0,
                   const float* v1, float* C, int ksplit, int precision);
/* The wider kernel unit-test tap: one launch of the tiled GEMM template with any epilogue, tile shape, batch (nz0 x nz1 problems),
 * row pitches, base offsets and fused side outputs (csrc/gemm.h, GemmP).  Every array is a host array that is copied to the device
 * WHOLE and (results) copied back WHOLE, so pad columns, guard rows and whatever the caller pre-filled them with come back untouched
 * wherever the kernel did not write.  Problem (z0, z1), split-K slab ks, row r starts at  off + z0 s0 + z1 s1 + ks ks + r pitch
 * (elements; 32-bit words for the mask arrays); `off` not a multiple of 4 gives a base that is not 16-byte aligned. */
typedef struct orl_gemm_buf {
  void* host;            /* null = not used */
  int64_t n;             /* elements in the array */
  int64_t off, pitch, s0, s1, ks;
} orl_gemm_buf;
typedef struct orl_gemm_ex {
  int32_t cfg;           /* tile shape 0..6 (csrc/gemm.h CFG_*); + 16 forces the scalar operand loaders */
  int32_t layout;        /* 0: A [M][K], B [N][K] (forward)   1: A [M][K], B [K][N] (dgrad)   2: A [K][M], B [K][N] (wgrad, epi 4 only) */
  int32_t epi;           /* 0..8: E_PLAIN, E_BIAS, E_BIAS_RELU, E_MASK, E_WGRAD, E_BIAS_SWISH, E_SWISH_GRAD, E_BIAS_LEAKY, E_LEAKY_MASK */
  int32_t pa;            /* 0: A as stored   1: rank-1 operand (A > 0 ? rowv * colv : 0), epi 0 / 3 / 4   2: the same from the mask words a_bits (epi 3) */
  int32_t precision;     /* 0 fp32 MFMA, 1 two 16-bit planes, 2 three planes */
  int32_t M, N, K, nz0, nz1, ksplit;
  int32_t a_kpad;        /* layout 0 / 1: A's rows are zero-padded to a multiple of 4 in k (the tap zero-fills the pad of the device copy) */
  int32_t c_trans;       /* epi 4: C stored (N, M)-major -- c_sr = 1, c_sn = C.pitch */
  int32_t c_null;        /* with w0: the masked tile itself is not stored */
  int32_t w0_in;         /* with w0: input columns of layer 0 (w0_x holds them, pitch <= 28) */
  int32_t tq_sm;         /* with tq_out: element stride between rows of tq_out */
  int32_t dry_run;       /* check the arguments and fill the report only: no device call */
  /* operands */
  orl_gemm_buf A, B, bias, aux, rowv, colv;
  orl_gemm_buf aux_bits;      /* epi 3: the mask as packed words (pitch = words per row); aux must still be given, it is what a launch reads that does not honour the words */
  orl_gemm_buf a_bits;        /* pa 2 */
  orl_gemm_buf tq_w, tq_b;    /* fused single-output tail of epi 2: weights [N], bias [1] */
  orl_gemm_buf w0_x;          /* fused layer-0 weight gradient of epi 3: the layer-0 input rows [M][pitch] */
  /* results (copied back whole) */
  orl_gemm_buf C;             /* [M][N], or [N][M] with c_trans; ks = split-K slab stride */
  orl_gemm_buf z_out;         /* epi 5: the pre-activation, C's geometry (only host / n are read) */
  orl_gemm_buf bias_out;      /* epi 4: row sums of A^T [M] per slab */
  orl_gemm_buf mb_out;        /* epi 2: mask words of the stored activation (pitch = words per row) */
  orl_gemm_buf tq_out;        /* [M] x tq_sm */
  orl_gemm_buf tq_part;       /* [column tile - 1][pitch >= M] */
  orl_gemm_buf w0_out;        /* [row tile (ks)][N][pitch >= w0_in] */
  orl_gemm_buf w0_bias;       /* [row tile (ks)][N]; s0 and ks must equal w0_out's */
  /* report: what the launch does with these arguments (filled before the device is touched) */
  int32_t r_cfg;              /* tile shape that runs (precision 2 reroutes CFG_WG to CFG_SQ) */
  int32_t r_la_pick, r_lb_pick;   /* pick_loader per operand (0 scalar, 1 VECK, 2 BLK4, 3 VECKU) */
  int32_t r_la, r_lb;             /* the instantiated pair after the rank-1 and pairing fall-backs */
  int32_t r_zmajor;
  int32_t r_store;            /* store path of problem (0, 0), slab 0: 0 staged through LDS, 1 direct 16-byte (scalar tail block), 2 scalar, 3 transposed through LDS */
  int32_t r_store_mixed;      /* some problem / slab takes another store path */
  int32_t r_mb, r_tq_parts, r_w0_slabs, r_aux_bits, r_a_bits;   /* requested side output honoured (0 = not) */
} orl_gemm_ex;
int orl_debug_gemm_ex(orl_gemm_ex* args);
/* The unit-test tap of the weight-stationary kernels (csrc/ws_gemm.h): ONE launch of one launch_ws_* function on host arrays.  Arrays
 * are described as in orl_debug_gemm_ex, copied to the device WHOLE and ALL copied back WHOLE (operands too), so guard words come back
 * untouched wherever the kernel did not write and an operand that comes back changed was written by the kernel.  An array named like a field of WsFwdP / WsDgradP / WsWgradP IS that field ("given or
 * not" picks the flavour); its `pitch` is the field's pitch (x_pitch, y_pitch, mb_g, x0_pitch, ab_g, c_pitch, h0_pitch, ...; 32-bit
 * words for the mask arrays), s0 / s1 the run / member strides, and, for the slab results (w0_out, b0_out, dW, db, dwt, dbt), s0 / s1
 * / ks = o_rs / the member stride / o_ks.  b0_out shares w0_out's s0 and ks; db, dwt and dbt share dW's.  Before the first HIP call the
 * tap checks every extent against the array sizes, refuses what the matching *_supported predicate refuses, per_z < 1, per_z > M / 32,
 * M > 4096 and nz0 * nz1 > 64, and fills the report. */
enum { ORL_WS_FWD = 0, ORL_WS_FWD3 = 1, ORL_WS_DGRAD = 2, ORL_WS_DGRAD3 = 3, ORL_WS_WGRAD = 4, ORL_WS_WGRAD3P = 5 };
typedef struct orl_ws_ex {
  int32_t kind;          /* ORL_WS_*: launch_ws_fwd, launch_ws_fwd3, launch_ws_dgrad_w0, launch_ws_dgrad3_w0, launch_ws_wgrad, launch_ws_wgrad3p */
  int32_t f32;           /* exact fp32 arithmetic (fwd, dgrad, wgrad) */
  int32_t np3;           /* wgrad: three planes of G (ws_wgrad_kernel<5>) */
  int32_t M, nz0, nz1;
  int32_t per_z;         /* workgroups (= split-K slabs) per problem; launch_ws_fwd gets it through WsGeom{cus = per_z * nz, one_round} */
  int32_t in0;           /* input columns of the first layer (fused first layer, layer-0 gradient, recompute) */
  int32_t x0_discard;    /* fwd / fwd3 with X0: h0 is not stored */
  int32_t w_sn, w_sk;    /* fwd / dgrad: strides of W (nn.Linear: fwd 256, 1, dgrad 1, 256; EnsembleLinear the other way round) */
  int32_t w0_sn, w0_sk;  /* strides of W0 */
  int32_t o_sr, o_sc;    /* dgrad: strides of a w0_out element (unit n, input c) inside a slab */
  int32_t tq_sm, dq_sm;  /* element strides between the rows of tq / dq */
  int32_t dry_run;       /* check the arguments and fill the report only: no device call */
  /* operands */
  orl_gemm_buf X;             /* fwd: input rows [M][pitch >= 256] (with X0: the RESULT h0, copied back); dgrad: layer-0 input rows [M][pitch <= 32] */
  orl_gemm_buf W, bias;       /* fwd: the layer; dgrad: W1 (no bias) */
  orl_gemm_buf tw, tb;        /* fwd: fused tail weights [256], bias [1] */
  orl_gemm_buf X0, W0, b0;    /* fwd: fused first layer; wgrad: h0 recomputed (X0 rows [M][pitch <= 32]) */
  orl_gemm_buf dmask;         /* fwd: plain dgrad mode, mask words of the receiving activation */
  orl_gemm_buf abits, xbits;  /* dgrad / wgrad: mask words of the top (abits) and the layer-0 (xbits) activation */
  orl_gemm_buf dq, wt;        /* dgrad / wgrad: dLoss/dq per row, w_tail [256] */
  orl_gemm_buf Z;             /* dgrad: materialised incoming gradient (PLAIN) */
  orl_gemm_buf H0, H1, W1, b1, dZ;   /* wgrad */
  orl_gemm_buf gscale;        /* one float per run (z0), flat from `off` */
  /* results */
  orl_gemm_buf Y, mb, mb0, tq, tq2;       /* fwd */
  orl_gemm_buf C, w0_out, b0_out;         /* dgrad: dz0 (STORE) or the dW0 / db0 slabs (W0) */
  orl_gemm_buf dW, db, dwt, dbt;          /* wgrad slabs */
  /* report (filled before the device is touched) */
  int32_t r_launcher;         /* = kind */
  int32_t r_flavour;          /* index into the tap's table of instantiations (orl_debug_ws_flavour) */
  int32_t r_lds;              /* dynamic LDS bytes of the launch */
  int32_t r_groups;           /* M / 32 */
} orl_ws_ex;
int orl_debug_ws(orl_ws_ex* args);
/* name of instantiation `idx` of the tap's table ("ws_fwd<TQ,L0,DG,SY,F32,XS>", "ws_wgrad32<MODE>", ...); NULL past its end */
const char* orl_debug_ws_flavour(int idx);
/* The unit-test tap of the few-rows kernels (csrc/small_fwd.h, csrc/small_bwd.h): ONE launch of launch_small_fwd (ORL_SMALL_FWD) or
 * launch_small_abwd (ORL_SMALL_ABWD) on host arrays.  Arrays are described as in orl_debug_gemm_ex, copied to the device WHOLE and ALL
 * copied back WHOLE (operands too).  An array named like a field of SmallFwdP / SmallABwdP IS that field; given or not picks the mode
 * (G: QG mode; H0 / H1 null: not stored; job[i].eps / .logp null: deterministic / no log-probability).  `pitch` is the field's pitch
 * (x_pitch, o_pitch, g_pitch, dst_pitch, xa_pitch, ga_pitch), s0 / s1 the run / member strides (qa, ga: s1 = the critic stride; a job's
 * arrays: s0 = eps_rs / dst_rs / logp_rs), out.ks = o_ks.  small_abwd: nz0 = runs, nz1 = 1; sc is a float array [runs][16] in RunScalars'
 * layout (csrc/scalars.h), hy 8 floats (Hyper), gstep two 32-bit words = one 64-bit value at an even offset, part [runs][64][2], ticket
 * [runs] (zero on entry); sc, metrics_*, part and ticket are dense per run.  Before the first HIP call the tap checks every extent against
 * the array sizes (job.dst / eps / logp and the six slab offsets against o_ks included), refuses what small_fwd_supported /
 * small_abwd_supported refuse, a null OUT, o_pitch < out_dim, M > 2048 and nz0 * nz1 > 16, and fills the report. */
enum { ORL_SMALL_FWD = 0, ORL_SMALL_ABWD = 1 };
typedef struct orl_small_job {
  int32_t head_row0, rows, rep;   /* SampleJob: output row j draws from head row head_row0 + j / rep */
  int32_t dst_row0, dst_col;
  orl_gemm_buf eps;               /* [runs][rows][A]; null: deterministic */
  orl_gemm_buf dst;               /* action a of row j at off + z0 s0 + (dst_row0 + j) pitch + dst_col + a */
  orl_gemm_buf logp;              /* [runs][rows]; null: not written */
} orl_small_job;
typedef struct orl_small_ex {
  int32_t kind;          /* ORL_SMALL_* */
  int32_t f32;           /* exact fp32 MFMA instead of the split 16-bit planes */
  int32_t M, nz0, nz1;
  int32_t in0;           /* input columns of the first layer (1..31) */
  int32_t out_dim;       /* fwd: tail outputs (1..16) */
  int32_t gc0, gn;       /* fwd, QG: differentiated input columns gc0 .. gc0 + gn */
  int32_t njobs, A;      /* fwd: sampling jobs (out_dim = 2 A); abwd: action dimensions */
  int32_t K;             /* abwd: critics (2) */
  int32_t xa_col;        /* abwd: first action column inside xa's rows */
  int32_t auto_alpha, clamp_alpha01;
  int32_t nm, m_actor, m_alpha_loss, m_alpha;    /* abwd: metrics per run and the three slots */
  int32_t dry_run;       /* check the arguments and fill the report only: no device call */
  float fixed_alpha, target_entropy, adam_b1, adam_b2, adam_eps;
  int64_t off_w0, off_b0, off_w1, off_b1, off_wh, off_bh;   /* abwd: the six tensors inside a slab */
  /* both launchers */
  orl_gemm_buf X, W0, b0, W1, b1, Wt, bt;   /* abwd takes X and W1 only */
  orl_gemm_buf H0, H1;                      /* fwd: results (null: not stored); abwd: operands */
  orl_gemm_buf OUT, G;                      /* fwd results */
  orl_small_job job[3];
  /* abwd */
  orl_gemm_buf head, eps, xa, logp, qa, ga, Wh;
  orl_gemm_buf out;                         /* slab g of run z0 at off + z0 s0 + g ks */
  orl_gemm_buf sc, hy, gstep, metrics_last, metrics_sum, part, ticket;
  /* report (filled before the device is touched) */
  int32_t r_kind;             /* = kind */
  int32_t r_flavour;          /* index into the tap's table of instantiations (orl_debug_small_flavour) */
  int32_t r_lds;              /* dynamic LDS bytes of the launch */
  int32_t r_groups;           /* M / 32 */
} orl_small_ex;
int orl_debug_small(orl_small_ex* args);
/* name of instantiation `idx`: "small_fwd<F32,QG>" x 4, then "small_abwd<F32>" x 2; NULL past the end */
const char* orl_debug_small_flavour(int idx);
/* times `reps` launches of one GEMM tile configuration on random data (kind 0 forward, 1 dgrad, 2 wgrad) */
int orl_debug_gemm_time(int cfg, int kind, int M, int N, int K, int nz, int ksplit, int reps, float* ms_out);
/* average duration (ms) of the kernel with the largest accumulated time during the last orl_learn_n
 * when profiling was enabled with orl_profile_enable(e,1); name copied to `name`. */
int orl_profile_enable(orl_engine* e, int on);
int orl_profile_query(orl_engine* e, int idx, char* name, int name_cap, double* total_ms, int64_t* launches,
                      double* flops_per_launch, double* bytes_per_launch);

/* -- dynamics ensemble (dynamics/ensemble_dynamics.py, modules/dynamics_module.py): its own object ----------------------------
 * The probabilistic ensemble of MOPO / COMBO: num_ensemble EnsembleLinear MLPs with Swish activations whose output layer gives a
 * mean and a soft-clamped log-variance for (delta obs, reward).  Like orl_engine it carries n_runs independent runs (seeds); every
 * host array has a leading run dimension.  Parameters per run, in the reference's state_dict order (orl_dyn_tensor): max_logvar,
 * min_logvar, then backbones.{i}.{weight,bias,saved_weight,saved_bias} and output_layer.* (weights (K, in, out), biases (K, 1, out));
 * each tensor starts on a 16-byte boundary of the flat per-run block.  `elites` (int64 in the reference) lives outside the fp32 block
 * (orl_dyn_set_elites / orl_dyn_get_elites).  Only precision 0 (fp32 MFMA) is implemented. */
typedef struct orl_dyn_config {
  int32_t obs_dim, act_dim;
  int32_t n_hidden;                 /* <= ORL_MAX_HIDDEN */
  int32_t hidden[ORL_MAX_HIDDEN];
  int32_t num_ensemble, num_elites, with_reward;
  float weight_decay[ORL_MAX_HIDDEN + 1];   /* per layer, the output layer last (dynamics_module.py:56-68) */
  float lr, adam_beta1, adam_beta2, adam_eps;
  int32_t batch_size;
  float logvar_loss_coef;
  int32_t n_runs, device, precision;
  uint64_t seed;                    /* device Philox seed of orl_dyn_step without teacher-forced noise */
  float* external_arena;            /* optional caller-owned device block of n_runs * orl_dyn_floats floats (torch aliasing); NULL = hipMalloc */
} orl_dyn_config;

#define ORL_DYN_PENALTY_ALEATORIC 0      /* max_k || std_k ||  (all out dims) */
#define ORL_DYN_PENALTY_PAIRWISE_DIFF 1  /* max_k || mean_k - mean over k ||  (obs dims) */
#define ORL_DYN_PENALTY_ENSEMBLE_STD 2   /* sqrt(mean_d var_k mean_k)  (obs dims) */

typedef struct orl_dynamics orl_dynamics;
void orl_dyn_config_default(orl_dyn_config* cfg);       /* run_mopo.py defaults: [200]*4, 7 members, 5 elites, its decays, lr 1e-3, batch 256 */
int orl_dyn_create(const orl_dyn_config* cfg, orl_dynamics** out);
void orl_dyn_destroy(orl_dynamics* d);
int orl_dyn_sync(orl_dynamics* d);
int64_t orl_dyn_floats(orl_dynamics* d);                /* floats of one run's parameter block */
int64_t orl_dyn_config_floats(const orl_dyn_config* cfg); /* the same before creation (size of external_arena / n_runs) */
int orl_dyn_num_tensors(orl_dynamics* d);
int orl_dyn_tensor(orl_dynamics* d, int idx, char* name, int name_cap, int64_t* offset_floats, int32_t* ndim, int64_t shape[4]);
float* orl_dyn_ptr(orl_dynamics* d, int run);           /* device pointer to the run's parameter block (aliasing from torch) */
int orl_dyn_set(orl_dynamics* d, int run, const float* host, int64_t n_floats);
int orl_dyn_get(orl_dynamics* d, int run, float* host, int64_t n_floats);
/* torch.optim.Adam state of the run: exp_avg / exp_avg_sq over the parameter block (zero where the reference keeps no state:
 * saved_* get no gradient) and its step count */
int orl_dyn_adam_get(orl_dynamics* d, int run, float* exp_avg, float* exp_avg_sq, int64_t n_floats, int64_t* step);
int orl_dyn_adam_set(orl_dynamics* d, int run, const float* exp_avg, const float* exp_avg_sq, int64_t n_floats, int64_t step);
int orl_dyn_set_elites(orl_dynamics* d, int run, const int64_t* idx, int n);   /* model.set_elites */
int orl_dyn_get_elites(orl_dynamics* d, int run, int64_t* idx, int cap);       /* returns the number of elites, < 0 on error */
/* format_samples_for_training output loaded into HBM once: inputs [n][obs+act], targets [n][obs + with_reward] */
int orl_dyn_load_data(orl_dynamics* d, const float* inputs, const float* targets, int64_t n);
int orl_dyn_set_scaler(orl_dynamics* d, int run, const float* mu, const float* std);   /* StandardScaler of the run (obs+act each) */
/* learn() (ensemble_dynamics.py:178-209) for every run: idx host int64 [n_runs][num_ensemble][train_size], rows of the loaded data
 * (the bootstrap indices composed with the run's train split), in minibatch order; active: host int32 [n_runs] (NULL = all), an
 * inactive run's parameters and Adam state stay bit for bit.  No host synchronisation inside the epoch; loss_out: host [n_runs]
 * mean minibatch loss (0 for inactive runs). */
int orl_dyn_learn_epoch(orl_dynamics* d, const int64_t* idx, int64_t train_size, const int32_t* active, float* loss_out);
/* validate() (:211-217): idx host int64 [n_runs][holdout_size] rows of the loaded data; mse_out host [n_runs][num_ensemble] */
int orl_dyn_validate(orl_dynamics* d, const int64_t* idx, int64_t holdout_size, float* mse_out);
int orl_dyn_update_save(orl_dynamics* d, int run, const int32_t* member_mask);   /* update_save(indexes): mask [num_ensemble] */
int orl_dyn_load_save(orl_dynamics* d, int run);
/* step() (:29-80) without the terminal function: obs [n_runs][n][obs_dim], act [n_runs][n][act_dim] (device pointers when on_device).
 * noise [n_runs][num_ensemble][n][obs_dim + with_reward] and model_idx [n_runs][n] teacher-force the reference's np.random.normal /
 * random_elite_idxs draws; NULL = device Philox (seed, call counter): N(0,1) noise, model index uniform over the elites.
 * Outputs [n_runs][n][obs_dim] and [n_runs][n]: reward = raw_reward - penalty_coef * penalty; model_idx_out may be NULL.
 * Outputs are host arrays, device arrays when on_device. */
int orl_dyn_step(orl_dynamics* d, const float* obs, const float* act, int64_t n, int on_device, const float* noise,
                 const int64_t* model_idx, int penalty_mode, float penalty_coef, float* next_obs, float* reward, float* raw_reward,
                 float* penalty, int32_t* model_idx_out);
/* sample_next_obss (:82-99) for MOBILE: one shared-input ensemble forward on the n rows, then for each of num_samples samples and each
 * ELITE (in orl_dyn_set_elites order) mean + eps * std with mean[..., :obs_dim] += obs, in fp32 with the two roundings of
 * randn_like(std) * std + mean.  next_obs [n_runs][num_samples * E * n][obs_dim], row (s * E + e) * n + b: the reference's
 * reshape(-1, obs_dim).  noise [n_runs][num_samples][E][n][obs_dim + with_reward] teacher-forces the draws (the reward column is drawn
 * and dropped); NULL = a device Philox stream of this entry point alone, keyed by (seed, its own call counter, run, sample, elite
 * position, row, dim): orl_dyn_step and orl_dynadv_forward draw what they draw without this call.  Pointers are device pointers when
 * on_device (then nothing visits the host); the call ends with a stream synchronisation.  Refused: num_samples < 1, fewer than 2
 * elites, runs with different elite counts.  (Named orl_dynsample_*, not orl_dyn_*, like orl_dynadv_*.) */
int orl_dynsample_next(orl_dynamics* d, const float* obs, const float* act, int64_t n, int32_t num_samples, int on_device,
                       const float* noise, float* next_obs);
/* how many sample calls the object has made: orl_dynsample_next's call counter, which also advances once per step of
 * orl_mobile_learn_n (the Philox key of the next call's draws); < 0 for a null handle */
int64_t orl_dynsample_calls(orl_dynamics* d);
/* test tap: parameter gradient of the LAST minibatch of the last orl_dyn_learn_epoch, or of the last orl_dynadv_update, whichever
 * ran later (flat like orl_dyn_get; decay terms excluded) */
int orl_dyn_debug_grads(orl_dynamics* d, int run, float* host, int64_t n_floats);
/* test taps: one run's workspaces as the last call left them (the stream is synchronised; nothing is added to any call's path).  Only
 * the first `rows` rows of each member block come back, `rows` being that call's row count (of orl_dyn_learn_epoch: its LAST
 * minibatch's).  With D = obs_dim + with_reward and pitch0 = obs_dim + act_dim rounded up to 4:
 *   after orl_dyn_learn_epoch    "learn.x" [K][rows][pitch0] (pad columns included), "learn.t" [K][rows][D], "learn.out" / "learn.dout"
 *                                [K][rows][2 D], "learn.lterm" / "learn.gmax" / "learn.gmin" [K][rows][D], "learn.nll" [1] (the loss
 *                                without the decay term) and "learn.decay" [ceil(floats / 1024)] (the decay loss of each 1024-float
 *                                block); the last two cells are shared with orl_dynadv_update and hold the later call's
 *   after orl_dyn_step, orl_dynsample_next, orl_dyn_validate   "step.x" [n][pitch0], "step.out" [K][n][2 D]; after validate "step.t" [H][D]
 *   after orl_dynadv_forward     "adv.x" [Ba + Bs][pitch0], "adv.t" [Bs][D], "adv.obs" [Ba][obs_dim], "adv.s" [Ba][D] (the kept sample),
 *                                "adv.out" [K][Ba + Bs][2 D]
 *   after orl_dynadv_update      "adv.dout" [K][Ba + Bs][2 D], "adv.lterm" / "adv.gmax" / "adv.gmin" [K][Ba + Bs][D], "adv.rowlp" [Ba][2]
 *                                (each row's double log-probability x as hi = (float)x, lo = (float)(x - hi)), "adv.advm" [2]
 * Returns the floats written; < 0 (the message names the tap) for an unknown name, a run out of range, a tap whose call has not happened
 * yet or whose workspace has been replaced since, an "adv." tap before orl_dynadv_configure, and a cap that is too small. */
int64_t orl_dyn_debug_read(orl_dynamics* d, int run, const char* name, float* host, int64_t cap);

/* -- RAMBO's adversarial model update (policy/model_based/rambo.py:129-207) on an orl_dynamics ------------------------------------
 * One update of dynamics_step_and_forward is two calls; the caller computes the advantage (actor and critics) between them
 * (orl_engine_adv_advantage does, on a SAC engine; orl_rambo_update_dynamics runs whole updates of many steps without the host).
 * The optimizer (dynamics_adv_optim) has its own exp_avg / exp_avg_sq / step count: orl_dyn_learn_epoch's Adam state is never touched,
 * and the forward's activations, workspaces and kept sample belong to these calls alone (orl_dyn_step / validate / learn_epoch
 * between the two calls leave them alone).  fp32, run-batched like every orl_dyn_* call. */
/* Adam hyper-parameters of the adversarial optimizer, adv_weight, and the row counts of a call (rollout rows Ba, dataset rows Bs).
 * Allocates the state on the first call (zero moments, step 0); a later call keeps the state and re-sizes the workspaces. */
int orl_dynadv_configure(orl_dynamics* d, float lr, float adam_beta1, float adam_beta2, float adam_eps, float adv_weight,
                         int32_t rollout_rows, int32_t sl_rows);
/* Forward: obs [n_runs][Ba][obs_dim], act [n_runs][Ba][act_dim] rollout rows and sl_* [n_runs][Bs][..] dataset rows (sl_rew
 * [n_runs][Bs]) are scaled and concatenated into one input shared by the members; one ensemble forward keeps the activations.
 * The row's sample s = mean_m + std_m * eps_m (fp32, like Normal.sample) of its member m gives next_obs [n_runs][Ba][obs_dim] and
 * reward [n_runs][Ba]; s stays on the device for the update.  noise [n_runs][num_ensemble][Ba][obs_dim + 1] (device when on_device)
 * and model_idx (HOST int64 [n_runs][Ba]) teacher-force the draws; NULL = device Philox / uniform over the run's elites.
 * model_idx_out [n_runs][Ba] may be NULL.  Arrays are device pointers when on_device.  Synchronises the stream before returning. */
int orl_dynadv_forward(orl_dynamics* d, const float* obs, const float* act, const float* sl_obs, const float* sl_act,
                       const float* sl_next_obs, const float* sl_rew, int on_device, const float* noise, const int64_t* model_idx,
                       float* next_obs, float* reward, int32_t* model_idx_out);
/* Update: advantage [n_runs][Ba] (already normalised; device pointer when on_device).  Loss = adv_weight * mean_i(log_prob_i A_i)
 * + Gaussian NLL of the dataset rows + decay + 0.001 (sum max_logvar - sum min_logvar), where log_prob_i is the log of the elite
 * mixture's density at the kept sample, computed as a log-sum-exp (finite where the reference's exp underflows).  One backward over
 * the Ba + Bs rows and one Adam step of the adversarial optimizer.  active: host int32 [n_runs] (NULL = all); an inactive run's
 * parameters and state stay bit for bit.  metrics_out: host [n_runs][4] = all_loss, sl_loss, adv_loss (unweighted), mean log_prob
 * (zeros for inactive runs).  Fails without a pending orl_dynadv_forward: one update per forward. */
int orl_dynadv_update(orl_dynamics* d, const float* advantage, int on_device, const int32_t* active, float* metrics_out);
/* the adversarial optimizer's state, as orl_dyn_adam_get / orl_dyn_adam_set */
int orl_dynadv_adam_get(orl_dynamics* d, int run, float* exp_avg, float* exp_avg_sq, int64_t n_floats, int64_t* step);
int orl_dynadv_adam_set(orl_dynamics* d, int run, const float* exp_avg, const float* exp_avg_sq, int64_t n_floats, int64_t step);

/* RAMBO's update_dynamics (rambo.py:95-127) without a host round trip per step.  A segment is one draw of `rows` initial observations
 * from `real` followed by segment_steps[s] steps; a step is: a ~ pi(. | obs) by the engine's actor on the unscaled observations
 * (noise from a Philox stream of this entry point alone), a fresh draw of `rows` dataset rows, the adversarial forward, the advantage
 * (orl_engine_adv_advantage's pass), the adversarial update, obs <- next_obs (all rows carry on, terminated or not). */
typedef struct orl_rambo_loop {
  int32_t rows;                 /* adv_rollout_batch_size: rollout rows = dataset rows per step, as given to orl_dynadv_configure */
  int32_t term_kind;            /* the codes of orl_buffer_append_rollout */
  int32_t include_ent;
  int32_t n_segments;
  const int32_t* segment_steps; /* host [n_segments], each >= 1 */
} orl_rambo_loop;
/* Every launch of the loop goes to the engine's stream (the dynamics' own stream is waited for through an event first), the host
 * synchronises once at the end.  The five logged values (all_loss, sl_loss, adv_loss, adv_advantage, adv_log_prob) are summed in a
 * device array, read once and divided by the step count into metrics_mean[5]; elapsed_ms (optional) is the HIP-event time of the loop.
 * Step i draws from the dynamics what orl_dynadv_forward(noise = NULL, model_idx = NULL) at the same call counter draws and advances
 * that counter; a buffer draw is orl_buffer_sample(idx = NULL, seed = the engine's seed) at the buffer's draw counter and advances it;
 * the adversarial optimizer's step count advances by the number of steps.  A non-finite value raises the engine's
 * ORL_HEALTH_NONFINITE_LOSS like orl_learn_n (return code ORL_RC_UNHEALTHY).  Taps of the LAST step's unscaled rows on the engine:
 * "loop.obs", "loop.act", "loop.sl_obs", "loop.sl_act", "loop.sl_next_obs", "loop.sl_rew", "loop.next_obs", "loop.reward"; the
 * "adv.*" taps of both objects hold the last step's.  Refused before anything is launched or any counter moves: an engine that is
 * not ORL_ALGO_SAC, n_runs != 1 on either side, no orl_dynadv_configure, rows that differ from the configured row counts, different
 * devices or dims, an empty buffer, an unknown term_kind (or one that reads a missing observation column), rows < 2, no steps. */
int orl_rambo_update_dynamics(orl_engine* e, orl_dynamics* d, orl_buffer* real, const orl_rambo_loop* a, float* metrics_mean /*[5]*/,
                              float* elapsed_ms);

/* MOBILE's learn (mobile.py:144-196) n_steps times without a host round trip per step: `e` an ORL_ALGO_MOBILE engine with a dataset
 * buffer (orl_engine_attach_buffer) and a model ring (orl_engine_attach_model_buffer, real_rows = the engine's mobile_real_rows), `d`
 * its dynamics.  Every launch of both objects goes to the engine's stream (the dynamics' own stream is waited for through an event
 * first), launched eagerly, and the host synchronises once at the end.  Step i: the minibatch draw and the three noise slots of
 * orl_learn_n at the step counter (rows [0, real_rows) from the dataset, the rest from the ring; same Philox keys as a SAC engine's
 * orl_learn_n); the launches of orl_dynsample_next(noise = NULL) on the drawn observation / action rows at the dynamics' sample call
 * counter, with the S * E * B samples written straight into the operands of the penalty pass (no sample array, no assemble launch:
 * the same values bit for bit); orl_step's launches behind the assemble.  Metrics are summed on the device and divided by n_steps
 * into metrics_mean [n_runs][ORL_MAX_METRICS]; elapsed_ms (optional) is the HIP-event time of the loop; health flags and the return
 * code ORL_RC_UNHEALTHY as for orl_learn_n.  The engine's step counter and the dynamics' sample call counter advance by n_steps;
 * orl_dyn_step's and orl_dynadv_*'s counters do not move and a pending orl_dynadv_forward stays pending.  The taps "penalty", "lcb_q",
 * "xs", "xl", "ql1", "ql2", "logp_l", the batch slots and the noise slots hold the last step's values.  Refused before anything is
 * launched or any counter moves: an engine that is not ORL_ALGO_MOBILE, n_runs != 1 on either object, different devices or dims, a
 * dynamics without reward, fewer than 2 elites or a count that differs from mobile_num_elites, no dataset buffer, no or an empty model
 * ring (or one attached with another real_rows), n_steps < 1, pending samples of orl_engine_set_next_samples (they stay usable by
 * the next orl_step).  orl_learn_n keeps refusing MOBILE engines. */
int orl_mobile_learn_n(orl_engine* e, orl_dynamics* d, int n_steps, float* metrics_mean /*[n_runs][ORL_MAX_METRICS]*/, float* elapsed_ms);

/* RcslPolicy.rollout (rcsl.py:57-120) as one device loop: `policy` an ORL_ALGO_AUTOREG engine, `d` its dynamics, `store` the
 * trajectory store (reset here for n_traj trajectories).  Every launch of the three objects goes to the policy engine's stream (the
 * dynamics' own stream and the store's reset are waited for through events first).  Step t: orl_autoreg_sample's launches on the
 * current observation rows, orl_dyn_step's launches, orl_traj_append_step_counted into the other of two observation buffers, an
 * asynchronous copy of the survivor count into slot t of a pinned host array, an event.  Before enqueueing step t the host waits for
 * the event of step t - 1 - lag (if any) and uses that count as the row bound of all three parts: a stale count is a valid bound, rows
 * in [live, bound) are computed from finite stale data and never stored.  lag = 0: exact sizes, one wait per step.  When a known count
 * is 0 the host stops (at most `lag` steps run with nothing live); one stream synchronisation at the end, then orl_traj_finish, whose
 * three HOST outputs these are.  init_obs: DEVICE [n_traj][obs_dim].  eps: DEVICE [length][n_traj][act_dim] standard normals, step t
 * reads the first `bound` rows of slice t (noise keyed by step and row position); NULL: the sampler's own Philox stream.  The dynamics
 * draws what orl_dyn_step(noise = NULL, model_idx = NULL) draws at the same call counter, which advances once per step enqueued.
 * steps_enqueued, elapsed_ms (the HIP-event time of the loop): optional HOST outputs.  Refused before any launch, the store and every
 * counter untouched: n_runs != 1 on either object, an engine that is not ORL_ALGO_AUTOREG, different devices or dims, a store created
 * for fewer than n_traj trajectories or n_traj * length rows, an unknown term_kind (or one that reads a missing observation column),
 * an unknown penalty_mode, lag < 0, a dynamics without reward. */
int orl_mbrcsl_rollout(orl_engine* policy, orl_dynamics* d, orl_traj* store, const float* init_obs, int32_t n_traj, int32_t length,
                       int32_t term_kind, int32_t penalty_mode, float penalty_coef, const float* eps, int32_t lag, int64_t* rows,
                       double* reward_sum, double* returns_host, int32_t* steps_enqueued, float* elapsed_ms);

/* the int32 indices of the live trajectories of the current rollout, in row order, widened to int64 into the DEVICE array
 * out_device (room for the live count, which is returned; < 0 on error).  Live indices ascend and are never compacted, so a per-trajectory
 * table (a frozen noise, say) is indexed with them directly. */
int64_t orl_traj_live(orl_traj* t, int64_t* out_device);

/* -- DiffusionBC: the diffusion behaviour policy (policy/others/diffusion.py, nets/unet.py at sequence length 1) ---------------
 * The network is ConditionalUnet1D called with one time step: every Conv1d(k, padding = k / 2) reads its centre tap only, the
 * down / up sampling is absent, and the U-Net is a FiLM-conditioned residual MLP of GroupNorm + Mish blocks with skip concatenations.
 * The engine keeps the centre taps as dense [out][in] matrices; the off-centre taps never receive a gradient and stay with the caller.
 * One object = one run, precision 0 (fp32 MFMA). */
#define ORL_DIFF_MAX_LEVELS 4
typedef struct orl_diffusion orl_diffusion;
typedef struct {
  int32_t obs_dim, act_dim;
  int32_t step_embed_dim;           /* diffusion_step_embed_dim, even and >= 4 */
  int32_t n_levels;                 /* len(down_dims), 1 .. ORL_DIFF_MAX_LEVELS */
  int32_t down_dims[ORL_DIFF_MAX_LEVELS];
  int32_t kernel_size;              /* odd: only the centre tap takes part */
  int32_t n_groups;                 /* of the blocks' norms: every channel count is a multiple of it; final_conv's norm has 8 */
  int32_t num_diffusion_iters;      /* N */
  int32_t batch_size;
  float adam_beta1, adam_beta2, adam_eps;
  int32_t n_runs, device, precision;
  uint64_t seed;
} orl_diffusion_config;
void orl_diffusion_config_default(orl_diffusion_config* cfg);  /* hopper: 11 / 3, embed 256, [256, 512, 1024], k 5, 8 groups, N 10, batch 256 */
/* Refused: n_runs != 1, precision != 0, an even kernel_size, a channel count that n_groups does not divide, a group wider than 512,
 * down_dims[0] not a multiple of 8 (final_conv's norm is GroupNorm(8) whatever n_groups is). */
int orl_diffusion_create(const orl_diffusion_config* cfg, orl_diffusion** out);
void orl_diffusion_destroy(orl_diffusion* d);
int64_t orl_diffusion_floats(orl_diffusion* d);          /* floats of the parameter block */
int orl_diffusion_num_tensors(orl_diffusion* d);
/* tensor idx of the block: its state_dict name, offset and shape (a conv weight is its centre tap, [out][in]) */
int orl_diffusion_tensor(orl_diffusion* d, int idx, char* name, int name_cap, int64_t* offset_floats, int32_t* ndim, int64_t shape[4]);
/* which: 0 parameters, 1 EMA parameters, 2 exp_avg, 3 exp_avg_sq; host arrays of orl_diffusion_floats floats */
int orl_diffusion_set(orl_diffusion* d, int which, const float* host, int64_t n_floats);
int orl_diffusion_get(orl_diffusion* d, int which, float* host, int64_t n_floats);
int orl_diffusion_set_step_count(orl_diffusion* d, int64_t k);   /* optimizer steps taken: Adam's t, the lr index, the EMA step, the RNG counter */
int64_t orl_diffusion_step_count(orl_diffusion* d);
/* acp: alphas_cumprod, float32 [N].  coef: float32 [N][5] per sampling step t = {sqrt(acp_t), sqrt(1 - acp_t), the x0 coefficient,
 * the x coefficient, sigma_t (0 at t = 0)} of the DDPM update  x <- c0 clip((x - s1 e) / s0, -1, 1) + c1 x + sigma z. */
int orl_diffusion_set_schedule(orl_diffusion* d, const float* acp, const float* coef);
/* the learning rate of optimizer step k, float64 [n], uploaded once; a step past the table is refused */
int orl_diffusion_set_lr(orl_diffusion* d, const double* table, int64_t n);
int orl_diffusion_attach_buffer(orl_diffusion* d, orl_buffer* b);    /* the dataset rows (obs, act) the steps gather */
/* One optimizer step on `rows` (1 .. batch_size) rows idx[] of the attached buffer: x_t, the network, the MSE against eps, the
 * backward, Adam with lr[k], the EMA.  t (int64 [rows], 0 .. N-1) and eps (float32 [rows][act_dim]) teacher-force the draws; NULL:
 * device Philox keyed by (seed, k, row).  All pointers are HOST pointers.  loss_out: the minibatch loss (synchronous). */
int orl_diffusion_step(orl_diffusion* d, const int64_t* idx, int32_t rows, const int64_t* t, const float* eps, float* loss_out);
/* ceil(n_rows / batch_size) steps over order[0 .. n_rows) (int64, a device pointer when on_device), the last one short; no host
 * synchronisation but the one at the end.  losses_out: host, one loss per step. */
int orl_diffusion_learn_epoch(orl_diffusion* d, const int64_t* order, int64_t n_rows, int on_device, float* losses_out);
/* select_action for n rows: x starts at init_noise (row i reads row noise_idx[i] of it when noise_idx is given, else row i), then
 * N forward-only passes on the EMA parameters with the DDPM update between them; z (float32 [N][n][act_dim], entry t used at step t > 0)
 * teacher-forces the update's noise, NULL: device Philox on a stream of its own.  obs [n][obs_dim], init_noise [*][act_dim],
 * act_out [n][act_dim]; every array is a device pointer when on_device.  One host synchronisation, at the end. */
int orl_diffusion_sample(orl_diffusion* d, const float* obs, int64_t n, const float* init_noise, const int64_t* noise_idx,
                         int64_t noise_rows, const float* z, int on_device, float* act_out);
/* test taps of the last step: "pred", "eps", "x_t", "t" (as floats), "gf" (the condition vector), "film", "loss", and the forward
 * activations it left in the training workspace: "e0" (the sinusoidal embedding), "mc" (Mish of the condition vector), "y1.<b>" and
 * "out.<b>" (block b of the layer table after its FiLM and at its output, b = 0 .. blocks - 1), "yf" (final_conv's GN + Mish); of the
 * last sample: "z" (the last noise drawn), "x".  Unknown names and a block index out of range are refused.  Returns the floats
 * written, < 0 on error. */
int64_t orl_diffusion_debug_read(orl_diffusion* d, const char* name, float* host, int64_t cap);
int orl_diffusion_debug_grads(orl_diffusion* d, float* host, int64_t n_floats);   /* parameter gradient of the last step */

/* -- RNNDynamics: the GRU sequence dynamics model (dynamics/rnn_dynamics.py, nets/rnn.py:RNNModel) ------------------------------
 * nn.GRU(in, H, L layers, batch_first, h0 = 0) beside a LayerNorm(dropout(swish(Linear))) input block, both merged by
 * swish(Linear(2H -> H)), then len(hidden) - 1 residual blocks LayerNorm(x + dropout(swish(Linear(x)))) and a Linear head.  Every
 * sequence array is [rows][T][cols], row-major.  Precision 0 (fp32 MFMA).
 * One object trains n_runs (1 .. 64) independent runs in the same launches: parameters, Adam moments and gradients are [n_runs][P] with
 * P = orl_rnn_floats, every run reads the one loaded data set through its own row indices, and run r draws the dropout stream of a
 * one-run object with seed + r.  Run r's results do not depend on n_runs, bit for bit.  On an object of several runs the one-run
 * entry points orl_rnn_set / _get / _step / _learn_epoch / _forward / _debug_read / _debug_grads are refused; use the _run / _runs
 * forms below, which are valid for n_runs == 1 too. */
typedef struct orl_rnn orl_rnn;
typedef struct {
  int32_t input_dim, output_dim;
  int32_t n_hidden;                 /* len(hidden_dims), 2 .. ORL_MAX_HIDDEN + 1 */
  int32_t hidden[ORL_MAX_HIDDEN + 1];   /* all equal: H, a multiple of 4 in [8, 512] */
  int32_t rnn_num_layers;           /* 1 .. 4 */
  float dropout_rate;               /* 0 <= p < 1 */
  int32_t batch_size;               /* most rows (sequences) of a training step */
  int32_t max_seq_len;              /* most time steps of a sequence */
  double lr, adam_beta1, adam_beta2, adam_eps;   /* doubles, as torch.optim.Adam holds them: 1 - beta is formed before the rounding to fp32 */
  int32_t n_runs, device, precision;
  uint64_t seed;                    /* of the dropout masks' Philox stream */
  void* external_arena;             /* device memory of n_runs * orl_rnn_config_floats floats that holds the parameters (run r's
                                       block at r * orl_rnn_config_floats floats), or NULL */
} orl_rnn_config;
void orl_rnn_config_default(orl_rnn_config* cfg);  /* hopper: 14 / 12, [200] * 4, 3 layers, p 0.1, batch 256, T 20, lr 1e-3 */
int64_t orl_rnn_config_floats(const orl_rnn_config* cfg);      /* floats of ONE run's parameter block of such a config; < 0: refused */
/* Refused: n_runs outside [1, 64], precision != 0, unequal hidden dims, H not a multiple of 4 or outside [8, 512], rnn_num_layers outside
 * [1, 4], n_hidden outside [2, ORL_MAX_HIDDEN + 1], dims < 1, dropout_rate outside [0, 1). */
int orl_rnn_create(const orl_rnn_config* cfg, orl_rnn** out);
void orl_rnn_destroy(orl_rnn* d);
int64_t orl_rnn_floats(orl_rnn* d);                             /* per run */
int orl_rnn_num_tensors(orl_rnn* d);
/* tensor idx of a run's block in RNNModel.state_dict() order: name, offset within the block (a multiple of 4 floats) and shape */
int orl_rnn_tensor(orl_rnn* d, int idx, char* name, int name_cap, int64_t* offset_floats, int32_t* ndim, int64_t shape[4]);
/* which: 0 parameters, 1 exp_avg, 2 exp_avg_sq; host arrays of orl_rnn_floats floats */
int orl_rnn_set(orl_rnn* d, int which, const float* host, int64_t n_floats);
int orl_rnn_get(orl_rnn* d, int which, float* host, int64_t n_floats);
int orl_rnn_set_run(orl_rnn* d, int run, int which, const float* host, int64_t n_floats);    /* the same on run `run`'s block */
int orl_rnn_get_run(orl_rnn* d, int run, int which, float* host, int64_t n_floats);
int orl_rnn_set_step_count(orl_rnn* d, int64_t k);       /* optimizer steps taken: Adam's t and the dropout counter (shared by the runs) */
int64_t orl_rnn_step_count(orl_rnn* d);
/* the data set into HBM, once: inputs [n][T][input_dim], targets [n][T][output_dim], masks [n][T] (host, float32); T <= max_seq_len */
int orl_rnn_load_data(orl_rnn* d, const float* inputs, const float* targets, const float* masks, int64_t n, int32_t T);
/* One optimizer step on `rows` (1 .. batch_size) sequences idx[] of the loaded data: forward in training mode, the masked MSE
 * (((pred - target)^2).mean(-1) * masks).mean(), the backward, Adam.  drop_masks: host float32 [len(hidden)][rows * T][H] keep masks
 * (1 keep, 0 drop; entry 0 the input block, entry 1 + i residual block i) teacher-force the dropout; NULL: device Philox keyed by
 * (seed, step count, block, row, column).  All pointers are HOST pointers.  loss_out: the minibatch loss (synchronous). */
int orl_rnn_step(orl_rnn* d, const int64_t* idx, int32_t rows, const float* drop_masks, float* loss_out);
/* The same step of every run at once: idx [n_runs][rows] (run r trains on its own rows), drop_masks [n_runs][len(hidden)][rows * T][H]
 * or NULL, losses_out [n_runs].  An index out of range in any run refuses the whole call. */
int orl_rnn_step_runs(orl_rnn* d, const int64_t* idx, int32_t rows, const float* drop_masks, float* losses_out);
/* ceil(n_rows / batch_size) steps over order[0 .. n_rows) (int64, a device pointer when on_device), the last one short; one host
 * synchronisation, at the end.  losses_out: host, one loss per step. */
int orl_rnn_learn_epoch(orl_rnn* d, const int64_t* order, int64_t n_rows, int on_device, float* losses_out);
/* The same with one order per run: orders [n_runs][n_rows] (a device pointer when on_device), losses_out [steps][n_runs]; one host
 * synchronisation, at the end. */
int orl_rnn_learn_epoch_runs(orl_rnn* d, const int64_t* orders, int64_t n_rows, int on_device, float* losses_out);
/* eval-mode forward (no dropout) of n sequences inputs [n][T][input_dim], 1 <= T <= max_seq_len: out_last [n][output_dim] is the
 * prediction of the last time step, out_all [n][T][output_dim] (or NULL) every step's.  Device pointers when on_device. */
int orl_rnn_forward(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, float* out_last, float* out_all);
/* run >= 0: that run alone on inputs [n][T][input_dim], outputs as orl_rnn_forward's.  run == -1: every run, on the same inputs
 * [n][T][input_dim] when shared_inputs != 0 and on inputs [n_runs][n][T][input_dim] otherwise; out_last [n_runs][n][output_dim],
 * out_all [n_runs][n][T][output_dim] or NULL. */
int orl_rnn_forward_runs(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, int shared_inputs, int run, float* out_last,
                         float* out_all);
/* test taps of the last step (or of the last forward when it came later), [rows * T][cols] each: "pred", "gru.<l>" (layer l's
 * output), "in" (the input block's output), "merge", "block.<i>" (residual block i's output), "mask.<s>" (the keep mask of dropout
 * s, training only), "act.<s>" (what that dropout reads) and "drop.<s>" (what its LayerNorm reads); and "loss".  Unknown names are
 * refused.  Returns the floats written, < 0 on error. */
int64_t orl_rnn_debug_read(orl_rnn* d, const char* name, float* host, int64_t cap);
int orl_rnn_debug_grads(orl_rnn* d, float* host, int64_t n_floats);   /* parameter gradient of the last step */
/* the same taps of run `run` (one that the last pass computed) */
int64_t orl_rnn_debug_read_run(orl_rnn* d, int run, const char* name, float* host, int64_t cap);
int orl_rnn_debug_grads_run(orl_rnn* d, int run, float* host, int64_t n_floats);
/* Further taps, of both forms: "x0" (the gathered or given inputs, [rows * T][input_dim]) and "gi.<l>" (layer l's input projections,
 * [rows * T][3H]) after a step or a forward; and what only a training step computes, refused after a forward:
 *   "tgt" [rows * T][output_dim], "msk" [rows * T]          the gathered targets and loss masks
 *   "r.<l>", "z.<l>", "n.<l>", "hn.<l>", "hp.<l>"          what layer l's forward scan saves: the gates, W_hn h + b_hn, h_{t-1}
 *   "zpre.<s>", "zmerge"                                   the Swish pre-activations of norm slot s's Linear and of the merge layer
 *   "dpred", "dx", "dzm", "dcat" ([rows * T][2H])          gradients of pred, of the last block's output, of zmerge, of the merge input
 *   "du.<i>", "dt.<i>"                                     block i's LayerNorm-input gradient and its Linear's input gradient
 *   "dz.<s>"                                               the Linear-output gradient of norm slot s (0 the input block, 1 + i block i)
 *   "dgi.<l>", "dgh.<l>" ([rows * T][3H]), "dxl.<l>"       layer l's backward scan outputs; the gradient of layer l's input, l >= 1
 *   "part" [rows * T][2 H len(hidden)], "chunk" [ceil(rows * T / 64)][..]   the dgamma | dbeta row terms and their 64-row sums
 *   "slab.<k>" [orl_rnn_floats]                            slab k of the split weight gradients (one the last step wrote)
 * du, dt, dz, dgi, dgh and dxl live in buffers that the stages of a step share: the name of a stage that a later one has overwritten
 * is refused (readable: index 0, and dxl.1 / dxl.2), unless orl_rnn_debug_keep is on. */
/* Tests only.  on != 0: every backward stage of the following steps writes a matrix of its own (same pitches and run strides as the
 * shared ones; no kernel, launch or copy is added, and the results are the same bits), so that all of them can be read back; 0: the
 * shared buffers again (the default) and the extra matrices freed.  Either change waits for the stream and forgets the last step's taps. */
int orl_rnn_debug_keep(orl_rnn* d, int on);
/* Timing of the training steps with device events (off by default).  While enabled every step records events around its phases;
 * orl_rnn_profile_read waits for the last step and writes its milliseconds: ms[0] the whole step, [1] the forward, [2] the forward
 * scans of all layers, [3] the loss and the backward, [4] the backward scans of all layers, [5] Adam. */
int orl_rnn_profile(orl_rnn* d, int enable);
int orl_rnn_profile_read(orl_rnn* d, float ms[6]);
/* -- carried GRU state: one model step at a time (what a rollout needs) ----------------------------------------------------------
 * The object keeps the h of every GRU layer of n_traj trajectories in HBM, [n_runs][L][n_traj][H]: trajectory j in slot j.  A step of
 * n rows reads the h of each row's trajectory, applies ONE GRU step per layer (k_rnn_cell: the input projection, the recurrent
 * product and the gates in one launch per layer), writes the new h back to the slot, and runs the tail of the window forward on the
 * n rows: O(1) work per model step at any horizon, no history on the host.  In exact arithmetic k steps from a zero state equal the
 * window forward over the k inputs; in fp32 the two differ by rounding (other products, other orders).  The state is kept twice, with
 * a side bit per (run, slot) that names the buffer holding the slot's h: a step reads that buffer and writes the other one (the
 * workgroups of a row each read the whole previous row while their neighbours write parts of the new one), and its last launch flips
 * the bits of the slots it stepped.  A slot that a step does not name keeps its bits, so any subset may be stepped at any time.
 * No atomics: identical call sequences give identical bits, and run r's bits do not depend on n_runs.
 *
 * orl_rnn_set_scaler: the input scaler (StandardScaler's mu and std, input_dim host floats each, shared by the runs).
 * orl_rnn_state_reset: (re)allocates the state for n_traj trajectories and zeroes it, in every run.
 * orl_rnn_state_prime: starts slots 0 .. n - 1 of every run from a history: the eval forward over the ALREADY SCALED windows inputs
 *   [n][T][input_dim] (shared_inputs != 0) or [n_runs][n][T][input_dim], then each layer's h of the last time step into the slots.
 *   n <= n_traj; the other slots are untouched.  Device pointer when on_device.
 * orl_rnn_state_step: one model step of n <= n_traj rows.  obs [n][obs_dim], act [n][act_dim] (unscaled: the step applies the scaler),
 *   obs_dim = output_dim - 1 (the model predicts [delta obs | reward]) and act_dim = input_dim - obs_dim, refused when < 1.  index
 *   [n] int64: the trajectory of row i, NULL: 0 .. n - 1; the indices must be distinct and < n_traj (host indices are checked, device
 *   ones are clamped into the state by the kernels and are the caller's to keep distinct).  run >= 0: that run alone; run == -1: every
 *   run, obs / act / next_obs / reward with a leading n_runs and the index shared.  next_obs [n][obs_dim] = pred[:, :-1] + obs, reward
 *   [n] = pred[:, -1].  All pointers are device pointers when on_device, host pointers otherwise.  Synchronous.
 * orl_rnn_state_set: plants layer `layer` of run `run`, host [n_traj][H] (tests).
 * Taps (orl_rnn_debug_read_run): "state.<l>" [n_traj][H], the carried h of layer l; after a state step "roll.x" [n][input_dim] (the
 * scaled inputs), "roll.h.<l>" [n][H] (the new h in row order), "roll.pred" [n][output_dim], and the tail's names above with n rows
 * ("gi.<l>" is refused: the one-step path keeps no input projections). */
int orl_rnn_set_scaler(orl_rnn* d, const float* mu, const float* std, int64_t n);
int orl_rnn_state_reset(orl_rnn* d, int64_t n_traj);
int orl_rnn_state_prime(orl_rnn* d, const float* inputs, int64_t n, int32_t T, int on_device, int shared_inputs);
int orl_rnn_state_step(orl_rnn* d, const float* obs, const float* act, const int64_t* index, int64_t n, int on_device, int run, float* next_obs,
                       float* reward);
int orl_rnn_state_set(orl_rnn* d, int run, int layer, const float* host, int64_t n_traj);

#ifdef __cplusplus
}
#endif
#endif /* ORL_ENGINE_H */
