/* carl_amd.h -- C ABI of the MI355X batched step/reset engine for CARL's
 * contextual classic-control (and Brax-locomotion) families: reset / step / fused open-loop rollout for both, and the
 * closed-loop rollout with a policy network on the device (carl_rollout_policy and its sampled / valued / episodes / ES
 * forms for the classic-control families; carl_brax_rollout_policy, transitions and summary, its sampled form
 * carl_brax_rollout_policy_sampled and carl_brax_evaluate_policy, whole episodes, for Brax).
 *
 * The reference (automl/CARL v1.1.1) has NO FFI on this path: its boundary is a
 * Python protocol, "the object CARLEnv wraps" (SURVEY.md section 8b).  This header
 * is what a ctypes binding on the reference side would load (INTEGRATION.md shows
 * the stub).  Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no torch/HIP types in signatures:
 *    `stream` is a hipStream_t passed as void* (0 = the null stream).
 *  - All array pointers are DEVICE pointers owned by the caller (the Python shim
 *    allocates them as PyTorch-ROCm tensors and passes tensor.data_ptr()).  The
 *    library never allocates persistent device memory and never frees caller
 *    memory; scratch is caller-provided.
 *  - Calls enqueue on `stream` and return without synchronising; one carl_batch_t per
 *    device, caller serialises calls per batch.  No global mutable state that a result
 *    depends on: the only process-wide data is a mutex-guarded record of which kernels
 *    were already granted > 48 KiB of dynamic LDS (an idempotent driver attribute).
 *  - Return value: 0 on success, otherwise a hipError_t value or CARL_ERR_*;
 *    carl_last_error() returns a thread-local message.  Nothing throws or exits.
 *  - Layouts: per-lane state is struct-of-arrays  state[s * n_lanes + lane];
 *    the context table is feature-major  ctx_table[f * ctx_stride + c]  with
 *    features in the order of the reference class's get_context_features();
 *    observations are lane-major  obs[lane * obs_dim + d]  (what a VectorEnv
 *    returns: carl/envs/brax/wrappers.py:111-118).
 */
#ifndef CARL_AMD_H_
#define CARL_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARL_ABI_VERSION 9
#define CARL_MAX_CTX_OBS 32

#define CARL_ERR_INVALID_ARGUMENT (-1)
#define CARL_ERR_UNSUPPORTED (-2)

/* env families.  Context-feature order per family = get_context_features():
 *  CARTPOLE          carl/envs/gymnasium/classic_control/carl_cartpole.py:15-42
 *  PENDULUM          carl/envs/gymnasium/classic_control/carl_pendulum.py:15-39
 *  ACROBOT           carl/envs/gymnasium/classic_control/carl_acrobot.py:15-69
 *  MOUNTAINCAR       carl/envs/gymnasium/classic_control/carl_mountaincar.py:15-51
 *  MOUNTAINCAR_CONT  carl/envs/gymnasium/classic_control/carl_mountaincarcontinuous.py:15-48 */
typedef enum carl_family {
  CARL_CARTPOLE = 0,
  CARL_PENDULUM = 1,
  CARL_ACROBOT = 2,
  CARL_MOUNTAINCAR = 3,
  CARL_MOUNTAINCAR_CONT = 4,
  CARL_N_FAMILIES = 5
} carl_family_t;

/* per-lane context selection rule applied on every reset of a lane
 * (carl/context/selection.py: StaticSelector :125-136, RoundRobinSelector
 * :110-122, RandomSelector :98-107).  HOST = ids are written by the caller
 * (CustomSelector :139-180); the device leaves ctx_idx alone. */
typedef enum carl_selector {
  CARL_SEL_STATIC = 0,
  CARL_SEL_ROUND_ROBIN = 1,
  CARL_SEL_RANDOM = 2,
  CARL_SEL_HOST = 3
} carl_selector_t;

enum {
  CARL_FLAG_AUTORESET = 1,          /* reset done lanes inside step */
  CARL_FLAG_CARTPOLE_RECOMPUTE = 2, /* recompute total_mass / polemass_length from
                                       the context (NOT reference behaviour; the
                                       default replicates Quirk C1) */
  CARL_FLAG_ACROBOT_FP32 = 4,       /* evaluate Acrobot's _dsdt/rk4 in fp32 instead of
                                       fp64 (faster; up to ~1e-3 relative error on
                                       states near the velocity bounds).  Without the flag the step is float64
                                       ARITHMETIC, not a float64 reference: sin / cos come from a 512-entry table with a
                                       short correction (7e-14), 1 / det from v_rcp_f64 + one Newton step (4e-15), the
                                       angle wrap is x - rint(x / 2 pi) 2 pi (the reference's strict > pi / < -pi
                                       compares differ for the doubles within one ulp of +-pi), the state is stored as
                                       float32 and the observation / _terminal trig is taken at the STORED angles
                                       (2e-7 from the reference's unrounded ones).  Each transition is within 1e-5 of
                                       gymnasium's arithmetic; Acrobot is chaotic, so free-running trajectories
                                       separate from a true float64 run at the float32 state rounding's rate */
  CARL_FLAG_ROLLOUT_DIRECT = 16,    /* carl_rollout: launch the direct-store kernel even where the staged one
                                       applies (A/B measurements and tests; ~50 % slower, same results) */
  CARL_FLAG_AUTORESET_FIRST_STATE = 8 /* Brax families, with AUTORESET: a done env is put back to the state
                                       its last explicit reset produced -- no new draw, no selector advance,
                                       no context change: brax.envs.wrappers.training.AutoResetWrapper as the
                                       reference reaches it through carl/envs/brax/wrappers.py:54-78,121-145
                                       (needs carl_batch_t::first_state).  Default: re-draw. */
  ,
  CARL_FLAG_BRAX_GENERIC = 32         /* Brax families: step planar models (Halfcheetah, Hopper, Walker2d) with the general
                                       3-D substep too -- the A/B and test switch for the planar substep, which the
                                       library otherwise picks for models whose joints and geometry lie in the y = 0
                                       plane (same records, same results to rounding, a third of the instructions).  A
                                       planar model's state must BE planar (what reset produces); a caller that sets
                                       an out-of-plane state itself passes this flag. */
  ,
  CARL_FLAG_BRAX_FP32 = 64            /* Brax families, OPT-IN, never a default (ABI 9): carl_brax_step / carl_brax_rollout run the
                                       n_frames substeps of an env step with their pose algebra (anchor separation, relative
                                       joint rotation, joint angles, contact depth, integration) in float32 -- the precision
                                       brax itself runs at under JAX's default (carl/envs/brax/carl_brax_env.py:163-176 creates
                                       the env without enabling x64).  The product path forms these differences of poses in
                                       float64 to stay within north_star's 1e-5 of the float64 restatement; this flag tells a
                                       user what that bar costs: faster, and off the restatement by the amounts reported in
                                       profiles/r06_brax_fp32_deviation.txt (like CARL_FLAG_ACROBOT_FP32 for the classic
                                       path).  Between env steps the state record is the same 48-bit pose; reset, observe
                                       and reward are unchanged.  Not built for the reach / push task models
                                       (CARL_ERR_UNSUPPORTED). */
};

/* Storage type of carl_step_io.action.  The reference's discrete action is whatever integer the caller's policy
 * produced (gymnasium Discrete: np.int64; carl/envs/carl_env.py:321 passes it through): I32 / I64 everywhere.
 * U8 (ABI 7) is a ROLLOUT-ONLY input format for discrete families: one byte per lane-step -- the action stream is the
 * fused rollout's only per-step read, and at 4 bytes it costs a fifth of a CartPole launch.  Accepted by carl_rollout
 * in its lean staged configuration (row pitch % 16 == 0 -- dense rows: n_lanes % 16 == 0 --, STATIC / HOST selector, no
 * finished-episode log, no final_obs;
 * action pointer 4-byte aligned); anything else returns CARL_ERR_UNSUPPORTED and the caller widens the actions.
 * Same values in, same transitions out: bit-identical to the I32 launch (tests/test_gpu_parity.py). */
enum { CARL_ACTION_I32 = 0, CARL_ACTION_I64 = 1, CARL_ACTION_F32 = 2, CARL_ACTION_U8 = 3,
       /* Box families, carl_rollout's lean staged configuration only (pointer 8-byte aligned): IEEE float16 / bfloat16 as
        * a policy network under autocast emits them; widened exactly, so the transitions are those of the float32
        * launch fed the widened values */
       CARL_ACTION_F16 = 4, CARL_ACTION_BF16 = 5 };

typedef struct carl_family_info {
  int32_t state_dim;          /* S: columns of `state` */
  int32_t obs_dim;            /* D */
  int32_t n_features;         /* F: rows of ctx_table */
  int32_t action_dim;         /* 1 */
  int32_t action_is_discrete; /* 1: Discrete(n_actions); 0: Box */
  int32_t n_actions;          /* discrete: 2 or 3 */
  int32_t max_episode_steps;  /* gymnasium registry TimeLimit default */
  int32_t reserved;
  float action_low, action_high; /* Box bounds when continuous */
} carl_family_info_t;

/* One batch of lanes (env instances) resident on one device.  Replaces the
 * attribute state of N x {CARLEnv + TimeLimit + gymnasium env} objects:
 *   state      <- env.unwrapped.state              (carl_cartpole.py:51 ...)
 *   elapsed    <- TimeLimit._elapsed_steps         (gymnasium.make, carl_gymnasium_env.py:64)
 *   ctx_idx    <- context_selector.context_id      (carl_env.py:118-120)
 *   n_calls    <- context_selector.n_calls         (selection.py:45,75)
 *   ctx_table  <- env.contexts after insert_defaults (carl_env.py:122-137) and the
 *                 setattr loop of CARLGymnasiumEnv._update_context
 *                 (carl_gymnasium_env.py:75-77)
 *   ctx_obs    <- the "context" half of the observation dict (carl_env.py:276-305)
 * RNG: Philox4x32-10, key = seed, counter = (global lane id lo, hi, episode, sub);
 * global lane id = lane_offset + lane, so results do not depend on how lanes are
 * split across devices. */
typedef struct carl_batch {
  int32_t family;            /* carl_family_t */
  int32_t n_lanes;
  int32_t n_contexts;        /* C: valid columns of ctx_table */
  int32_t ctx_stride;        /* elements between feature rows, >= n_contexts */
  int32_t max_episode_steps; /* TimeLimit; <= 0 -> never truncate */
  int32_t selector;          /* carl_selector_t */
  int32_t selector_stride;   /* round robin: id = (id + stride) mod C */
  int32_t flags;             /* CARL_FLAG_* */
  int64_t lane_offset;
  uint64_t seed;
  /* persistent per-lane state */
  float* state;              /* [S][n_lanes] */
  int32_t* elapsed;          /* [n_lanes] */
  int32_t* ctx_idx;          /* [n_lanes] in [0, C) */
  uint32_t* episode;         /* [n_lanes] resets so far under this seed (RNG counter) */
  int32_t* n_calls;          /* [n_lanes] selector calls so far */
  float* ep_return;          /* [n_lanes] running return of the current episode */
  /* contexts */
  const float* ctx_table;    /* [F][ctx_stride] */
  float* ctx_obs;            /* [n_ctx_obs][n_lanes] or NULL */
  int32_t n_ctx_obs;
  int32_t ctx_obs_feat[CARL_MAX_CTX_OBS]; /* table row of each observed feature */
  int32_t fin_capacity;      /* entries in the finished-episode log */
  /* episode statistics, all nullable */
  float* last_return;        /* [n_lanes] return of the lane's last finished episode */
  int32_t* last_length;      /* [n_lanes] */
  int32_t* episodes_done;    /* [n_lanes] finished-episode count */
  /* finished-episode log (wave-ballot compaction, one atomic per wavefront):
   * entry k < min(*fin_count, fin_capacity) = one finished episode.  Entry order
   * is unspecified; the multiset of entries is deterministic. */
  int32_t* fin_count;        /* [1] or NULL */
  int64_t* fin_lane;         /* [fin_capacity] global lane id */
  float* fin_return;         /* [fin_capacity] */
  int32_t* fin_length;       /* [fin_capacity] */
  /* goal-directed Brax mode (BraxWalkerGoalWrapper, brax_walker_goal_wrapper.py:113-140);
   * NULL otherwise */
  float* goal_pos;           /* [2][n_lanes] position integrated from the observed x/y velocities */
  uint8_t* success;          /* [n_lanes] (or [T][n_lanes] in a rollout): goal reached on this step */
  /* Brax families, CARL_FLAG_AUTORESET_FIRST_STATE: [n_lanes][20 L] (records like `state`), written by carl_brax_reset, read by the
   * in-kernel auto-reset; NULL otherwise */
  float* first_state;
} carl_batch_t;

/* Inputs/outputs of one step (or, for carl_rollout, of T steps: every array gains
 * a leading [T] dimension).  Replaces the return tuple of CARLEnv.step
 * (carl/envs/carl_env.py:321-342) minus the context half (see carl_batch.ctx_obs). */
typedef struct carl_step_io {
  const void* action;   /* [n_lanes * action_dim], dtype per action_dtype */
  int32_t action_dtype; /* CARL_ACTION_* ; discrete families take I32/I64 (carl_rollout also U8), Box F32 (carl_rollout
                           also F16 / BF16) */
  int32_t row_pitch;    /* carl_rollout / carl_rollout_pair (classic-control families; ABI 9): lanes per ROW of `action` and of
                           every [T][...] output -- row t of an array starts row_pitch lanes after row t - 1; 0 = n_lanes (dense
                           rows).  Must be 0 or >= n_lanes.  The staged kernel (16-byte stores) runs when the pitch is a multiple
                           of 16 AND either n_lanes is one too or the pitch is exactly carl_rollout_pitch(n_lanes): it then also
                           WRITES columns [n_lanes, carl_rollout_pitch(n_lanes)) of every output row (the records of the padding
                           lanes) and reads the same columns of the action rows, which must hold valid actions (the engine
                           repeats the last lane's) -- never anything beyond.  Any other pitch (a view into a wider array) takes
                           the direct-store kernel, which touches columns [0, n_lanes) only.  Ignored by carl_step; the Brax
                           entry points take 0 only.  (this field was `reserved`, always 0, in ABI <= 8) */
  float* obs;           /* [n_lanes][D]; with AUTORESET the post-reset observation
                           for done lanes (gymnasium vector-env convention) */
  float* reward;        /* [n_lanes] */
  uint8_t* terminated;  /* [n_lanes] */
  uint8_t* truncated;   /* [n_lanes] TimeLimit */
  float* final_obs;     /* [n_lanes][D] or NULL; written for done lanes only */
  uint8_t* done;        /* [n_lanes] or NULL: terminated | truncated, the done mask of this step (what
                           info["_final_observation"] of a vector env is); per-call carl_step / carl_brax_step
                           only, ignored by the rollout entry points */
  uint32_t* branch_sig; /* Brax families: [n_lanes][2] or NULL.  Hash of the DISCRETE decisions the physics took in
                           this env step: [0] which collision spheres delivered an impulse in which substep
                           (discontinuous: an impulse appears when a point starts to approach; push task: also which
                           gripper / object contacts pushed -- round 6), [1] which joint
                           range limits were active (continuous: the limit spring starts at zero).  Two
                           implementations of the same arithmetic can only be compared to rounding on lanes
                           whose word [0] agrees; tests/test_gpu_brax.py uses it for exactly that.  Ignored by
                           the classic-control entry points. */
} carl_step_io_t;

int carl_abi_version(void);
const char* carl_last_error(void);

/* static facts about a family: replaces reading env.observation_space /
 * env.action_space / spec.max_episode_steps of the gymnasium env the reference
 * builds with gymnasium.make (carl_gymnasium_env.py:63-64). */
int carl_family_info(int family, carl_family_info_t* out);

/* CARLEnv.reset for the lanes selected by `mask` (device u8 [n_lanes]; NULL = all):
 * selector advance -> (context switch) -> CARL init-state draw -> elapsed = 0 -> obs.
 * Replaces carl/envs/carl_env.py:245-274 + the per-family reset overrides
 * (carl_cartpole.py:44-66, carl_pendulum.py:41-65, carl_acrobot.py:71-115,
 * carl_mountaincar.py:53-85, carl_mountaincarcontinuous.py:50-82).
 * `obs` [n_lanes][D] receives the initial observation of reset lanes only. */
int carl_reset(const carl_batch_t* batch, const uint8_t* mask, float* obs, void* stream);

/* Same, for the compact list idx[0 .. *count) produced by carl_done_compact
 * ("reset_masked over the compacted done list"). */
int carl_reset_indexed(const carl_batch_t* batch, const int32_t* idx, const int32_t* count,
                       float* obs, void* stream);

/* CARLEnv.step over all lanes: env physics + TimeLimit + episodic-return
 * bookkeeping + (AUTORESET) in-kernel reset of done lanes.  Replaces
 * carl/envs/carl_env.py:321-342 -> gymnasium TimeLimit.step -> <Env>.step. */
int carl_step(const carl_batch_t* batch, const carl_step_io_t* io, void* stream);

/* T consecutive steps in ONE launch, state held in registers between steps; every
 * step still emits its full transition (obs/reward/terminated/truncated at
 * [t][lane]).  action is [T][n_lanes].  No reference counterpart (the reference
 * steps one env object per Python call); exists because a single step of 65 536
 * lanes is shorter than a kernel launch. */
int carl_rollout(const carl_batch_t* batch, const carl_step_io_t* io, int32_t n_steps, void* stream);

/* T consecutive steps of TWO batches of different classic-control families in ONE launch: BASELINE config 3's mixed
 * batch ("CARLAcrobot + CARLMountainCar", carl/envs/gymnasium/classic_control/carl_acrobot.py:11-115 +
 * carl_mountaincar.py:11-85 -- in the reference two unrelated env objects, carl/envs/carl_env.py:245-342 holds no
 * cross-env state).  One part must be the float64 Acrobot, the other any other family; both in the lean staged
 * configuration (row pitch % 16 == 0, static / host selector, no finished-episode log, io.final_obs NULL, int32 /
 * float32 actions).  Each family's workgroups run the same staged rollout as carl_rollout at 4-step chunks, so one
 * workgroup of each fits a compute unit and the second family's wavefronts issue in the gaps of Acrobot's RK4:
 * results are bit-identical to two carl_rollout calls, the launch takes ~max instead of the sum.
 * Returns CARL_ERR_UNSUPPORTED (nothing enqueued) for any other combination: the caller then makes the two
 * carl_rollout calls itself (carl_amd.mixed.MixedVecEngine.rollout does). */
int carl_rollout_pair(const carl_batch_t* batch_a, const carl_step_io_t* io_a, const carl_batch_t* batch_b,
                      const carl_step_io_t* io_b, int32_t n_steps, void* stream);

/* Which kernel carl_rollout launches for this batch (classic-control families).  The staged kernel (transition
 * records assembled in LDS, written with 16-byte stores by dedicated waves) needs rows of a pitch that is a multiple of
 * 16 lanes; this entry point answers for DENSE rows (io.row_pitch = 0: n_lanes % 16 == 0).  Any other lane count
 * silently took the ~50 % slower direct-store kernel in ABI <= 4; a caller could ask since ABI 5; since ABI 9 it lays
 * its rows out at carl_rollout_pitch(n_lanes) and gets the staged kernel (carl_rollout_variant_io). */
enum { CARL_ROLLOUT_STAGED = 0, CARL_ROLLOUT_DIRECT_SHAPE = 1, CARL_ROLLOUT_DIRECT_FLAG = 2 };
int carl_rollout_variant(const carl_batch_t* batch); /* CARL_ERR_INVALID_ARGUMENT for a non-classic family */
/* ... for this batch WITH these buffers (ABI 9): the staged kernel needs (io->row_pitch ? io->row_pitch : n_lanes) % 16
 * == 0 -- a caller whose lane count is not a multiple of 16 lays its rows out at carl_rollout_pitch(n_lanes) and gets
 * the staged kernel (carl_amd.engine.VecEngine.alloc_rollout does; uneven lane shards of a multi-GPU run end up here:
 * carl_amd/distributed.py::lane_shard).  No reference counterpart: the reference has no batched layout at all
 * (carl/envs/carl_env.py:321-342 returns one env's tuple). */
int carl_rollout_variant_io(const carl_batch_t* batch, const carl_step_io_t* io);
/* ... and which INSTANCE (additive; ABI version unchanged: a new symbol and a new struct, no existing layout moves): what
 * the library's one launch rule decided for this batch with these buffers, field by field -- rollout_staged_kernel's
 * template arguments and dynamic LDS where variant == CARL_ROLLOUT_STAGED, and the LDS argument / block size of the
 * reset, per-call step and direct-store rollout kernels.  Host logic only (no HIP call, no allocation, nothing
 * dereferenced: the pointers' alignment is all that is read), so a test can hold a table of configurations against it
 * without a GPU.  io NULL = dense rows, aligned arrays, int32 actions (as carl_rollout_variant).  No reference
 * counterpart.  Returns 0, or CARL_ERR_INVALID_ARGUMENT (NULL batch / out, a non-classic family, n_lanes < 0,
 * n_contexts <= 0, io.row_pitch < n_lanes).  The action dtype is reported as given: whether the family accepts it is
 * carl_step's / carl_rollout's own check. */
typedef struct carl_rollout_plan {
  int32_t variant;      /* CARL_ROLLOUT_* */
  int32_t lean;         /* the lean staged configuration (static / host selector, no finished-episode log, no final_obs) */
  int32_t unsupported;  /* a narrow action format outside the lean staged configuration: carl_rollout declines */
  int32_t ak;           /* action kind: 0 int32 / float32, 1 int64, 2 uint8, 3 float16, 4 bfloat16 */
  int32_t plain, ldsctx, moves, fin, ar, deep; /* rollout_staged_kernel<Fam, AK, PLAIN, LDSCTX, MOVES, FIN, AR, DEEP> */
  int32_t has_staged_kernel; /* an instance with these arguments exists (variant == CARL_ROLLOUT_STAGED only) */
  int32_t use_lds_ctx;  /* reset / step / direct rollout kernels: context table staged in LDS (their LDS argument) */
  int32_t step_block;   /* threads per workgroup of a carl_step launch */
  int32_t acrobot_fp32; /* the batch runs the float32 Acrobot (CARL_FLAG_ACROBOT_FP32 on CARL_ACROBOT) */
  int64_t lds_bytes;    /* dynamic LDS of the staged launch */
} carl_rollout_plan_t;
int carl_rollout_plan_io(const carl_batch_t* batch, const carl_step_io_t* io, carl_rollout_plan_t* out);
int32_t carl_rollout_pitch(int32_t n_lanes); /* n_lanes rounded up to the next multiple of 16 (0 for n_lanes <= 0) */

/* done-mask compaction: ascending lane ids with terminated|truncated set.
 * idx_out [n], count_out [1], scratch >= carl_done_compact_scratch_elems(n) int32.
 * No reference counterpart (the gymnasium path has no auto-reset; the user calls
 * reset() per env, carl_env.py:245). */
int carl_done_compact(const uint8_t* terminated, const uint8_t* truncated, int32_t n,
                      int32_t* idx_out, int32_t* count_out, int32_t* scratch, void* stream);
int32_t carl_done_compact_scratch_elems(int32_t n);

/* ======================= closed-loop rollout: a policy network on the device (ABI 9, additive) =======================
 * carl_rollout takes actions written before the launch (open loop).  carl_rollout_policy evaluates a small fp32 MLP
 * for every lane at every step instead, and that step takes the action it yields: the workload of evaluating a
 * trained agent over a context set (the reference's examples/carl_with_sb3.py trains a policy on
 * FlattenObservation(env); carl/envs/carl_env.py:276-305 builds what it sees).  Classic-control families only: a
 * Brax batch (family >= CARL_N_FAMILIES) is refused here -- the Brax families have carl_brax_rollout_policy, a mode of
 * their own rollout kernel, further down; the episodes mode, sampling, the critic, ES and the input statistics below
 * stay classic-control only -- and so are the pair launch (carl_rollout_pair) and the
 * narrow action formats -- the kernel writes the actions it takes, it reads none.
 *
 * The policy's input is what FlattenObservation(env) yields for a lane:
 *   x = [ctx_table[ctx_rows[0]][c], ..., ctx_table[ctx_rows[n_ctx - 1]][c], obs_0, ..., obs_{D-1}]
 * with c the lane's CURRENT context (after any auto-reset of the previous step) and obs the lane's current
 * observation (before the step).  n_in = n_ctx + D.  Then
 *   x = min(max((x - shift) * scale, -clip), clip)          (SB3 VecNormalize; shift 0, scale 1, clip inf: identity;
 *                                                            a NaN -- a NaN input, or 0 * inf -- becomes -clip)
 *   h = act(W_l h + b_l)  for each of the n_hidden layers     (act: CARL_POLICY_* below, the same for every layer)
 *   y = W_head h + b_head                                    (n_out values)
 * Discrete families: the action is the index of the largest y (the first one on ties: `>` comparisons); n_out must
 * be carl_family_info().n_actions.  Box families: the action is y[0] as it comes (n_out = 1), and the env clips it
 * exactly as it clips an action given to carl_rollout.  Every product is an explicit fma (in input order, bias
 * first); tanh is evaluated as 1 - 2 / (exp(2 v) + 1) with the hardware exponential and reciprocal (within 6 * 2^-24
 * absolute; exactly +-1 once exp(2 v) overflows or underflows).  The kernel pads the network to a fixed width with
 * zero weights and forces padded hidden units to 0: the padding changes no result, infinite inputs included.
 *
 * Packed parameters, float32, one block of carl_policy_set_floats() floats per weight set (set k at params +
 * k * carl_policy_set_floats(p)), each block: for every layer in order (hidden layers, then the head) W[out][in]
 * row-major followed by b[out]; then shift[n_in], scale[n_in], clip (one value for every input); zero padding up to a
 * multiple of 4 floats.  Lane l uses weight set l / lanes_per_set; lanes_per_set is a positive multiple of
 * carl_policy_lane_quantum() (the lanes of one workgroup: it stages one set in LDS) and n_sets * lanes_per_set must
 * cover n_lanes. */
#define CARL_POLICY_MAX_IN 32
#define CARL_POLICY_MAX_HIDDEN 2
#define CARL_POLICY_MAX_WIDTH 64
enum { CARL_POLICY_IDENTITY = 0, CARL_POLICY_TANH = 1, CARL_POLICY_RELU = 2 };  /* hidden-layer activation */
enum { CARL_POLICY_HEAD_ARGMAX = 0, CARL_POLICY_HEAD_BOX = 1 };               /* discrete / Box families */

typedef struct carl_policy {
  int32_t n_in;                          /* n_ctx + obs_dim */
  int32_t n_ctx;                         /* leading inputs that are context values */
  int32_t ctx_rows[CARL_POLICY_MAX_IN];  /* [n_ctx] context-table row of each, in FlattenObservation order; < F */
  int32_t n_hidden;                      /* 0 (a linear policy) .. CARL_POLICY_MAX_HIDDEN */
  int32_t width[CARL_POLICY_MAX_HIDDEN]; /* [n_hidden] 1 .. CARL_POLICY_MAX_WIDTH */
  int32_t n_out;                         /* head width */
  int32_t activation;                    /* CARL_POLICY_IDENTITY / TANH / RELU */
  int32_t head;                          /* CARL_POLICY_HEAD_ARGMAX (discrete) / CARL_POLICY_HEAD_BOX */
  int32_t n_sets;                        /* >= 1 */
  int32_t lanes_per_set;                 /* multiple of carl_policy_lane_quantum(); n_sets * lanes_per_set >= n_lanes */
  int32_t reserved;
  const float* params;                   /* DEVICE [n_sets][carl_policy_set_floats()] */
} carl_policy_t;

/* per-lane totals of one launch (summary mode; optional in transitions mode) */
typedef struct carl_policy_summary {
  int32_t* episodes;   /* [n_lanes] episodes finished in the launch */
  float* return_sum;   /* [n_lanes] fp32 sum of their returns, added in step order */
  int32_t* length_sum; /* [n_lanes] sum of their lengths */
} carl_policy_summary_t;

/* T steps of every lane in ONE launch, each step's action chosen by `policy_host` (a HOST pointer; its `params` are on
 * the device).  No reference counterpart on this path: the reference steps one env object per Python call and its
 * caller runs the policy between the calls (carl/envs/carl_env.py:321-342).
 *  - transitions mode (io != NULL): everything carl_rollout writes (obs / reward / terminated / truncated per step,
 *    io->final_obs when not NULL, the engine state at the end), plus the action taken at step t in row t of
 *    io->action -- an OUTPUT here: int32 (CARL_ACTION_I32) for discrete families, float32 (CARL_ACTION_F32) for Box
 *    ones.  Row layout as carl_rollout's staged kernel: (io->row_pitch ? io->row_pitch : n_lanes) % 16 == 0 and
 *    either n_lanes % 16 == 0 or the pitch is carl_rollout_pitch(n_lanes) (the padding columns receive the padding
 *    lanes' records), every array on a 16-byte boundary; other layouts return CARL_ERR_UNSUPPORTED.
 *    Replaying the recorded actions with carl_rollout from the same engine state gives the same bits.
 *  - summary mode (io == NULL): no per-step stores; summary_out (required) receives each lane's totals, and the
 *    engine state ends exactly as after a transitions-mode launch.  A summary (in either mode) needs
 *    CARL_FLAG_AUTORESET, else CARL_ERR_UNSUPPORTED: without auto-reset a finished lane reports done on every later
 *    step, and its one episode would be counted on each of them.
 * summary_out is optional in transitions mode (then both are written).  The batch is validated exactly as carl_rollout
 * validates it (same checks, same messages; e.g. a ctx_obs_feat[k] >= F is refused).  Bad arguments -- those batch
 * checks, widths over their limits, a head width that is not n_actions (discrete) or 1 (Box), a Brax family, a bad
 * lanes_per_set, a context row >= F -- return CARL_ERR_INVALID_ARGUMENT before anything is enqueued. */
int carl_rollout_policy(const carl_batch_t* batch, const carl_policy_t* policy_host, const carl_step_io_t* io,
                        int32_t n_steps, const carl_policy_summary_t* summary_out, void* stream);
int32_t carl_policy_lane_quantum(void); /* lanes_per_set must be a positive multiple of this (256) */
/* floats per weight set of the packed parameters (see above) for this policy's shape; -1 for an invalid shape */
int32_t carl_policy_set_floats(const carl_policy_t* policy_host);

/* one record per finished episode of carl_evaluate_policy; the [n_episodes][n_lanes] arrays are dense rows (pitch
 * n_lanes), row k holding each lane's k-th episode of the launch */
typedef struct carl_policy_episodes {
  int32_t* episodes;   /* [n_lanes] episodes finished in this launch, 0 .. n_episodes */
  int32_t* steps;      /* [n_lanes] steps this lane took in this launch */
  float* ret;          /* [n_episodes][n_lanes] fp32 return of each finished episode (ep_return, added in step order) */
  int32_t* length;     /* [n_episodes][n_lanes] its length (elapsed at its end) */
  int32_t* context_id; /* [n_episodes][n_lanes] the context-table index it ran in (ctx_idx before the step that ended it) */
  uint8_t* terminated; /* [n_episodes][n_lanes] 1: ended by termination (also when truncated at the same step); 0:
                          truncated only */
} carl_policy_episodes_t;

/* Episodes mode of the closed-loop rollout: every lane runs `policy_host` (as carl_rollout_policy) until it has
 * finished n_episodes episodes or taken max_steps steps in this launch, whichever comes first, and then stops stepping.
 * A lane stops right after the step that ends its n_episodes-th episode, with that step's auto-reset applied (its
 * stored state is the start of the next episode, as per-call stepping leaves it); a lane that reaches max_steps first
 * stops there, mid-episode.  Its state and bookkeeping (last_return / last_length / episodes_done, the finished-
 * episode log, the episode counter of the reset streams) advance exactly as for the steps it took, so a lane's
 * records are bit-identical to its first n_episodes episodes in a transitions-mode carl_rollout_policy from the same
 * engine state.  Episodes are counted from the current state: an episode already running when the launch starts is
 * reported with its full length and return.  A wavefront stops stepping once none of its lanes is live.
 * Every slot of `out` is written: a slot at or beyond episodes[lane] holds ret = NaN, length = 0, context_id = -1,
 * terminated = 0, so nothing needs clearing beforehand.  The batch and the policy are validated exactly as
 * carl_rollout_policy validates them; then out and its six arrays non-NULL, n_episodes >= 1, max_steps >= 0 and
 * n_episodes * n_lanes < 2^31.  Any failure returns CARL_ERR_INVALID_ARGUMENT before anything is enqueued; without
 * CARL_FLAG_AUTORESET the call returns CARL_ERR_UNSUPPORTED (as a summary does).  n_lanes == 0 enqueues nothing;
 * max_steps == 0 still fills every output.  No host synchronisation: stream-ordered and capturable. */
int carl_evaluate_policy(const carl_batch_t* batch, const carl_policy_t* policy_host, int32_t n_episodes,
                         int32_t max_steps, const carl_policy_episodes_t* out, void* stream);

/* ---- stochastic policies: sampled actions and their log-probabilities (additive; ABI version unchanged) ----
 * The same network as above; the action is drawn from the distribution the family implies instead of taken as its
 * mode:
 *  - discrete families: a categorical over the head's n_out logits y;
 *  - Box families: a diagonal Gaussian, mean y[0], state-independent log_std: one float per weight set (SB3's PPO
 *    default), a DEVICE array [n_sets] of its own.
 * Random words: each lane-step draws one Philox4x32-10 block w, key sample_seed (separate from the batch seed: new
 * actions leave the reset and context streams alone), counter (glane lo, glane hi, e, 0x80000000 | elapsed), with e the
 * index of the episode the step belongs to (episode counter - 1, the index the per-step noise of Acrobot uses) and
 * elapsed the lane's step count in that episode before the step.  A draw is therefore a pure function of (sample_seed,
 * lane, episode, step in episode): it does not depend on how a horizon is split into launches or on which mode runs the
 * step.  The high bit keeps the stream apart from the engine's own sub-streams (0, 1, 2 + elapsed), even when a caller
 * passes the batch seed as sample_seed.
 * Categorical:  u = (w.x >> 8) * 2^-24;  m = max_k y_k, e_k = exp(y_k - m), S = sum_k e_k, all in index order;
 *               t = u * S in fp32; the action is the first k with t < c_k, c_k the fp32 prefix sums of e in index
 *               order (the last index if there is none);  log_prob = (y_a - m) - log(S).
 * Gaussian:     u1 = ((w.x >> 8) + 1) * 2^-24 in (0, 1], u2 = (w.y >> 8) * 2^-24;
 *               z = sqrt(-2 ln u1) * cos(2 pi u2);  a = mu + exp(log_std) * z (one fma);
 *               log_prob = -z^2 / 2 - log_std - ln(2 pi) / 2.
 *               The recorded action is the raw a; the step clips it as it clips a deterministic Box policy's action
 *               (SB3 also stores the unclipped sample).
 * exp / log / sqrt / cos are the device's accurate fp32 functions (not the hardware approximations).
 * Padding lanes (the columns [n_lanes, pitch) a transitions launch writes) run as clones of lane n_lanes - 1 -- its
 * state, context, weight set, episode index and elapsed count -- but draw with their own glane = lane_offset + lane, so
 * their actions and log-probabilities are valid samples, not copies of lane n_lanes - 1's. */
typedef struct carl_policy_sampling {
  uint64_t seed;          /* sample_seed: the Philox key of the action draws */
  const float* log_std;   /* DEVICE [n_sets]: required for Box families, ignored for discrete ones */
  float* log_prob;        /* optional DEVICE [T][pitch] fp32, the layout of io->action: each action's log-probability;
                             transitions mode only */
} carl_policy_sampling_t;

/* carl_rollout_policy with sampled actions.  Everything carl_rollout_policy validates, in the same order and with the
 * same codes; then `sampling` non-NULL, a log_std for Box families, and no log_prob in summary mode (io == NULL): each
 * refused with CARL_ERR_INVALID_ARGUMENT before anything is enqueued.  Records, state and replay guarantees as
 * carl_rollout_policy's: replaying the recorded actions with carl_rollout gives the same bits; a summary launch leaves
 * the state a transitions launch leaves.  A categorical policy whose mode has probability 1 in fp32 (every other
 * exp(y_k - m) underflows to 0) takes exactly carl_rollout_policy's actions, with log_prob 0. */
int carl_rollout_policy_sampled(const carl_batch_t* batch, const carl_policy_t* policy_host,
                                const carl_policy_sampling_t* sampling, const carl_step_io_t* io, int32_t n_steps,
                                const carl_policy_summary_t* summary_out, void* stream);
/* carl_evaluate_policy with sampled actions: its validation, then `sampling` non-NULL, a log_std for Box families and
 * no log_prob (episodes mode stores no per-step output), each refused with CARL_ERR_INVALID_ARGUMENT.  A lane's records
 * are its first n_episodes episodes in a transitions-mode carl_rollout_policy_sampled with the same sample_seed. */
int carl_evaluate_policy_sampled(const carl_batch_t* batch, const carl_policy_t* policy_host,
                                 const carl_policy_sampling_t* sampling, int32_t n_episodes, int32_t max_steps,
                                 const carl_policy_episodes_t* out, void* stream);

/* ---- a critic in the closed-loop launch, and GAE on the device (additive; ABI version unchanged) ----
 * carl_rollout_policy_valued is the transitions-mode carl_rollout_policy (sampling == NULL) or
 * carl_rollout_policy_sampled (sampling != NULL) with a second network, the critic, evaluated on the inputs the actor
 * sees: everything those calls write, bit for bit, plus the columns of carl_policy_value_t.
 * The critic is a carl_policy_t with n_out == 1, hidden widths and an activation of its own, and the actor's n_in, n_ctx,
 * ctx_rows, n_sets and lanes_per_set; `head` is not read.  It reads the actor's transformed inputs x (after the actor's
 * shift / scale / clip): the shift / scale / clip section of its own packed block is NOT READ, so a block whose section
 * equals the actor's makes the documented forward pass of that block the exact reference.  V = y[0], the same explicit
 * fma order, bias first, the same tanh.
 *   value      [n_steps][pitch] fp32, the layout of io->action: V(x_t), x_t the input step t's action was chosen from
 *   last_value [n_lanes] fp32: V of each lane's input after the launch's last step (its current context, re-read if
 *              the last step moved the lane, and its current observation)
 *   boot_value [n_steps][pitch] fp32, NULL: not wanted.  Needs CARL_FLAG_AUTORESET (CARL_ERR_UNSUPPORTED without).  On a
 *              step that ends a lane's episode by truncation only (truncated && !terminated):
 *              V([context values of the context the episode ran in, terminal observation]); +0.0f everywhere else
 *              (SB3's timeout bootstrap: reward + gamma * boot_value).
 * Validation: carl_rollout_policy's, in its order; then io != NULL (transitions mode only: CARL_ERR_INVALID_ARGUMENT),
 * the sampling checks of carl_rollout_policy_sampled when sampling != NULL, plus sampling->log_prob != NULL (a sampled
 * valued launch always stores the log-probabilities); then the critic and `out`.  value / boot_value on 16-byte
 * boundaries.  n_lanes == 0 or n_steps == 0 enqueues nothing and writes nothing.  summary_out as carl_rollout_policy's
 * transitions mode.  Padding columns [n_lanes, pitch) of value / boot_value receive the padding lanes' values. */
typedef struct carl_policy_value {
  float* value;      /* DEVICE [n_steps][pitch] */
  float* last_value; /* DEVICE [n_lanes] */
  float* boot_value; /* DEVICE [n_steps][pitch], nullable */
} carl_policy_value_t;

int carl_rollout_policy_valued(const carl_batch_t* batch, const carl_policy_t* policy_host,
                               const carl_policy_t* critic_host, const carl_policy_sampling_t* sampling,
                               const carl_step_io_t* io, int32_t n_steps, const carl_policy_summary_t* summary_out,
                               const carl_policy_value_t* out, void* stream);

/* Generalised advantage estimation over [n_steps][pitch] rows (row_pitch lanes per row, 0 = n_lanes; no alignment
 * rule), one launch, stream-ordered.  With gl = fp32(gamma) * fp32(lambda) (one fp32 rounding), A = 0 and, for
 * t = n_steps - 1 .. 0:
 *   done  = terminated[t] | truncated[t]
 *   vn    = done ? ((truncated[t] && !terminated[t] && boot_value) ? boot_value[t] : 0)
 *                : (t == n_steps - 1 ? last_value : value[t + 1])
 *   delta = fma(gamma, vn, reward[t]) - value[t]
 *   A     = fma(gl, done ? 0 : A, delta);   advantage[t] = A;   ret[t] = A + value[t]
 * every operation in fp32, selects not mask products (a masked-out NaN or infinity changes nothing).  This is SB3's
 * RolloutBuffer.compute_returns_and_advantage with the timeout bootstrap folded in.  Only columns [0, n_lanes) of rows
 * [0, n_steps) of advantage / ret are written.  All pointers but boot_value are required; n_lanes, n_steps >= 0;
 * row_pitch 0 or >= n_lanes: else CARL_ERR_INVALID_ARGUMENT before anything is enqueued. */
typedef struct carl_gae {
  int32_t n_lanes;
  int32_t n_steps;
  int32_t row_pitch;
  float gamma;
  float lambda;
  int32_t reserved;
  const float* reward;       /* DEVICE [n_steps][pitch] */
  const float* value;        /* DEVICE [n_steps][pitch] */
  const float* boot_value;   /* DEVICE [n_steps][pitch], nullable */
  const float* last_value;   /* DEVICE [n_lanes] */
  const uint8_t* terminated; /* DEVICE [n_steps][pitch] */
  const uint8_t* truncated;  /* DEVICE [n_steps][pitch] */
  float* advantage;          /* DEVICE [n_steps][pitch] */
  float* ret;                /* DEVICE [n_steps][pitch] */
} carl_gae_t;

int carl_gae(const carl_gae_t* gae_host, void* stream);

/* ---- evolution strategies on the device: perturb and gradient (additive; ABI version unchanged) ----
 * The population side of the closed-loop rollout (ES, Salimans et al. 2017; ARS, Mania et al. 2018): a centre parameter
 * vector -- one packed weight set, the layout above -- is perturbed into n_pairs antithetic pairs of weight sets, written
 * straight into the [n_sets][carl_policy_set_floats()] block carl_policy_t::params points at (n_sets = 2 * n_pairs: set
 * 2i is centre + sigma * z_i, set 2i + 1 is centre - sigma * z_i), and after the sets have been evaluated the gradient
 * estimate sum_i weight[i] * z_i is rebuilt by REGENERATING z from its counter: the noise is never stored.  No reference
 * counterpart (the reference has no population path: its caller builds one env and one agent, carl/envs/carl_env.py).
 *
 * Noise rule.  Parameter j of pair i takes its standard normal z_ij from the Philox4x32-10 block w with key `seed` and
 * counter (j >> 1, i, generation, 0x40000000): even j uses (a, b) = (w.x, w.y), odd j uses (w.z, w.w), and
 *   u1 = ((a >> 8) + 1) * 2^-24 in (0, 1],  u2 = (b >> 8) * 2^-24,  z = sqrtf(-2 logf(u1)) * cospif(2 u2)
 * -- carl_policy_sampling_t's Gaussian rule: the device's accurate fp32 functions, every product rounded on its own
 * (no fma).  z is a pure function of (seed, generation, i, j): it does not depend on the grid, on how a population is
 * sharded or on the number of launches.  The last counter word keeps the stream apart from the engine's sub-streams
 * (0, 1, 2 + elapsed) and from the action draws (0x80000000 | elapsed) even under a shared seed.  |z| <= 5.8
 * (u1 >= 2^-24).
 *
 * carl_es_perturb: for j < n_noisy
 *   params[2i][j] = center[j] + d,  params[2i + 1][j] = center[j] - d,  d = sigma * z_ij
 * in fp32 with two roundings each (the product, then the sum; no fma), so NumPy float32 reproduces both from z exactly;
 * for j in [n_noisy, set_floats) (the shift | scale | clip section and the padding) both sets receive center[j]'s bits
 * unchanged (a NaN or infinite clip included).  noise[i][j] = z_ij for j < n_noisy when `noise` is not NULL (dense rows
 * of n_noisy floats; for tests and diagnostics -- carl_es_gradient does not read it).  Every element of params is
 * written and nothing beyond it.
 *
 * carl_es_gradient: grad[j] = sum_i weight[i] * z_ij for j < n_noisy, in this order: the pairs are cut into slices of
 * carl_es_slice_pairs() consecutive pairs (the last one may be shorter); inside a slice p = +0.0f, then
 * p = p + weight[i] * z_ij for its pairs in order (fp32, the product and the sum rounded separately, no fma); then
 * g = +0.0f, g = g + p_s over the slices in order.  The result is a pure function of the inputs whatever the grid (no
 * floating-point atomics), and a host that holds the noise carl_es_perturb wrote reproduces it bit for bit.  Only
 * grad[0 .. n_noisy) is written.  No scratch buffer is needed.
 *
 * Validation, before anything is enqueued, CARL_ERR_INVALID_ARGUMENT each: a NULL struct, center, params, weight or
 * grad; n_pairs < 1; set_floats <= 0 or not a multiple of 4; n_noisy outside 1 .. set_floats; sigma not finite or not
 * positive; 2 * n_pairs * set_floats >= 2^31; params off a 16-byte boundary.  Both calls are stream-ordered and
 * capturable; the library allocates nothing. */
typedef struct carl_es {
  uint64_t seed;        /* Philox key of the noise */
  uint32_t generation;  /* counter word */
  int32_t n_pairs;      /* >= 1; the population is 2 * n_pairs weight sets */
  int32_t set_floats;   /* carl_policy_set_floats() of the shape: > 0, a multiple of 4 */
  int32_t n_noisy;      /* leading floats of a set that receive noise (every W and b); 1 .. set_floats */
  float sigma;          /* finite, > 0 */
  int32_t reserved;
} carl_es_t;

int carl_es_perturb(const carl_es_t* es_host, const float* center /* DEVICE [set_floats] */,
                    float* params /* DEVICE [2 * n_pairs][set_floats], 16-byte aligned */,
                    float* noise /* DEVICE [n_pairs][n_noisy], nullable */, void* stream);
int carl_es_gradient(const carl_es_t* es_host, const float* weight /* DEVICE [n_pairs] */,
                     float* grad /* DEVICE [n_noisy] */, void* stream);
int32_t carl_es_slice_pairs(void); /* pairs of one summation slice of carl_es_gradient (16) */

/* ---- input statistics inside the episodes launch, and their running merge (additive; ABI version unchanged) ----
 * What produces the shift and scale of the input transform above (SB3's VecNormalize; ARS V2, Mania et al. 2018: the
 * mean and variance of every state every member of a population visited, applied to the next generation's inputs).
 * In episodes mode no per-step output exists, so the sums are gathered inside the launch.  No reference counterpart.
 *
 * carl_evaluate_policy_stats is carl_evaluate_policy (sampling == NULL) or carl_evaluate_policy_sampled (sampling !=
 * NULL): the records, the engine state and the bookkeeping are theirs bit for bit.  In addition, for every LIVE
 * lane-step (the steps `episodes_out.steps` counts: a frozen lane and a padding lane add nothing) and every policy
 * input i < n_in, in FlattenObservation order (the n_ctx context inputs, then the observation):
 *     d_i = fp32(x_i - shift_i)       x_i the raw input, shift_i that of the lane's weight set: the first operation
 *                                     of the input transform, before the scale and the clip
 *     S1_i += d_i,  S2_i += d_i * d_i
 * (the shifted-data algorithm: once the shift tracks the mean, the variance suffers no cancellation).  Workgroup w --
 * lanes [256 w, 256 w + 256) -- writes its own sums to partial[w][0][i] (S1) and partial[w][1][i] (S2), float64,
 * partial being [n_workgroups][2][CARL_POLICY_MAX_IN]; entries i >= n_in receive +0.0.  Every workgroup writes its slab
 * in full, so nothing needs clearing, and max_steps == 0 writes zeros.  The number of lane-steps is not stored again:
 * it is the sum of episodes_out.steps.
 * Accuracy: for an observation input a lane adds in fp32 (S2 by one fma per step) over at most one chunk of 8 steps (4
 * for Acrobot); the chunk partials are widened to float64, added across the wavefront in a fixed order and accumulated in
 * float64 from there on.  So |S1_i - exact| <= 10 * 2^-24 * sum |d_i|, likewise S2_i against sum d_i^2.  A context
 * input, constant while the lane stays in one context, enters as c * d_i and c * d_i * d_i formed in float64, c the
 * lane's steps in that context since the last chunk boundary (<= 8): both products are exact, so a context input's
 * sums carry float64 rounding only.  No floating-point atomics: the slabs are a fixed function of the launch's inputs,
 * the same bits whatever the grid's schedule.
 * Validation: everything carl_evaluate_policy (and, with `sampling`, carl_evaluate_policy_sampled) validates, in the
 * same order with the same codes; then `stats` and stats->partial non-NULL, partial on a 16-byte boundary and
 * partial_capacity >= carl_policy_stats_workgroups(n_lanes): CARL_ERR_INVALID_ARGUMENT before anything is enqueued. */
typedef struct carl_policy_stats {
  double* partial;          /* DEVICE [partial_capacity][2][CARL_POLICY_MAX_IN] float64 */
  int32_t partial_capacity; /* workgroup slabs `partial` holds */
} carl_policy_stats_t;

int32_t carl_policy_stats_workgroups(int32_t n_lanes); /* slabs a launch over n_lanes writes (0 for n_lanes <= 0) */
int carl_evaluate_policy_stats(const carl_batch_t* batch, const carl_policy_t* policy_host,
                               const carl_policy_sampling_t* sampling /* NULL: deterministic */, int32_t n_episodes,
                               int32_t max_steps, const carl_policy_episodes_t* episodes_out,
                               const carl_policy_stats_t* stats, void* stream);

/* The running statistics of a policy's inputs, on the device: count of lane-steps, mean[n_in], M2[n_in] (the sum of
 * squared deviations from the mean).  All zero: nothing seen yet. */
typedef struct carl_policy_running_stats {
  int64_t* count; /* DEVICE [1] */
  double* mean;   /* DEVICE [CARL_POLICY_MAX_IN] ([n_in] used) */
  double* m2;     /* DEVICE [CARL_POLICY_MAX_IN] ([n_in] used) */
} carl_policy_running_stats_t;

/* Merge the slabs of one carl_evaluate_policy_stats launch into `running` and, when params_out is not NULL, write the
 * transform the new statistics imply into n_write consecutive packed weight sets at params_out.  One small workgroup,
 * every operation in float64, each rounded on its own (no fma):
 *   n_b  = sum of steps[0 .. n_lanes) (int64);  n_b == 0: nothing is read further and nothing is written.
 *   S1_i = 0.0; S1_i += partial[w][0][i] for w = 0 .. n_workgroups - 1 in order;  S2_i likewise from partial[w][1][i]
 *   shift_i = policy_host->params[transform offset + i] of weight set 0 -- the shift the launch ran under; every
 *             weight set of that launch must have carried the same shift
 *   mean_b = (double)shift_i + S1_i / n_b;   M2_b = max(S2_i - S1_i * S1_i / n_b, 0)
 *   count == 0:  mean_i = mean_b, M2_i = M2_b
 *   else (Chan et al.):  n = count + n_b;  delta = mean_b - mean_i;
 *                mean_i = mean_i + delta * (n_b / n);   M2_i = (M2_i + M2_b) + delta * delta * (count * n_b / n)
 *   count = count + n_b
 *   var = M2_i / count;   floor = max(min_std^2, (2^-18 * |mean_i|)^2)
 *   scale_i = var <= floor ? 0 : 1 / sqrt(var + eps)
 *   block k < n_write: params_out[k * set_floats + transform offset + i] = fp32(mean_i),
 *                      params_out[k * set_floats + transform offset + n_in + i] = fp32(scale_i)
 * with transform offset = the floats of every W and b of the shape (the packing rule above) and set_floats =
 * carl_policy_set_floats().  Weights, biases, clip and the padding keep their bits.  An input whose variance is at
 * or below the floor counts as CONSTANT and gets scale 0: the policy ignores it (ARS's convention).  The relative
 * term is a derived bound, not a measurement: a constant fp32 input summed over a chunk of at most 8 steps carries at
 * most about 8 * 2^-24 = 2^-21 of relative rounding, and 2^-18 leaves a factor of 8 over that.  (That is a bound on
 * the SUMS.  The variance M2 / count = S2 / n - (S1 / n)^2 loses them to cancellation: a relative error r of S2 is a
 * variance of r * mean^2, a deviation of sqrt(r) * |mean| -- 2^-12 |mean| for one fp32 rounding of d * d.  The floor
 * therefore tells a constant input only because the context inputs' sums are formed exactly, see above: r is then a
 * few float64 roundings per addition, far below 2^-36.  A constant OBSERVATION entry summed in fp32 is not detected.)
 * params_out may be policy_host->params itself.  Validation, CARL_ERR_INVALID_ARGUMENT before anything is enqueued: a
 * NULL policy_host, an invalid shape or NULL params; stats / stats->partial NULL; n_workgroups outside
 * 0 .. partial_capacity; n_lanes < 0, or steps NULL with n_lanes > 0; `running` or one of its pointers NULL; eps or
 * min_std negative or not finite; n_write < 0.
 * Both calls are stream-ordered and capturable, never synchronise with the host and allocate nothing. */
int carl_policy_stats_merge(const carl_policy_t* policy_host, const carl_policy_stats_t* stats, int32_t n_workgroups,
                            const int32_t* steps /* DEVICE [n_lanes] */, int32_t n_lanes,
                            const carl_policy_running_stats_t* running, double eps, double min_std,
                            float* params_out /* DEVICE [n_write][set_floats], nullable */, int32_t n_write,
                            void* stream);

/* ---- the PPO update on the device: per-step context ids and minibatch gradients (additive; ABI version unchanged) ----
 * carl_rollout_policy_valued + carl_gae leave a complete PPO rollout buffer on the device (actions, log-probabilities,
 * values, advantages, returns).  The two calls below turn it into the clipped-surrogate loss and its gradients (SB3's
 * PPO; the reference's one training example, examples/carl_with_sb3.py, trains PPO on FlattenObservation(env)) without
 * carrying the buffer into an autograd framework.  Classic-control families only.  No existing kernel is touched.
 *
 * carl_policy_context_trace: the context each step of a launch ran in.  A launch stores each step's observation but not
 * the context half of the policy's input, and a moving selector changes a lane's context at every reset.  From each
 * lane's ctx_idx / episode BEFORE the traced launch (copies the caller took: ctx_idx0 [n_lanes] int32, episode0
 * [n_lanes] uint32) and that launch's terminated / truncated rows the walk is replayed, one thread per lane:
 *   c = ctx_idx0[lane], e = episode0[lane];  for t = 0 .. n_steps - 1:
 *     context_id[t][lane] = c                                      (the context step t's action was chosen in)
 *     with CARL_FLAG_AUTORESET, if terminated[t][lane] | truncated[t][lane]:
 *       c = the selector's next context (the engine's own rule, called with (c, lane_offset + lane, e));  e += 1
 * -- the order of a lane's reset.  Without auto-reset the context never moves.  `batch` is read for family, n_lanes,
 * n_contexts, selector, selector_stride, flags, seed and lane_offset only (no pointer of it is read).  Rows are
 * row_pitch lanes long (0 = n_lanes); only columns [0, n_lanes) of context_id are written.  Validation, each
 * CARL_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL batch or pointer, a Brax family, n_lanes or n_steps < 0,
 * n_contexts < 1, an unknown selector, a pitch that is neither 0 nor >= n_lanes.  n_lanes == 0 or n_steps == 0 enqueues
 * nothing. */
int carl_policy_context_trace(const carl_batch_t* batch, const int32_t* ctx_idx0 /* DEVICE [n_lanes] */,
                              const uint32_t* episode0 /* DEVICE [n_lanes] */,
                              const uint8_t* terminated /* DEVICE [n_steps][pitch] */,
                              const uint8_t* truncated /* DEVICE [n_steps][pitch] */, int32_t n_steps, int32_t row_pitch,
                              int32_t* context_id /* DEVICE [n_steps][pitch] */, void* stream);

/* carl_ppo_grad: loss and gradients of one minibatch of a rollout buffer.  All pointers of carl_ppo_batch_t are DEVICE
 * pointers; the [n_steps][pitch] columns use the layout carl_rollout_policy writes (pitch = row_pitch, 0 = n_lanes).
 * Sample (t, lane) has the flat index t * pitch + lane.  Its input is exactly what the rollout's actor saw:
 *   x_k = ctx_table[ctx_rows[k]][context_id[t][lane]] for k < n_ctx, then obs0[lane] (t == 0) or obs[t - 1][lane],
 * transformed by the actor's shift / scale / clip; the critic reads the same transformed x (its own section is not
 * read), as in carl_rollout_policy_valued.  Forward arithmetic is the rollout's (explicit fma in input order, bias
 * first, the same tanh, expf / logf for the heads).  With lp, V and the entropy H under the given parameters,
 * A' = adv_norm ? (A - adv_norm[0]) * adv_norm[1] : A,  r = exp(lp - log_prob) and c = clip_range:
 *   pl = -mean(min(r A', clamp(r, 1 - c, 1 + c) A'))    vl = mean((ret - V)^2)    el = -mean(H)
 *   L  = pl + ent_coef el + vf_coef vl
 * Categorical head: lp = (y_a - m) - log S, H = -sum_k p_k log p_k.  Gaussian head (log_std [1] on the device):
 * z = (a - mu) exp(-log_std), lp = -z^2 / 2 - log_std - ln(2 pi) / 2, H = 1/2 + ln(2 pi) / 2 + log_std.  The surrogate's
 * gradient flows through r A' unless the clip is active (A' > 0 && r > 1 + c, or A' < 0 && r < 1 - c).
 * Outputs (carl_ppo_out_t):
 *   grad_actor  [carl_policy_set_floats(actor)]: dL/dparams in the packed layout; the shift / scale / clip entries and
 *               the padding receive +0.0 (an optimiser stepping the whole packed block leaves them untouched)
 *   grad_critic [carl_policy_set_floats(critic)]: likewise
 *   grad_log_std [1]: Box families only (ignored, may be NULL, for discrete ones)
 *   stats [6]: pl, vl, mean entropy, approx_kl = mean((r - 1) - log r), clip fraction = mean(|r - 1| > c), n_samples
 *   new_log_prob / new_value [n_samples], nullable: lp and V of each sample, in idx order
 * How it runs: a launch per network (the actor, then the critic: both at width 64 with a tile's activations do not fit
 * the LDS of a compute unit) of carl_ppo_grad_workgroups(n_samples) persistent workgroups that loop over tiles of
 * carl_ppo_tile() samples with a grid stride.  The weights are staged in LDS once per workgroup; one thread runs one
 * sample's forward and backward pass in registers; the tile's activations and deltas go to LDS, and every thread adds
 * dW[i][j] = sum_s delta[s][i] h[s][j] for its own fixed (i, j) entries, walking the tile's samples in index order
 * (blocks of 16 samples, block sums added in order).  Each workgroup writes one partial slab to `workspace`; a last
 * small kernel adds the slabs in workgroup order in float64, multiplies by 1 / n_samples and rounds once.  No
 * floating-point atomics: the same call twice gives the same bits.
 * Preconditions the host cannot check: idx entries are distinct, each t * pitch + lane with lane < n_lanes (an entry
 * outside the buffer is skipped: it contributes zero); actions of a discrete family lie in [0, n_actions).
 * new_log_prob[m] / new_value[m] of a skipped entry are not written.
 * Validation, each CARL_ERR_INVALID_ARGUMENT with a message before anything is enqueued: a NULL struct or required
 * pointer; a Brax family; n_lanes < 1, n_steps < 1; a pitch that is neither 0 nor >= n_lanes; the networks as
 * carl_rollout_policy_valued validates them (shape limits, the head against the family, n_in == n_ctx + obs_dim, context
 * rows, activation, params; the critic's inputs against the actor's) and n_sets == 1 (several weight sets are
 * evolution-strategies territory); obs_dim against the family; the action dtype against the head (CARL_ACTION_I32 /
 * CARL_ACTION_F32); n_contexts < 1 or ctx_stride < n_contexts; n_samples < 1, n_samples > n_steps * n_lanes, or idx NULL
 * with n_samples != n_steps * n_lanes; clip_range / vf_coef / ent_coef negative or not finite; a Box family without
 * log_std or grad_log_std; workspace NULL, off a 16-byte boundary or smaller than carl_ppo_workspace_floats().
 * Stream-ordered and capturable; never synchronises with the host; allocates nothing. */
typedef struct carl_ppo_batch {
  int32_t family;          /* carl_family_t of the batch that produced the buffer */
  int32_t n_lanes;
  int32_t n_steps;
  int32_t row_pitch;       /* lanes per row of every [n_steps][pitch] column; 0 = n_lanes */
  int32_t obs_dim;         /* D */
  int32_t n_contexts;      /* valid columns of ctx_table */
  int32_t ctx_stride;      /* elements between its feature rows */
  int32_t action_dtype;    /* CARL_ACTION_I32 (discrete families) / CARL_ACTION_F32 (Box) */
  int32_t n_samples;       /* M */
  int32_t reserved;
  float clip_range;        /* c >= 0 */
  float vf_coef;           /* >= 0 */
  float ent_coef;          /* >= 0 */
  int32_t reserved2;
  const float* obs0;       /* [n_lanes][D]: the observation step 0's action was chosen from */
  const float* obs;        /* [n_steps][pitch][D]: the launch's observation rows */
  const int32_t* context_id; /* [n_steps][pitch]: carl_policy_context_trace's output */
  const float* ctx_table;  /* [F][ctx_stride] */
  const void* action;      /* [n_steps][pitch] int32 or float32 */
  const float* log_prob;   /* [n_steps][pitch] */
  const float* advantage;  /* [n_steps][pitch] */
  const float* ret;        /* [n_steps][pitch] */
  const int32_t* idx;      /* [n_samples] flat sample indices, or NULL: every (t, lane), t-major */
  const float* adv_norm;   /* [2] (mean, 1 / (std + eps)), or NULL: advantages as they are */
} carl_ppo_batch_t;

typedef struct carl_ppo_out {
  float* grad_actor;       /* [carl_policy_set_floats(actor)] */
  float* grad_critic;      /* [carl_policy_set_floats(critic)] */
  float* grad_log_std;     /* [1], Box families */
  float* stats;            /* [6] */
  float* new_log_prob;     /* [n_samples], nullable */
  float* new_value;        /* [n_samples], nullable */
  float* workspace;        /* [workspace_floats], 16-byte aligned */
  int64_t workspace_floats; /* >= carl_ppo_workspace_floats() */
} carl_ppo_out_t;

int32_t carl_ppo_tile(void);                           /* samples of one tile (256) */
int32_t carl_ppo_grad_workgroups(int32_t n_samples);   /* workgroups of a launch: min(tiles, 256); 0 for n_samples < 1 */
/* floats of the workspace for these shapes and n_samples; -1 for an invalid shape or n_samples < 1 */
int64_t carl_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples);
int carl_ppo_grad(const carl_ppo_batch_t* ppo_host, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                  const float* log_std /* DEVICE [1], Box families */, const carl_ppo_out_t* out, void* stream);

/* ---- PPO's running normalisation: input sums over a rollout buffer, return statistics (additive; ABI version unchanged) ----
 * What SB3's VecNormalize and Brax's PPO do around the update: the policy's inputs are shifted and scaled by running
 * statistics, the rewards divided by the running deviation of the discounted return.  The input transform and its
 * running merge exist (the shift | scale | clip section; carl_policy_stats_merge); the calls below are the source of sums
 * for a PPO collection, and everything for rewards.  No existing kernel is touched; no reference counterpart.
 *
 * carl_ppo_input_stats: for EVERY sample (t, lane), t < n_steps, lane < n_lanes, of a carl_ppo_batch_t and every policy
 * input i < n_in, the input is formed exactly as carl_ppo_grad's gather forms it --
 *   x_i = ctx_table[ctx_rows[i]][clamp(context_id[t][lane], 0, n_contexts - 1)]   for i < n_ctx,
 *   else entry i - n_ctx of obs0[lane] (t == 0) or of obs[t - 1][lane]
 * -- and accumulated by carl_evaluate_policy_stats's definition,
 *   d_i = fp32(x_i - shift_i)   shift_i that of weight set 0;      S1_i += d_i,  S2_i += d_i * d_i
 * with EVERY addition and the product in float64 from the first sample on (the product of two widened floats is exact).
 * So |S_i - exact| <= n * 2^-53 * sum |terms| for n samples, for every input alike, and a constant observation entry is
 * recognised by the merge's constant rule, which the fp32 chunk sums of the episodes launch do not give.
 * Row n_steps - 1 of obs is deliberately not counted: it is the next collection's obs0, so over a run every input the
 * policy acts on is counted once.  Of the batch idx must be NULL; adv_norm, action, log_prob, advantage, ret, n_samples,
 * action_dtype and the three coefficients are not read.  Rows are row_pitch lanes long (0 = n_lanes).
 * Output: partial[slab][2][CARL_POLICY_MAX_IN] float64, slab < carl_ppo_input_stats_slabs(n_lanes, n_steps), every slab
 * written in full, entries i >= n_in +0.0 -- what carl_policy_stats_merge reads, with `steps` an int32 [n_lanes] array
 * filled with n_steps.
 * How it runs: min(ceil(n_steps * n_lanes / 256), 256) persistent workgroups of 256 threads.  A thread owns one input
 * slot of one sample of each pass of floor(256 / n_in) consecutive samples (t-major), so it holds one (S1, S2) pair
 * and consecutive threads read consecutive floats of consecutive observation rows; the passes go round the grid; a
 * thread chains its samples in order, the workgroup's pairs of a slot are added from LDS in thread order, one slab
 * per workgroup.  No floating-point atomics: two calls give the same bits, and the slabs are a fixed function of the
 * buffer and the launch shape.  One read of the observation rows and the id rows.
 * Validation, each CARL_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL ppo or policy; a Brax family; obs_dim
 * against the family; a policy shape outside the limits or NULL params; n_ctx, the context rows, n_in != n_ctx + obs_dim;
 * idx != NULL; n_steps < 1 or n_lanes < 0; a pitch that is neither 0 nor >= n_lanes; n_steps * pitch >= 2^31;
 * n_contexts < 1 or ctx_stride < n_contexts; obs0, obs, context_id or ctx_table NULL; stats / stats->partial NULL,
 * partial off a 16-byte boundary, partial_capacity below the slab count.  n_lanes == 0 enqueues nothing.
 * Stream-ordered and capturable; never synchronises with the host; allocates nothing. */
int32_t carl_ppo_input_stats_slabs(int32_t n_lanes, int32_t n_steps); /* host only; 0 for n_lanes < 1 or n_steps < 1 */
int carl_ppo_input_stats(const carl_ppo_batch_t* ppo_host, const carl_policy_t* policy_host,
                         const carl_policy_stats_t* stats, void* stream);

/* carl_ppo_return_stats: the discounted return of every lane and its sums, for reward scaling.  One thread per lane walks
 * its column forward from the persistent ret[lane] (the caller zeroes it once, before the first collection):
 *   for t = 0 .. n_steps - 1:
 *     ret = fp32(fp32(gamma * ret) + reward[t][lane])          (no fma: a NumPy float32 restatement gives the same bits)
 *     ret_rows[t][lane] = ret  (when ret_rows != NULL);    S1 += ret,  S2 += ret * ret  (float64, the product exact)
 *     ret = 0  where terminated[t][lane] | truncated[t][lane]                                (VecNormalize's order)
 * and writes ret[lane] back.  Workgroup w -- lanes [256 w, 256 w + 256) -- adds its lanes' sums in a fixed order and
 * writes partial[w][0] = S1, partial[w][1] = S2 (float64); no atomics.  Rows are row_pitch lanes long (0 = n_lanes).
 * Validation, each CARL_ERR_INVALID_ARGUMENT before anything is enqueued: a NULL struct; n_steps < 1 or n_lanes < 0; a pitch
 * that is neither 0 nor >= n_lanes; gamma negative or not finite; reward, terminated, truncated or ret NULL; partial NULL
 * or off a 16-byte boundary; partial_capacity < carl_ppo_return_stats_slabs(n_lanes).  n_lanes == 0 enqueues nothing. */
typedef struct carl_ppo_return_stats {
  int32_t n_lanes;
  int32_t n_steps;
  int32_t row_pitch;         /* lanes per row of the [n_steps][pitch] columns; 0 = n_lanes */
  float gamma;
  const float* reward;       /* DEVICE [n_steps][pitch] */
  const uint8_t* terminated; /* DEVICE [n_steps][pitch] */
  const uint8_t* truncated;  /* DEVICE [n_steps][pitch] */
  float* ret;                /* DEVICE [n_lanes]: read, advanced, written back */
  float* ret_rows;           /* DEVICE [n_steps][pitch], nullable: the return after each step's reward */
  double* partial;           /* DEVICE [partial_capacity][2] float64 */
  int32_t partial_capacity;
  int32_t reserved;
} carl_ppo_return_stats_t;

int32_t carl_ppo_return_stats_slabs(int32_t n_lanes); /* ceil(n_lanes / 256); 0 for n_lanes < 1 */
int carl_ppo_return_stats(const carl_ppo_return_stats_t* rs_host, void* stream);

/* carl_ppo_return_merge: the slabs of one carl_ppo_return_stats launch into the running (count, mean[0], m2[0]) and the
 * reward scale.  One thread, every operation in float64, each rounded on its own (no fma) -- carl_policy_stats_merge's
 * rule for one entry, without a shift and without the constant rule:
 *   S1 = 0.0; S1 += partial[w][0] for w = 0 .. n_slabs - 1 in order;  S2 likewise from partial[w][1]
 *   mean_b = S1 / n_b;   M2_b = max(S2 - S1 * S1 / n_b, 0)                  n_b = n_steps * n_lanes, given by the host
 *   count == 0:  mean = mean_b, M2 = M2_b
 *   else:        n = count + n_b;  delta = mean_b - mean;
 *                mean = mean + delta * (n_b / n);   M2 = (M2 + M2_b) + delta * delta * (count * n_b / n)
 *   count = count + n_b;    scale[0] = fp32(1 / sqrt(M2 / count + eps))
 * Validation, each CARL_ERR_INVALID_ARGUMENT before anything is enqueued: partial NULL or off a 16-byte boundary; n_slabs
 * < 0; n_b < 0; `running` or one of its pointers NULL; eps negative or not finite; scale NULL.  n_b == 0 enqueues nothing.
 * Both calls are stream-ordered and capturable, never synchronise with the host and allocate nothing. */
int carl_ppo_return_merge(const double* partial /* DEVICE [n_slabs][2] */, int32_t n_slabs, int64_t n_b,
                          const carl_policy_running_stats_t* running, double eps, float* scale /* DEVICE [1] */,
                          void* stream);

/* ---- PPO's minibatch step: advantage statistics of an epoch, global-norm clip and Adam (additive; ABI version unchanged) ----
 * What stands between two carl_ppo_grad calls of a PPO update: each minibatch's advantage mean and scale, the global-norm
 * clip of the gradients and Adam's step.  With the two calls below a minibatch is carl_ppo_grad's three launches plus one,
 * and a caller of this header trains without another library.  Neither call knows a family: they serve the classic and
 * the Brax families alike.  No existing kernel is touched; no reference counterpart.
 *
 * carl_ppo_adv_stats: row k of adv_norm is what carl_ppo_batch_t.adv_norm takes for minibatch k of an epoch whose
 * permutation idx [n_total] is the concatenation of its minibatches of batch_size samples in order (the last one may be
 * shorter).  With the n samples a_i = advantage[idx[k * batch_size + i]] of minibatch k, everything in float64, every
 * operation rounded on its own (no fma):
 *   c = a_0;   d_i = (double)a_i - (double)c;   S1 = sum d_i,  S2 = sum d_i * d_i   in a fixed order
 *   mean = c + S1 / n;    var = max(0, (S2 - S1 * S1 / n) / (n - 1))                 (unbiased, as torch's std())
 *   adv_norm[k] = (fp32(mean), fp32(1 / (sqrt(var) + eps)))
 * n == 1 writes (+0.0, 1.0), the identity (what adv_norm == NULL does).  The shift by the first sample makes a constant
 * column give var == 0 exactly, so its scale is fp32(1 / eps).  An index outside [0, storage_floats) is not read and counts
 * as d = 0 (where it is the minibatch's first, c = 0).  |S - exact| <= n * 2^-53 * sum |terms|.
 * How it runs: one workgroup of 256 threads per minibatch.  Thread t chains samples t, t + 256, ... in that order, 8
 * gathers issued ahead of the dependent adds; a wavefront adds its 64 values by a shuffle tree, thread 0 the four
 * wavefronts' sums in order.  No atomics: two calls give the same bits.
 * Validation, each CARL_ERR_INVALID_ARGUMENT with a message before anything is enqueued: a NULL struct; advantage, idx or
 * adv_norm NULL; n_total < 1 or batch_size < 1; storage_floats < 1; eps negative or not finite.
 * Stream-ordered and capturable; never synchronises with the host; allocates nothing. */
typedef struct carl_ppo_adv_stats {
  const float* advantage;  /* DEVICE: the [n_steps][pitch] storage carl_ppo_grad reads */
  const int32_t* idx;      /* DEVICE [n_total]: flat indices into it, an epoch's minibatches in order */
  float* adv_norm;         /* DEVICE [carl_ppo_adv_stats_rows(n_total, batch_size)][2] */
  int64_t storage_floats;  /* floats of the storage an index may address */
  int32_t n_total;
  int32_t batch_size;
  double eps;
} carl_ppo_adv_stats_t;

int32_t carl_ppo_adv_stats_rows(int32_t n_total, int32_t batch_size); /* ceil(n_total / batch_size); 0 where either is < 1 */
int carl_ppo_adv_stats(const carl_ppo_adv_stats_t* as_host, void* stream);

/* carl_adam_step: the global-norm clip and one Adam step (torch.optim.Adam without weight decay or amsgrad) over
 * n_tensors float32 tensors in one launch.  Arithmetic is float64, every operation rounded on its own (no fma), each stored
 * value rounded to float32 once:
 *   norm = sqrt(sum over all tensors of (double)g * (double)g)   in a fixed order
 *   coef = min(1, max_grad_norm / (norm + 1e-6))                 (max_grad_norm = +inf: 1, no clip)
 *   step[0] += 1;   beta_pow[j] = beta_pow[j] * beta_j;   bc_j = 1 - beta_pow[j]
 *   per element:  gd = (double)g * coef
 *                 m = fp32(beta1 * m + (1 - beta1) * gd)
 *                 v = fp32(beta2 * v + ((1 - beta2) * gd) * gd)
 *                 p = fp32(p - ((lr / bc_1) * m) / (sqrt(v) / sqrt(bc_2) + eps))      m, v: the values just stored
 * The running products of the betas stand where torch has pow(beta, step), so that a restatement on the host gives the
 * same bits.  The caller sets step[0] = 0 and beta_pow = (1, 1) once; the call advances them.  An entry with g = +0.0 and
 * m = v = 0 keeps the bits of p, m and v (p may be -0.0 or infinite): a packed tensor's shift | scale | clip section and
 * padding, whose gradient carl_ppo_grad writes as +0.0, stay as they are.  norm_out, where given, receives the norm before
 * the clip and the coefficient.
 * How it runs: one workgroup of 1 024 threads.  Thread t chains the squares of elements t, t + 1024, ... of tensor 0, then
 * of tensor 1, ...; a wavefront adds its 64 values by a shuffle tree, thread 0 the sixteen wavefronts' sums in order;
 * then every thread updates its elements.  No atomics, no hand-over between workgroups: two calls on equal inputs give
 * the same bits.  carl_adam_step_max_floats() is the largest total of elements this shape takes.
 * Validation, each CARL_ERR_INVALID_ARGUMENT with a message before anything is enqueued: a NULL struct; n_tensors outside
 * [1, CARL_ADAM_MAX_TENSORS]; an n < 0; more elements in all than carl_adam_step_max_floats(); a NULL param, grad, m or v;
 * step or beta_pow NULL; lr, eps or a beta not finite; lr < 0; eps <= 0; a beta outside [0, 1); max_grad_norm negative or
 * NaN.  A total of 0 elements enqueues nothing (and advances nothing).
 * Stream-ordered and capturable; never synchronises with the host; allocates nothing. */
#define CARL_ADAM_MAX_TENSORS 4
typedef struct carl_adam {
  int32_t n_tensors;
  int32_t reserved;
  int64_t n[CARL_ADAM_MAX_TENSORS];             /* elements of each tensor */
  float* param[CARL_ADAM_MAX_TENSORS];          /* DEVICE */
  const float* grad[CARL_ADAM_MAX_TENSORS];     /* DEVICE */
  float* m[CARL_ADAM_MAX_TENSORS];              /* DEVICE: first moments, zero before the first step */
  float* v[CARL_ADAM_MAX_TENSORS];              /* DEVICE: second moments, zero before the first step */
  double lr, beta1, beta2, eps;
  double max_grad_norm;                         /* >= 0; +inf: no clip */
  int64_t* step;                                /* DEVICE [1] */
  double* beta_pow;                             /* DEVICE [2]: beta1^step, beta2^step as running products */
  double* norm_out;                             /* DEVICE [2], nullable: the norm before the clip, the coefficient */
} carl_adam_t;

int64_t carl_adam_step_max_floats(void);
int carl_adam_step(const carl_adam_t* adam_host, void* stream);

/* ---- a population of PPO learners: the update of n_sets independent learners in one sequence of launches (additive; ABI
 * version unchanged) ----
 * carl_rollout_policy_valued runs several weight sets in one launch (lane l uses set l / lanes_per_set, with a log_std, a
 * critic and GAE per set).  The three calls below are carl_ppo_grad, carl_ppo_adv_stats and carl_adam_step for such a
 * population: member s owns lanes [s * lanes_per_set, (s + 1) * lanes_per_set) of one buffer and has its own actor, critic,
 * log_std, minibatch, advantage statistics, gradients, Adam state and hyperparameters.  The whole population takes the
 * launches of one learner: four per minibatch step and one per epoch.  Classic-control families only.  Each kernel runs
 * the existing kernel's own body once per member (its source is included, not restated), so MEMBER s's OUTPUTS ARE
 * BIT-EQUAL to the one-set call's on member s's rows, and no existing kernel's code changes
 * (profiles/ppo_sets_refactor_identity.txt).  No reference counterpart.
 *
 * Hyperparameters live on the device: hyper is a DEVICE double [n_sets][CARL_PPO_HYPER], row s member s's, the columns
 * named below.  The kernels read member s's row; clip_range, vf_coef and ent_coef are rounded to float32 once, where
 * carl_ppo_grad takes floats.  Precondition the host cannot check (the values are in device memory): every entry is finite
 * and >= 0, except max_grad_norm, which may be +inf (no clip).  A caller validates before it uploads.
 *
 * carl_ppo_grad_sets: carl_ppo_grad for n_sets members in its three launches.  `ppo`: the whole buffer (n_lanes = n_sets *
 * lanes_per_set); n_samples is the size of EVERY member's minibatch; its clip_range, vf_coef, ent_coef, idx and adv_norm
 * are not read.  policy / critic: n_sets = P weight sets of lanes_per_set = L lanes, params DEVICE [P][set_floats];
 * log_std DEVICE [P] (Box families).  `sets`: hyper; idx [P][idx_set_stride], required, row s the n_samples flat indices
 * t * pitch + lane of member s's minibatch; adv_norm, nullable: row s at adv_norm + s * adv_norm_set_stride is member s's
 * (mean, 1 / (std + eps)).  Outputs (carl_ppo_out_t): grad_actor [P][set_floats], grad_critic [P][set_floats],
 * grad_log_std [P] (Box families), stats [P][6], each row what carl_ppo_grad writes; new_log_prob and new_value are not
 * offered and must be NULL.  workspace: carl_ppo_sets_workspace_floats() floats, P times the one-set call's need for
 * n_samples -- up to about 13 MB per member at 256 workgroups of 64-wide networks.
 * How it runs: the grid of each launch is (carl_ppo_grad_workgroups(n_samples), P).  Member s gets the workgroup count, the
 * tile-to-workgroup mapping, the slab order and the reduction carl_ppo_grad uses for n_samples samples; the second grid
 * index picks the member's parameters, log_std, hyper row, idx row, adv_norm row, slabs and outputs, all wavefront-uniform
 * reads.  One guard is new: a sample in row s whose lane is outside member s's lanes contributes zero, exactly like an
 * index outside the buffer (n_samples still counts it), so a bad index can never mix two learners.
 * Preconditions the host cannot check: carl_ppo_grad's, per row of idx; the hyper values (above).
 * Validation, each CARL_ERR_INVALID_ARGUMENT with a message before anything is enqueued: a NULL struct; a Brax family;
 * everything carl_ppo_grad checks of the buffer, the networks' shapes and the outputs, with the same messages; n_sets < 1 or
 * n_sets > 65535 (the members are the second grid dimension; the same limit holds in the two calls below);
 * lanes_per_set not a positive multiple of carl_policy_lane_quantum(); n_sets * lanes_per_set != n_lanes; actor and critic
 * set layouts that differ; hyper or idx NULL; idx_set_stride < n_samples; adv_norm given with adv_norm_set_stride < 2;
 * n_samples > n_steps * lanes_per_set; new_log_prob or new_value not NULL; workspace NULL, off a 16-byte boundary or
 * smaller than carl_ppo_sets_workspace_floats().
 *
 * carl_ppo_adv_stats_sets: carl_ppo_adv_stats over idx [P][idx_set_stride]: row s holds member s's epoch of n_total
 * indices, the concatenation of its minibatches of batch_size (the last may be short).  Writes adv_norm [P][rows][2], rows
 * = carl_ppo_adv_stats_rows(n_total, batch_size): one workgroup per (minibatch, member), the existing kernel's arithmetic
 * and order; row (s, k) is bit-equal to carl_ppo_adv_stats on row s.  Validation: carl_ppo_adv_stats's, then n_sets < 1, n_sets > 65535 and
 * idx_set_stride < n_total.
 *
 * carl_adam_step_sets: carl_adam_step for P members in one launch, one workgroup of 1 024 threads per member.  Tensor i is
 * [P][n[i]] in dense rows (param, grad, m, v: pointers to row 0), step [P], beta_pow [P][2], norm_out [P][2] or NULL; the
 * betas and eps are shared; lr and max_grad_norm are member s's hyper columns (the struct's lr and max_grad_norm are not
 * read).  The element limit carl_adam_step_max_floats() holds per member.  Member s is bit-equal to carl_adam_step on its
 * rows.  Validation: carl_adam_step's without lr and max_grad_norm, then n_sets < 1, n_sets > 65535 and hyper NULL.  A total of 0 elements
 * enqueues nothing.
 *
 * All three: float64 sums in a fixed order, no floating-point atomics, no cooperative launch and no grid-wide barrier; the
 * same call twice gives the same bits.  Stream-ordered and capturable; never synchronise with the host; allocate nothing. */
#define CARL_PPO_HYPER 5               /* columns of a hyper row */
#define CARL_PPO_HYPER_LR 0            /* Adam's learning rate */
#define CARL_PPO_HYPER_CLIP_RANGE 1    /* c; float32 in the kernels */
#define CARL_PPO_HYPER_VF_COEF 2       /* float32 in the kernels */
#define CARL_PPO_HYPER_ENT_COEF 3      /* float32 in the kernels */
#define CARL_PPO_HYPER_MAX_GRAD_NORM 4 /* +inf: no clip */
typedef struct carl_ppo_sets {
  const double* hyper;         /* DEVICE [n_sets][CARL_PPO_HYPER] */
  const int32_t* idx;          /* DEVICE [n_sets][idx_set_stride]: row s, member s's n_samples flat indices */
  const float* adv_norm;       /* DEVICE, member s's [2] at adv_norm + s * adv_norm_set_stride; NULL: advantages as they are */
  int64_t idx_set_stride;      /* elements between two rows of idx, >= n_samples */
  int64_t adv_norm_set_stride; /* floats between two members' adv_norm rows, >= 2 (read with adv_norm) */
} carl_ppo_sets_t;

/* floats of the workspace: n_sets x carl_ppo_workspace_floats() of one-set networks of these shapes; -1 for an invalid shape,
 * n_sets < 1 (the actor's) or n_samples < 1 */
int64_t carl_ppo_sets_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples);
int carl_ppo_grad_sets(const carl_ppo_batch_t* ppo_host, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                       const float* log_std /* DEVICE [n_sets], Box families */, const carl_ppo_sets_t* sets_host,
                       const carl_ppo_out_t* out, void* stream);
int carl_ppo_adv_stats_sets(const carl_ppo_adv_stats_t* as_host, int32_t n_sets, int64_t idx_set_stride, void* stream);
int carl_adam_step_sets(const carl_adam_t* adam_host, int32_t n_sets, const double* hyper /* DEVICE [n_sets][CARL_PPO_HYPER] */,
                        void* stream);

/* ======================= Brax-locomotion families (spring backend) =======================
 * Replaces CARLBraxEnv + BraxGymWrapper/VectorGymWrapper + brax.spring.pipeline.step x
 * n_frames + brax.envs.<env>.step/reset (carl/envs/brax/carl_brax_env.py:115-336,
 * carl/envs/brax/wrappers.py:32-158; brax==0.12.1 itself is NOT in the reference tree:
 * the pipeline is restated from upstream memory, SURVEY.md section 8a "Brax restatement";
 * PARITY UNPINNED).  One maximal-coordinate rigid-body system per lane; the model (links,
 * joints, colliders, actuators, env reward constants) is a carl_brax_sys_t table shared by
 * all lanes, the per-lane context overrides gravity / friction / elasticity / ang_damping /
 * link masses / joint-stiffness scale. */
#define CARL_BRAX_MAX_LINKS 16
#define CARL_BRAX_MAX_DOF 24
#define CARL_BRAX_MAX_Q 32
#define CARL_BRAX_MAX_ACT 24
#define CARL_BRAX_MAX_COLL 32
#define CARL_BRAX_MAX_CTX_MASS 16
#define CARL_BRAX_MAX_PAIR 8

enum { CARL_BRAX_ANT = 0, CARL_BRAX_HALFCHEETAH = 1, CARL_BRAX_HUMANOID = 2, CARL_BRAX_HOPPER = 3, CARL_BRAX_WALKER2D = 4,
       CARL_BRAX_INVERTED_PENDULUM = 5, CARL_BRAX_HUMANOIDSTANDUP = 6, CARL_BRAX_INVERTED_DOUBLE_PENDULUM = 7,
       CARL_BRAX_REACHER = 8, CARL_BRAX_PUSHER = 9 };

/* context-table rows the physics reads (row index in the family's feature table, -1 =
 * feature absent -> the model default is used) */
typedef struct carl_brax_ctx_map {
  int32_t gravity, friction, elasticity, ang_damping, joint_stiffness_scale;
  int32_t target_distance, target_direction, target_radius; /* goal mode rows (carl_ant.py:40-48) */
  int32_t n_mass;                               /* mass_<link> features */
  int32_t mass_row[CARL_BRAX_MAX_CTX_MASS];     /* table row */
  int32_t mass_link[CARL_BRAX_MAX_CTX_MASS];    /* link it scales */
  float mass_nominal[CARL_BRAX_MAX_CTX_MASS];   /* CARL default: value / nominal scales the link's effective mass
                                                 * (an EXTENSION of this build, like joint_stiffness: with brax's
                                                 * spring_mass_scale = 1 the spring backend runs every link at
                                                 * m**(1 - 1) = 1, so upstream a mass context would not move it) */
  float mass_ratio_floor[CARL_BRAX_MAX_CTX_MASS]; /* the ratio is clamped from below at this value per env (0 = no
                                                 * clamp): lighter links push the explicit spring integration past
                                                 * its stability bound (NaNs within a few steps); the context
                                                 * OBSERVATION keeps the unclamped value.  This floor applies to an
                                                 * env in which ONE mass feature is lighter than nominal ... */
  float mass_ratio_floor_multi[CARL_BRAX_MAX_CTX_MASS]; /* ... and this (higher) one when two or more are (ratio <
                                                 * 0.999): several light links at once are less stable than each
                                                 * alone (measured: tools/mass_combo_sweep.py) */
  int32_t goal_position[3];                     /* push task: goal_position_x / _y / _z rows (carl_pusher.py:80-103) */
} carl_brax_ctx_map_t;

typedef struct carl_brax_sys {
  int32_t env_kind;      /* CARL_BRAX_* : selects reward / obs / done rule */
  int32_t n_links, n_q, n_dof, n_act, n_coll, n_frames, obs_dim;
  int32_t max_episode_steps;   /* brax EpisodeWrapper episode_length (1000) */
  int32_t terminate_when_unhealthy;
  int32_t exclude_current_positions;  /* leading q entries left out of the observation (Ant 2, Halfcheetah 1) */
  int32_t reserved;
  float dt;              /* substep */
  float gravity_z, vel_damping, ang_damping, baumgarte_erp, elasticity, friction;
  float healthy_z_lo, healthy_z_hi, healthy_reward, ctrl_cost_weight, forward_reward_weight;
  float reset_noise_scale, reset_vel_scale;
  /* links, topological order, parent < child */
  int32_t parent[CARL_BRAX_MAX_LINKS];      /* -1: free root */
  int32_t n_link_dof[CARL_BRAX_MAX_LINKS];  /* 6 = free root; else n_slide prismatic dofs followed by 0..3
                                               revolute dofs turning, in order, about the joint frame's x, y,
                                               +-z axes (each carried by the preceding ones: MuJoCo's stacking of
                                               several hinges in one body).  parent -1 with n_link_dof < 6 =
                                               jointed to the static world (planar roots) */
  int32_t q_start[CARL_BRAX_MAX_LINKS], dof_start[CARL_BRAX_MAX_LINKS];
  float link_pos[CARL_BRAX_MAX_LINKS][3], link_rot[CARL_BRAX_MAX_LINKS][4];   /* child frame in parent frame at q = 0 */
  float joint_pos[CARL_BRAX_MAX_LINKS][3], joint_rot[CARL_BRAX_MAX_LINKS][4]; /* anchor / joint frame in the child frame */
  float com[CARL_BRAX_MAX_LINKS][3];        /* centre of mass in the link frame */
  float mass[CARL_BRAX_MAX_LINKS];          /* effective (spring_mass_scale applied) */
  float inv_inertia[CARL_BRAX_MAX_LINKS][3];/* effective inverse principal moments, link frame.  Every shipped model is
                                             * isotropic ([0] == [1] == [2]: brax's spring_inertia_scale = 1); a model with a
                                             * link whose three moments differ is stepped by the general kernels (the ones
                                             * the reach / push task models take: 4, 8 or 16 lanes per env), the only ones
                                             * that carry R diag(inv_inertia) R^T -- same results, lower throughput */
  float k_pos[CARL_BRAX_MAX_LINKS], k_vel[CARL_BRAX_MAX_LINKS];        /* constraint_stiffness / _vel_damping */
  float k_limit[CARL_BRAX_MAX_LINKS], k_ang_damp[CARL_BRAX_MAX_LINKS]; /* constraint_limit_stiffness / _ang_damping */
  float dof_lo[CARL_BRAX_MAX_DOF], dof_hi[CARL_BRAX_MAX_DOF];
  float dof_damping[CARL_BRAX_MAX_DOF], dof_stiffness[CARL_BRAX_MAX_DOF];
  int32_t act_dof[CARL_BRAX_MAX_ACT];
  float act_gear[CARL_BRAX_MAX_ACT], act_lo[CARL_BRAX_MAX_ACT], act_hi[CARL_BRAX_MAX_ACT];
  int32_t coll_link[CARL_BRAX_MAX_COLL];    /* collision spheres vs the plane z = plane_z (0: the ground) */
  float coll_pos[CARL_BRAX_MAX_COLL][3], coll_radius[CARL_BRAX_MAX_COLL];
  float init_q[CARL_BRAX_MAX_Q];
  /* goal-directed reward epilogue (carl/envs/brax/brax_walker_goal_wrapper.py:113-140): position +=
   * obs[goal_obs_idx] * goal_dt (the RAW MJCF timestep, Quirk B3); reward = max(0, d_prev - d_cur);
   * terminate with success when d_cur <= target_radius */
  int32_t goal_mode;
  int32_t goal_obs_idx[2];
  float goal_dt;
  int32_t n_slide[CARL_BRAX_MAX_LINKS];        /* 0..2 prismatic dofs (q order: slides, then the hinges) */
  float dof_sign3[CARL_BRAX_MAX_LINKS];        /* +1 / -1: third hinge axis = sign * (x cross y) of the joint frame */
  int32_t reset_vel_uniform;                   /* qd noise: 1 = U(-scale, scale) (humanoid), 0 = scale * N(0,1) */
  int32_t reward_on_com;                       /* forward velocity of the whole-body centre of mass (humanoid) */
  int32_t obs_extended;                        /* append com inertia (L x 10), com velocity (L x 6), qfrc_actuator */
  int32_t healthy_q_index;                     /* >= 0: the env is healthy only while q[index] is inside
                                                * [healthy_q_lo, healthy_q_hi] (hopper / walker2d torso pitch,
                                                * inverted-pendulum pole angle); -1: no such check */
  float healthy_q_lo, healthy_q_hi;
  float obs_qd_clip;                           /* > 0: velocities in the observation are clipped to +-this */
  int32_t lanes_per_env;                       /* HOST-side launch hint: lanes that share one env (rounded up
                                                * to an instantiated width, carl_brax_lane_widths); 0 = chosen
                                                * by the library from the model and the batch size */
  int32_t reward_height;                       /* 1: the "forward" term is weight * (root z) / dt_env
                                                * (humanoidstandup's uph_cost) instead of weight * dx / dt_env */
  int32_t obs_trig_from;                       /* > 0: coordinates q[obs_trig_from:] appear in the observation as
                                                * sin(q[from:]) ++ cos(q[from:]) instead of q[from:]
                                                * (inverted double pendulum); 0: plain q */
  /* tip reward / termination (brax.envs.inverted_double_pendulum): with tip = frame origin of
   * tip_link + R * tip_offset, reward = healthy_reward - (tip_x_weight * tip.x^2 + (tip.z -
   * tip_height)^2) - (tip_vel_weight[k] * qd[tip_vel_dof[k]]^2, k = 0, 1); done when tip.z <=
   * tip_min_height.  tip_link = 0: not used (the root is never the tip) */
  int32_t tip_link;
  float tip_offset[3];
  float tip_x_weight, tip_height, tip_min_height;
  float tip_vel_weight[2];
  int32_t tip_vel_dof[2];
  /* reach task (brax.envs.reacher; reference class carl/envs/brax/carl_reacher.py:9-39): target_link > 0
   * names the LAST link, jointed to the world by two slides whose coordinates q[tq : tq + 2]
   * (tq = q_start[target_link]) are the goal.  reset: q[tq], q[tq + 1] = d cos(a), d sin(a) with
   * d = target_max_dist * U, a = 2 pi U (draws n_q + n_dof and + 1 of the reset stream), goal rates 0;
   * observation = cos(q[:tq]) ++ sin(q[:tq]) ++ q[tq:] ++ qd[:dof_start[target_link]] ++ (tip - goal
   * position), tip = frame origin of tip_link + R * tip_offset; reward = -|tip - goal| -
   * ctrl_cost_weight * |a|^2; never terminates.  0: not used */
  int32_t target_link;
  float target_max_dist;
  /* push task (brax.envs.pusher; reference class carl/envs/brax/carl_pusher.py:9-103): push_link > 0 names
   * the LAST link (the object), on two slides against the world; every link before it is the arm (hinges
   * only), tip_link its end effector.  With goal = the context's goal_position_* (ctx.goal_position; rows
   * absent: push_goal):
   *   reset: arm q = init_q + reset_noise_scale U(-1, 1), arm rates U(-reset_vel_scale, reset_vel_scale);
   *          object offset c = push_lo + (push_hi - push_lo) U (draws n_q + n_dof and + 1 of the reset
   *          stream); d = link_pos[push_link].xy + c - goal.xy is stretched to length push_min_dist when
   *          shorter; object slides = goal.xy + d - link_pos.xy, at rest;
   *   observation = q[:na] ++ qd[:na] ++ COM(tip_link) ++ COM(push_link) ++ goal (na = arm dofs);
   *   reward = -|COM(object) - goal| - ctrl_cost_weight |a|^2 - push_near_weight |COM(object) - COM(tip)|;
   *   never terminates.  0: not used */
  int32_t push_link;
  float push_goal[3];
  float push_near_weight, push_min_dist;
  float push_lo[2], push_hi[2];
  /* link-pair contact of the push task: n_pair spheres fixed to pair_link (centre pair_pos[k] in its
   * frame, radius pair_radius[k]) against the object, an upright cylinder (radius pair_obj_radius, half
   * height pair_obj_half) centred at the frame origin of push_link.  A sphere whose centre is within
   * pair_obj_half + r_k of the object's mid-height and closer than r_k + R in the horizontal plane pushes
   * the object along the horizontal normal n with fm = max(0, pair_k depth + pair_c closing speed); the
   * opposite force acts on pair_link at the sphere's centre (the object's own rotation is locked by its
   * joint).  ABI 8 -- contact friction and the table:
   *   pair_ct > 0: Coulomb friction in the pair contact, regularised -- with vt the HORIZONTAL part of the sphere's
   *     velocity relative to the object minus its normal part, the object is dragged along vt by min(pair_ct |vt|, friction fm)
   *     (`friction`: the env's context value, as in the plane contacts) and the sphere held back by the same;
   *   obj_support = 1: the object rests on the plane z = plane_z (its joint has no vertical freedom, so the
   *     plane carries its weight): every substep, after the force update, its horizontal velocity shrinks by
   *     min(friction |gravity_z| dt, |v_h|) -- Coulomb friction under the normal load m |g| as an impulse, the
   *     form the sphere / plane contacts use (a sliding puck stops dead after v0^2 / (2 mu g));
   *   plane_z: the height of THE collision plane (0 for the locomotion models; the push task's table): every
   *     sphere of coll_* collides with z = plane_z. */
  int32_t n_pair, pair_link;
  float pair_pos[CARL_BRAX_MAX_PAIR][3], pair_radius[CARL_BRAX_MAX_PAIR];
  float pair_obj_radius, pair_obj_half, pair_k, pair_c;
  float pair_ct, plane_z;
  int32_t obj_support, reserved2;
  float slide_axis[CARL_BRAX_MAX_LINKS][2][3]; /* unit axes in the PARENT frame, mutually orthogonal */
  carl_brax_ctx_map_t ctx;
} carl_brax_sys_t;

/* persistent state per link: COM position 3, rotation 4 (w,x,y,z), linear velocity 3, angular velocity 3
 * (world frame) = 13 quantities.  The pose (the first 7) is carried to 48 significant bits as a float32 head
 * plus a float32 tail -- the spring pipeline multiplies pose DIFFERENCES by k dt / m = 20 .. 50 per substep, so a
 * pose rounded to float32 between steps costs 1e-5 of velocity per env step -- which makes
 * CARL_BRAX_LINK_RECORD = 20 floats per link in HBM.  One env's record = its L links' 80-byte records one after the
 * other (ABI 8; ABI 5 - 7 kept three blocks per env: heads, tails, velocities), a link's record being
 *   [0, 7)    pose head (p.x p.y p.z r.w r.x r.y r.z): the pose to float32
 *   [7, 14)   pose tail: pose = (double)head + (double)tail
 *   [14, 20)  velocities (v.x v.y v.z w.x w.y w.z)
 * -- the lane that owns a link moves it as five 16-byte pieces, a wavefront's envs x links one contiguous run. */
#define CARL_BRAX_LINK_STATE 13
#define CARL_BRAX_LINK_RECORD 20

/* carl_batch_t is reused: family = CARL_N_FAMILIES + env_kind is ignored here (sys decides),
 * state is [n_lanes][n_links][CARL_BRAX_LINK_RECORD] (env-major, then link-major: the lanes that share an env move
 * its 20 L floats as one contiguous run; the classic-control families keep [S][n_lanes]), ctx_table rows follow the CARL
 * class's feature table.
 * action is float32 [n_lanes][n_act] (lane-major, like obs).  `sys` is a DEVICE pointer to
 * one carl_brax_sys_t.  */
int carl_brax_reset(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                    const uint8_t* mask, float* obs, void* stream);
int carl_brax_step(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                   const carl_step_io_t* io, void* stream);
int carl_brax_rollout(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                      const carl_step_io_t* io, int32_t n_steps, void* stream);
/* the lane-group widths (values for sys.lanes_per_env) this library can launch for STEP / ROLLOUT launches of the model
 * in a batch with these carl_batch_t::flags (ABI 9: CARL_FLAG_BRAX_GENERIC moves a planar model to the general kernels,
 * whose instantiated widths differ), ascending; returns their number (<= cap).  Results do not depend on the width:
 * it is a pure scheduling choice (carl_amd.brax_engine.BraxVecEngine.autotune times them on the real batch).  No
 * reference counterpart (brax vmaps one env per array row, carl/envs/brax/carl_brax_env.py:163-167). */
int carl_brax_lane_widths(const carl_brax_sys_t* sys_host, uint32_t batch_flags, int32_t* widths_out, int32_t cap);
/* 1 when step / rollout launches of this model take the planar substep (root on two world slides x, z and a hinge
 * about y, every other link on a hinge about +-y, all geometry in the y = 0 plane: Halfcheetah, Hopper, Walker2d as
 * carl_amd.envs.brax.models builds them) unless the batch carries CARL_FLAG_BRAX_GENERIC; 0 otherwise.  The planar
 * substep neither reads nor updates out-of-plane state components, so a caller that writes states itself asks here
 * (carl_amd.brax_engine.BraxVecEngine.set_state64 does, and falls back to the general substep).  No reference
 * counterpart: brax's spring pipeline has one code path (carl/envs/brax/carl_brax_env.py:163-176). */
int carl_brax_model_is_planar(const carl_brax_sys_t* sys_host);
/* How a step / rollout launch of a batch larger than the chip holds at once is divided (no reference counterpart: the
 * reference steps its envs in vmapped lock-step, carl/envs/brax/carl_brax_env.py:163-190).  A "group" is one
 * wavefront's worth of envs; workgroup w of n_workgroups owns a contiguous share of the n_groups groups and cuts its
 * groups x n_steps group-steps into one contiguous piece per wavefront.  Writes, for (workgroup, wave), the fragments
 * in the order the wavefront runs them -- five int32 each: global group, first step, one-past-last step, waits for the
 * previous wavefront's hand-over (0/1), hands over to the next wavefront (0/1) -- and returns their number (-1: bad
 * argument).  Pure integer arithmetic, no device access: it is the same code the kernel runs (tests/test_abi.py checks
 * that every group-step is run exactly once, in step order, and that no hand-over can wait on a later one). */
int carl_brax_fragment_plan(int32_t n_groups, int32_t n_workgroups, int32_t waves_per_workgroup, int32_t n_steps,
                            int32_t workgroup, int32_t wave, int32_t* fragments_out, int32_t cap);

/* ---- closed-loop rollout of the Brax families (additive; ABI version unchanged) ----
 * carl_rollout_policy refuses a Brax batch; this is its Brax counterpart, a mode of the rollout kernel itself: T steps of
 * every env in ONE launch, each step's action computed on the device by `policy_host` from the env's current context and
 * observation.  No reference counterpart: the reference steps the env per Python call and its caller runs the policy
 * between the calls (carl/envs/carl_env.py:321-342, examples/carl_with_sb3.py).
 * The policy is a carl_policy_t as carl_rollout_policy specifies it -- the same input vector
 *   x = [ctx_table[ctx_rows[0]][c], ..., ctx_table[ctx_rows[n_ctx - 1]][c], obs_0, ..., obs_{obs_dim - 1}]
 * (c: the env's CURRENT context, after any auto-reset of the previous step), the same transform, layers, activations and
 * arithmetic (explicit fma, input order, bias first; tanh as described there), the same packed parameters -- with
 *   head == CARL_POLICY_HEAD_BOX, n_out == sys.n_act (the action is the head's n_act outputs as they come; the env clips
 *   them exactly as it clips actions given to carl_brax_rollout), n_in == n_ctx + sys.obs_dim <= CARL_POLICY_MAX_IN
 *   (Humanoid's and HumanoidStandup's 244 observations are refused), every ctx_rows[k] one of batch.ctx_obs_feat,
 *   lanes_per_set a positive multiple of carl_policy_lane_quantum() with n_sets * lanes_per_set >= n_lanes (env l uses
 *   set l / lanes_per_set), params on a 16-byte boundary, carl_brax_policy_set_floats() floats per set
 *   (carl_policy_set_floats limits n_out to 4).
 * `obs` [n_lanes][obs_dim] (DEVICE) holds every env's current observation when the launch starts -- what carl_brax_reset
 * and carl_brax_step leave in their obs arrays -- and every env's last observation when it ends.
 *  - transitions mode (io != NULL): everything carl_brax_rollout writes (dense rows), with io->action [T][n_lanes][n_act]
 *    float32 an OUTPUT: row t holds the actions step t took.  carl_brax_rollout of those actions from the same engine
 *    state gives the same bits, and the same engine state.
 *  - summary mode (io == NULL): no per-step stores; summary_out (required) receives each env's totals as
 *    carl_rollout_policy defines them.  A summary (in either mode) needs CARL_FLAG_AUTORESET, else CARL_ERR_UNSUPPORTED.
 * The batch, the model and io are checked as carl_brax_rollout checks them.  CARL_FLAG_BRAX_FP32 is refused with
 * CARL_ERR_UNSUPPORTED; both auto-reset modes and the goal wrapper work as in carl_brax_rollout.  Sampled actions and
 * their log-probabilities: carl_brax_rollout_policy_sampled below; the episodes mode: carl_brax_evaluate_policy, its input
 * statistics carl_brax_evaluate_policy_stats; a critic inside the sampled launch: carl_brax_rollout_policy_valued (then
 * carl_gae, which takes dense [T][n_lanes] rows).  Out of scope: a sampled episodes mode and Humanoid-size inputs. */
int carl_brax_rollout_policy(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                             float* obs, const carl_policy_t* policy_host, const carl_step_io_t* io, int32_t n_steps,
                             const carl_policy_summary_t* summary_out, void* stream);
/* carl_brax_rollout_policy with sampled actions (additive; ABI version unchanged): a diagonal Gaussian over all the model's
 * actuators, the data an on-policy learner collects (the reference's example agent is SB3 PPO over a CARL env,
 * examples/carl_with_sb3.py, which samples and scores the action in Python between two env steps).
 * The network, its inputs and its arithmetic are carl_brax_rollout_policy's, unchanged; the head's n_act outputs are the
 * means mu_j.  `sampling` is a carl_policy_sampling_t with these meanings:
 *   seed      sample_seed, the Philox key of the draws;
 *   log_std   DEVICE [n_sets][n_act]: one state-independent value per weight set and actuator (SB3's log_std parameter);
 *   log_prob  optional DEVICE [T][n_lanes] fp32, dense rows as every Brax output: the joint log-probability of each
 *             env-step's action; transitions mode only.
 * Random words: actuator j of an env-step uses Philox4x32-10 block b = j >> 1, key sample_seed, counter
 *   (genv lo, genv hi, e, 0x40000000 | (b << 28) | elapsed)
 * with genv = lane_offset + env, e the env's episode counter - 1 and elapsed the env's step count in that episode before
 * the step, both as carl_policy_sampling_t defines them.  Even j takes (w.x, w.y) of its block, odd j (w.z, w.w), as the
 * (u1, u2) of the Gaussian rule above:
 *   u1 = ((wa >> 8) + 1) * 2^-24, u2 = (wb >> 8) * 2^-24;  z_j = sqrt(-2 ln u1) * cos(2 pi u2);
 *   a_j = fma(exp(log_std[set][j]), z_j, mu_j);  lp_j = fma(-z_j / 2, z_j, -log_std[set][j] - ln(2 pi) / 2);
 *   log_prob = lp_0 + lp_1 + ... summed in fp32 in actuator order;
 * exp / log / sqrt / cos the device's accurate fp32 functions, every product rounded on its own.  The tag is 0x4..., not
 * the classic rule's 0x8...: the Brax reset draws use 0x80000000 | block with the batch seed, which a caller may pass as
 * sample_seed.  b has two bits -- eight actuators, what every model whose observation fits CARL_POLICY_MAX_IN has at most
 * (a model table with more, up to CARL_BRAX_MAX_ACT, is refused) -- which leaves elapsed < 2^28.
 * A draw is therefore a pure function of (sample_seed, global env, episode, step in episode, actuator): it does not depend
 * on the mode, on how a horizon is split into launches, on the lane width or on which wavefront of a split group runs the
 * step.  The recorded action is the raw a_j; the step clips it exactly as it clips a deterministic action, and
 * carl_brax_rollout of the recorded actions from the same engine state reproduces the launch bit for bit.  A summary
 * launch stores nothing per step and leaves the state the transitions launch leaves.  An env past the end of the batch
 * draws nothing.
 * Validation: everything carl_brax_rollout_policy checks, in its order and with its codes; then `sampling` non-NULL,
 * log_std non-NULL, no log_prob in summary mode (io == NULL), sys.n_act <= 8 and 0 < batch->max_episode_steps <= 2^28, each refused with
 * CARL_ERR_INVALID_ARGUMENT before anything is enqueued.  n_lanes == 0 enqueues nothing.  The launch has the shape
 * carl_brax_policy_launch_shape reports.  With a critic: carl_brax_rollout_policy_valued.  Out of scope: a sampled episodes
 * mode. */
int carl_brax_rollout_policy_sampled(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                     float* obs, const carl_policy_t* policy_host, const carl_policy_sampling_t* sampling,
                                     const carl_step_io_t* io, int32_t n_steps, const carl_policy_summary_t* summary_out,
                                     void* stream);
/* ---- a critic in the sampled Brax launch (additive; ABI version unchanged) ----
 * carl_brax_rollout_policy_valued is the transitions-mode carl_brax_rollout_policy_sampled with a second network, the
 * critic, evaluated inside the rollout kernel on the inputs the actor sees: everything the sampled call writes (records,
 * actions, log-probabilities, engine state, `obs`, summary totals) keeps its bits, and the three columns of
 * carl_policy_value_t are written beside them, dense rows as every Brax output.  carl_rollout_policy_valued's contract,
 * for these families: with carl_gae one launch and one GAE launch fill an on-policy rollout buffer, under every context
 * selector and without host synchronisation -- the launch knows the context an env ran in at every step, and at a
 * truncation it still holds both the terminal observation and the context of the episode that just ended.
 * The critic is a carl_policy_t with n_out == 1, hidden widths in [1, CARL_POLICY_MAX_WIDTH] and an activation of its own,
 * and the actor's n_in, n_ctx, ctx_rows, n_sets and lanes_per_set; `head` is not read.  It reads the actor's transformed
 * inputs x (after the actor's shift / scale / clip): the shift | scale | clip section of its own packed block is NOT READ.
 * V = y[0]: bias first, explicit fma in input order, the actor's activations and tanh.  Its block is packed by the Brax
 * rule (carl_brax_policy_set_floats() floats per set) and params starts on a 16-byte boundary.
 *   value      [n_steps][n_lanes] fp32: V(x_t), x_t the input step t's action was chosen from
 *   last_value [n_lanes] fp32: V of each env's input after the launch's last step -- its current context (the new one if
 *              that step reset it) and its current observation
 *   boot_value [n_steps][n_lanes] fp32, NULL: not wanted.  Needs CARL_FLAG_AUTORESET (CARL_ERR_UNSUPPORTED without).  On an
 *              env-step with truncated && !terminated: V([context values of the context the episode ran in, terminal
 *              observation]); +0.0f on every other env-step; every slot of rows [0, n_steps) is written.  Both auto-reset
 *              modes give the same rule.
 * Validation, in this order: everything carl_brax_rollout_policy checks (batch, model, policy / obs, the refusal of
 * CARL_FLAG_BRAX_FP32, the policy; then n_steps, io, the summary); io != NULL (transitions mode only:
 * CARL_ERR_INVALID_ARGUMENT); the sampling checks of carl_brax_rollout_policy_sampled, with `sampling` and
 * sampling->log_prob required; the critic, each refusal with a message of its own; out, out->value and out->last_value
 * non-NULL.  n_lanes == 0 or n_steps == 0 enqueues nothing and writes nothing.  The launch has the shape
 * carl_brax_policy_launch_shape reports, and no LDS beyond the sampled launch's.  Out of scope: a deterministic valued
 * launch. */
int carl_brax_rollout_policy_valued(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                    float* obs, const carl_policy_t* policy_host, const carl_policy_t* critic_host,
                                    const carl_policy_sampling_t* sampling, const carl_step_io_t* io, int32_t n_steps,
                                    const carl_policy_summary_t* summary_out, const carl_policy_value_t* out, void* stream);
/* Episodes mode of carl_brax_rollout_policy (additive; ABI version unchanged): carl_evaluate_policy's semantics for the
 * Brax families, a variant of the same rollout kernel.  No reference counterpart: the reference evaluates a policy by
 * stepping the env per Python call until `done` (carl/envs/carl_env.py:321-342; examples/carl_with_sb3.py runs SB3's
 * evaluate_policy over it).
 * Every env runs `policy_host` (as carl_brax_rollout_policy, deterministic) until it has finished n_episodes episodes or
 * taken max_steps steps in this launch, whichever comes first.  An env is LIVE until then.  At the step that ends its
 * n_episodes-th episode that step's auto-reset is applied as always (both auto-reset modes, the goal wrapper, the push
 * task's goal placement) and the env FREEZES: its state record, elapsed, ep_return, ctx_idx, episode, n_calls, the
 * episodes_done increment, goal_pos and its current observation in `obs` are stored then -- the start of the next episode,
 * as per-call stepping leaves it -- and nothing of it is stored afterwards (last_return / last_length, the finished-episode
 * log and ctx_obs included).  An env that reaches max_steps first stops there, mid-episode, exactly as
 * carl_brax_rollout_policy of max_steps steps leaves it.  An env's records and its stored state are bit-identical to its
 * first episodes in, and to its state after as many steps of, a transitions-mode carl_brax_rollout_policy from the same
 * engine state.  Episodes are counted from the current state: one already running is reported with its full length and
 * return.  A wavefront leaves the step loop once none of its envs is live.
 * `out` is carl_evaluate_policy's: slot k of an env holds ret (the fp32 ep_return at the episode's end, summed in step
 * order), length, context_id (ctx_idx before the step that ended it) and terminated; episodes [env] and steps [env] are
 * written for every env, and every slot at or beyond episodes [env] as NaN / 0 / -1 / 0, so nothing needs clearing.
 * Validation: everything carl_brax_rollout_policy checks, in its order (batch, model, policy / obs, the refusal of
 * CARL_FLAG_BRAX_FP32, the policy); then out and its six arrays non-NULL, n_episodes >= 1, max_steps >= 0 and n_episodes *
 * n_lanes < 2^31.  A failure returns CARL_ERR_INVALID_ARGUMENT before anything is enqueued; without CARL_FLAG_AUTORESET
 * the call returns CARL_ERR_UNSUPPORTED.  n_lanes == 0 enqueues nothing; max_steps == 0 fills every output and steps
 * nothing.  No host synchronisation: stream-ordered and capturable.  The launch has the shape
 * carl_brax_policy_launch_shape reports for n_steps = max_steps. */
int carl_brax_evaluate_policy(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                              float* obs, const carl_policy_t* policy_host, int32_t n_episodes, int32_t max_steps,
                              const carl_policy_episodes_t* out, void* stream);
/* ---- input statistics inside the Brax episodes launch (additive; ABI version unchanged) ----
 * carl_evaluate_policy_stats for the Brax families: what ARS V2 needs to normalise these models' inputs.  No reference
 * counterpart.
 * carl_brax_evaluate_policy_stats is carl_brax_evaluate_policy: the records, the engine state and `obs` are its, bit for
 * bit, and the launch has its shape.  In addition it gathers what carl_evaluate_policy_stats gathers, word for word: for
 * every LIVE env-step (the steps out.steps counts: a frozen env that computes along in a live wavefront, an env past the end
 * of the batch and a wavefront's spare lanes add nothing) and every policy input i < n_in, in FlattenObservation order,
 *     d_i = fp32(x_i - shift_i),   S1_i += d_i,  S2_i += d_i * d_i
 * with x_i the raw input the policy acted on at that step (the context value of the env's current context, or the
 * observation before the step) and shift_i that of the env's own weight set.  One float64 slab [2][CARL_POLICY_MAX_IN] per
 * WAVEFRONT of the launch, partial[workgroup * waves_per_workgroup + wave] (carl_brax_policy_launch_shape): the wavefront's
 * sums over all the (group, step range) fragments it ran, written once and in full, +0.0 at and beyond n_in and in the
 * slab of a wavefront that ran nothing, so nothing needs clearing.  The number of env-steps is the sum of out.steps.
 * Accuracy, from the operation list: d_i is one fp32 subtraction, the contract's own; it and its square are widened to
 * float64 exactly (the square of an fp32 value has at most 48 significant bits).  At every step a wavefront takes, lane i
 * adds the terms of its at most 64 / lanes_per_env envs in env order into a float64 step sum that starts at +0.0, then adds
 * the step sum to the slab's running float64 sum.  Nothing is added in fp32.  With u = 2^-53, a slab entry that took s
 * wavefront-steps has |S1_i - exact| <= (s + 64 / lanes_per_env) * u * sum |d_i| and likewise S2_i against sum d_i^2
 * (recursive summation, first order in u) -- for EVERY input, context and observation alike: float64 rounding only, below
 * the classic entry point's 10 * 2^-24 bound by a factor of 2^28 / s.  carl_brax_policy_stats_merge's constant rule needs
 * the relative error of the sums well under 2^-36: guaranteed (at most 2^-39) for s <= 2^14 - 32 wavefront-steps per
 * slab, i.e. (groups per wavefront) * max_steps <= 16 352 -- up to 523 264 env-steps per wavefront at 2 lanes per env,
 * 114 464 at 9; beyond that the bound grows linearly with s and the rule's margin shrinks with it.  No floating-point
 * atomics, no workgroup barrier: the slabs are a fixed function of the launch's inputs and shape, the same bits on every
 * repetition from the same state.
 * Validation: everything carl_brax_evaluate_policy checks, in its order and with its codes; then `stats` and
 * stats->partial non-NULL, partial on a 16-byte boundary and partial_capacity >= carl_brax_policy_stats_slabs(batch,
 * sys_host, policy_host, max_steps): CARL_ERR_INVALID_ARGUMENT before anything is enqueued.  n_lanes == 0 enqueues nothing.
 * max_steps == 0 fills the records as carl_brax_evaluate_policy does and writes every slab as zeros. */
int carl_brax_evaluate_policy_stats(const carl_batch_t* batch, const carl_brax_sys_t* sys_dev, const carl_brax_sys_t* sys_host,
                                    float* obs, const carl_policy_t* policy_host, int32_t n_episodes, int32_t max_steps,
                                    const carl_policy_episodes_t* out, const carl_policy_stats_t* stats, void* stream);
/* The slabs that launch writes: grid * waves_per_workgroup of carl_brax_policy_launch_shape for n_steps = max_steps; for
 * max_steps == 0, where nothing is launched over the envs, the count of max_steps == 1.  Host only (as
 * carl_brax_policy_launch_shape).  0 for n_lanes <= 0; -1 for a NULL argument, max_steps < 0, a model table out of range,
 * CARL_FLAG_BRAX_FP32 or a model without a launch shape. */
int32_t carl_brax_policy_stats_slabs(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                                     int32_t max_steps);
/* carl_policy_stats_merge for the slabs of carl_brax_evaluate_policy_stats: the same kernel, arithmetic, constant rule and
 * validation list, with n_slabs in the place of n_workgroups and the packing rule of the Brax families -- set_floats =
 * carl_brax_policy_set_floats() (n_out up to CARL_BRAX_MAX_ACT; carl_policy_stats_merge refuses such a shape), the
 * transform offset the floats of every W and b.  Stream-ordered and capturable like the launch above; neither call
 * synchronises with the host or allocates. */
int carl_brax_policy_stats_merge(const carl_policy_t* policy_host, const carl_policy_stats_t* stats, int32_t n_slabs,
                                 const int32_t* steps /* DEVICE [n_lanes] */, int32_t n_lanes,
                                 const carl_policy_running_stats_t* running, double eps, double min_std,
                                 float* params_out /* DEVICE [n_write][set_floats], nullable */, int32_t n_write,
                                 void* stream);
/* floats per packed weight set of a Brax policy's shape (n_out up to CARL_BRAX_MAX_ACT); -1 for an invalid shape */
int32_t carl_brax_policy_set_floats(const carl_policy_t* policy_host);

/* ---- the PPO update on the device for the Brax families (additive; ABI version unchanged) ----
 * carl_brax_rollout_policy_valued + carl_gae leave a complete PPO rollout buffer on the device; the two calls below are
 * carl_policy_context_trace and carl_ppo_grad for it: dense rows, a joint Gaussian over the model's n_act <= 8 actuators
 * with one log_std each, networks packed by the Brax rule (carl_brax_policy_set_floats() floats per set).  The classic
 * entry points keep refusing a Brax family; these refuse a classic one.  No existing kernel is touched.
 *
 * carl_brax_policy_context_trace: the walk documented at carl_policy_context_trace over dense rows ([n_steps][n_lanes]),
 * one thread per env, the selector called with (c, lane_offset + env, e).  One rule is added: with
 * CARL_FLAG_AUTORESET_FIRST_STATE set and batch->first_state != NULL a done env is put back to its first state, keeps its
 * context and does not advance its episode counter, so c never moves and e does not advance (as without auto-reset).
 * `batch` is read for family, n_lanes, n_contexts, selector, selector_stride, flags, seed, lane_offset and for whether
 * first_state is NULL.  Validation, each CARL_ERR_INVALID_ARGUMENT before anything is enqueued, in this order: a NULL
 * batch, a classic-control family, n_lanes or n_steps < 0, n_contexts < 1, an unknown selector, a NULL pointer.
 * n_lanes == 0 or n_steps == 0 enqueues nothing. */
int carl_brax_policy_context_trace(const carl_batch_t* batch, const int32_t* ctx_idx0 /* DEVICE [n_lanes] */,
                                   const uint32_t* episode0 /* DEVICE [n_lanes] */,
                                   const uint8_t* terminated /* DEVICE [n_steps][n_lanes] */,
                                   const uint8_t* truncated /* DEVICE [n_steps][n_lanes] */, int32_t n_steps,
                                   int32_t* context_id /* DEVICE [n_steps][n_lanes] */, void* stream);

/* carl_brax_ppo_grad: carl_ppo_grad for a Brax model.  `ppo` is a carl_ppo_batch_t read with Brax meanings: family is
 * not a classic one; rows are dense (row_pitch 0 or n_lanes); obs_dim == sys_host->obs_dim; action is
 * [n_steps][n_lanes][n_act] float32 (CARL_ACTION_F32), the raw samples the launch recorded (the env's clip does not
 * enter, as in SB3); context_id comes from carl_brax_policy_context_trace.  sys_host is read for obs_dim and n_act only.
 * A sample's input is [ctx_table[ctx_rows[k]][context_id[t][env]] for k < n_ctx, then obs0[env] (t == 0) or
 * obs[t - 1][env]] under the actor's shift / scale / clip; the critic reads the same transformed x.  Forward arithmetic
 * is the closed loop's (bias first, explicit fma in input order, the same tanh).  The loss, the statistics and the
 * clipping rule are exactly carl_ppo_grad's; the head is the joint Gaussian with log_std [n_act] on the device:
 *   z_j = (a_j - mu_j) exp(-log_std_j)
 *   lp  = sum_j fma(-z_j / 2, z_j, -log_std_j - ln(2 pi) / 2)   summed in fp32 in actuator order, as the sampled launch sums
 *   H   = sum_j (1/2 + ln(2 pi) / 2 + log_std_j)
 *   dlp/dmu_j = z_j exp(-log_std_j),  dlp/dlog_std_j = z_j^2 - 1,  dH/dlog_std_j = 1
 * Outputs (carl_ppo_out_t): grad_actor / grad_critic [carl_brax_policy_set_floats()] in the packed layout, their shift |
 * scale | clip entries and round-up padding +0.0; grad_log_std [n_act]; stats [6], new_log_prob / new_value [n_samples] as
 * carl_ppo_grad's.  An idx entry outside the buffer is skipped as carl_ppo_grad skips it (it contributes zero, n_samples
 * still counts it); new_log_prob[m] / new_value[m] of a skipped entry are not written.
 * How it runs: carl_ppo_grad's scheme -- a persistent launch per network of carl_brax_ppo_grad_workgroups(n_samples)
 * workgroups over tiles of carl_brax_ppo_tile() samples, the weights staged in LDS once per workgroup, one sample per
 * thread, a fixed block of every dW per thread summed in sample order in blocks of 16, one slab per workgroup in
 * `workspace`, a last kernel adding the slabs in workgroup order in float64.  The actor's kernel holds a head of 8
 * outputs (two transposed halves of four) and computes the n_act gradients of log_std as column sums like the head's
 * bias gradients; the critic's launch is carl_ppo_grad's own kernel.  No floating-point atomics: the same call twice
 * gives the same bits.
 * Validation, each CARL_ERR_INVALID_ARGUMENT with a message of its own before anything is enqueued, in this order: a NULL
 * struct; a classic-control family; n_lanes < 1 or n_steps < 1; a row_pitch that is neither 0 nor n_lanes; a model table
 * out of range; obs_dim against the model; more than 8 actuators; the actor as carl_brax_rollout_policy_valued checks it
 * (hidden layers, n_ctx, n_ctx + obs_dim <= CARL_POLICY_MAX_IN, context rows -- a carl_ppo_batch_t does not say which rows
 * its producer made visible, so only their sign is checked --, n_in == n_ctx + obs_dim, n_out == n_act, a Box head, the
 * activation, n_sets == 1, params); the critic likewise with one output, then its n_ctx and context rows against the
 * actor's; the action dtype; n_contexts < 1 or ctx_stride < n_contexts; n_steps * n_lanes >= 2^31; n_samples < 1,
 * n_samples > n_steps * n_lanes, or idx NULL with n_samples != n_steps * n_lanes; clip_range / vf_coef / ent_coef negative
 * or not finite; a NULL required pointer of ppo; of out; log_std or out->grad_log_std NULL; workspace NULL, off a 16-byte
 * boundary or smaller than carl_brax_ppo_workspace_floats().
 * Stream-ordered and capturable; never synchronises with the host; allocates nothing.
 * Out of scope: Humanoid-size inputs, more than 8 actuators, several weight sets. */
int32_t carl_brax_ppo_tile(void);                          /* samples of one tile (256) */
int32_t carl_brax_ppo_grad_workgroups(int32_t n_samples);  /* workgroups of a launch: min(tiles, 256); 0 for n_samples < 1 */
/* floats of the workspace for these shapes and n_samples; -1 for an invalid shape (an actor with more than 8 outputs, a
 * critic with more than one) or n_samples < 1 */
int64_t carl_brax_ppo_workspace_floats(const carl_policy_t* policy_host, const carl_policy_t* critic_host, int32_t n_samples);
int carl_brax_ppo_grad(const carl_ppo_batch_t* ppo_host, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                       const carl_policy_t* critic_host, const float* log_std /* DEVICE [n_act] */,
                       const carl_ppo_out_t* out, void* stream);
/* carl_ppo_input_stats for a Brax buffer: the same kernel, sums, slabs (carl_ppo_input_stats_slabs) and validation list,
 * with `ppo` read with Brax meanings -- family is not a classic one (a classic one is refused; carl_ppo_input_stats
 * refuses a Brax one), rows are dense (row_pitch 0 or n_lanes), obs_dim up to CARL_POLICY_MAX_IN - n_ctx, a context row is
 * checked for its sign alone -- and the packing rule of the Brax families (carl_brax_policy_set_floats()).  Its slabs
 * are merged by carl_brax_policy_stats_merge.  carl_ppo_return_stats and carl_ppo_return_merge serve both. */
int carl_brax_ppo_input_stats(const carl_ppo_batch_t* ppo_host, const carl_policy_t* policy_host,
                              const carl_policy_stats_t* stats, void* stream);
/* The shape carl_brax_rollout_policy, carl_brax_rollout_policy_sampled and carl_brax_rollout_policy_valued launch for this
 * batch, model and step count (host only, no device access beyond the
 * compute-unit count of the current device; 256 where there is none): with n_groups = ceil(n_lanes / (64 / lanes_per_env))
 * it is what carl_brax_fragment_plan takes. */
typedef struct carl_brax_launch_shape {
  int32_t grid;                /* workgroups */
  int32_t waves_per_workgroup; /* wavefronts per workgroup */
  int32_t lanes_per_env;       /* lanes that share an env (64 / lanes_per_env envs per wavefront) */
  int32_t reserved;
  int64_t lds_bytes;           /* dynamic LDS per workgroup */
} carl_brax_launch_shape_t;
int carl_brax_policy_launch_shape(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, const carl_policy_t* policy_host,
                                  int32_t n_steps, carl_brax_launch_shape_t* out);
/* The same for the launches of carl_brax_reset (step == 0; n_steps ignored), carl_brax_step (step != 0, n_steps == 1) and
 * carl_brax_rollout (step != 0): the closed-loop launch of the same batch has the same lanes_per_env, and each wavefront's
 * slice of lds_bytes is larger by the policy's rows alone. */
int carl_brax_launch_shape(const carl_batch_t* batch, const carl_brax_sys_t* sys_host, int32_t step, int32_t n_steps,
                           carl_brax_launch_shape_t* out);

/* ======================= context sets on the device =======================
 * Replaces ContextSampler.sample_contexts (carl/context/sampler.py:45-61: per-feature draws from
 * the distributions, defaults filled for every other feature) and ContextSpace.verify_context
 * (carl/context/context_space.py:54-59) for dense context sets: the [F][C] table the step kernels
 * read is produced (and bounds-checked) in HBM instead of as C Python dicts.
 * Draws are Philox4x32-10 keyed (seed; global context id, feature index, attempt): a pure function
 * of (seed, context id, feature) -- independent of sharding -- and NOT the reference's NumPy
 * MT19937 stream (carl_amd.context.sampler reproduces that one on the host, pinned by the
 * reference's notebook outputs; this entry point is the one that scales).
 *   CONSTANT       value                                   (features without a distribution: default)
 *   UNIFORM_FLOAT  fma(upper - lower, u, lower); log_scale: exp of the same between the logs
 *   NORMAL_FLOAT   mu + sigma * z (Box-Muller), redrawn while outside [lower, upper] (<= 32 times,
 *                  then clipped) -- ConfigSpace NormalFloat with bounds
 *   UNIFORM_INT    lower + floor(u * (upper - lower + 1))
 *   CATEGORICAL    choices[floor(u * n_choices)] (numeric choices, e.g. Brax target_direction) */
#define CARL_MAX_CHOICES 32
typedef enum {
  CARL_FEAT_CONSTANT = 0,
  CARL_FEAT_UNIFORM_FLOAT = 1,
  CARL_FEAT_NORMAL_FLOAT = 2,
  CARL_FEAT_UNIFORM_INT = 3,
  CARL_FEAT_CATEGORICAL = 4
} carl_feature_kind_t;

typedef struct {
  int32_t kind;       /* carl_feature_kind_t */
  int32_t n_choices;  /* CATEGORICAL */
  int32_t log_scale;  /* UNIFORM_FLOAT */
  int32_t reserved;
  float lower, upper; /* bounds: sampling range and carl_verify_contexts (+-inf allowed) */
  float mu, sigma;    /* NORMAL_FLOAT */
  float value;        /* CONSTANT */
  float reserved_f;
  float choices[CARL_MAX_CHOICES];
} carl_feature_spec_t;

/* ctx_table[f * ctx_stride + c] for c in [0, n_contexts), f in [0, n_features); context c is the
 * global context `context_offset + c`.  specs_dev / specs_host: the same n_features specs on the
 * device and on the host (validation). */
int carl_sample_contexts(const carl_feature_spec_t* specs_dev, const carl_feature_spec_t* specs_host,
                         int32_t n_features, int32_t n_contexts, int32_t ctx_stride, int64_t context_offset,
                         uint64_t seed, float* ctx_table, void* stream);
/* n_bad_out[0] (device int32) = number of table entries outside their feature's bounds (or not one
 * of a categorical feature's choices, or NaN) */
int carl_verify_contexts(const carl_feature_spec_t* specs_dev, const carl_feature_spec_t* specs_host,
                         int32_t n_features, int32_t n_contexts, int32_t ctx_stride, const float* ctx_table,
                         int32_t* n_bad_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CARL_AMD_H_ */
