/*
 * nfsp.h -- C ABI of libnfsp, the MI355X (gfx950) NFSP-on-Leduc self-play engine.
 *
 * The reference (dantodor/Neural-Ficititious-Self-Play-in-Imperfect-Information-Games)
 * has no FFI: its boundary is the duck-typed Python object API that main.train calls
 * (SURVEY.md §8b).  Every entry point below replaces one of those Python methods, in
 * batched form (n envs / n records per call); the file:line it replaces is cited.
 * The Python host side (the package's leduc.py / agent.py / buffers.py) binds these
 * with ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - Every function returns an int status: NFSP_OK (0) or a negative NFSP_E* code;
 *     nfsp_last_error() returns a thread-local message for the last failure.
 *     Game-level misuse is NOT an error, mirroring the reference, which never raises:
 *     illegal raises are remapped (leduc/newenv.py:141-145) and a step after the hand
 *     ended only updates env.s[p] and counts a warning (leduc/newenv.py:346-348).
 *   - Pointers named dev_* are device (HBM) pointers, e.g. torch.Tensor.data_ptr() of a
 *     cuda tensor; everything else is host memory.  Outputs are caller-owned; the ctx
 *     owns env state and its workspaces.
 *   - All work is enqueued on the ctx's stream (default: the null stream; see
 *     nfsp_set_stream) and is asynchronous unless the function says otherwise.
 *   - A ctx is not thread-safe (the reference is single-threaded with one env shared
 *     by both agents, agent/agent.py:28).
 *   - Layouts: observations are float32 [n,30] (24 history bits + 2x3 card bits, values
 *     0/1, leduc/newenv.py:53,118), action vectors float32 [n,3], rewards float32.
 *     Network weights are float32, packed W1[30][H] | b1[H] | W2[H][3] | b2[3]
 *     (= Keras get_weights() order, flattened), H = hidden width (config HiddenLayer).
 */
#ifndef NFSP_H
#define NFSP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFSP_OK 0
#define NFSP_EINVAL (-1)   /* bad argument (null pointer, size, unsupported width) */
#define NFSP_EHIP (-2)     /* a HIP runtime call failed (message has the HIP error) */
#define NFSP_ENOMEM (-3)

#define NFSP_GAME_LEDUC 0
/* Kuhn swap-in (BASELINE config C5): the same 30-bit observation layout (history bits of
 * round 0, card one-hot at bit 24 + rank), 3 distinct ranks (0 best), antes 1 / 1, one
 * betting round with at most one bet (further raises remap to call), showdown by rank. */
#define NFSP_GAME_KUHN 1

/* MLP output activation / loss (agent/agent.py:103,106,112,115) */
#define NFSP_ACT_RELU 0        /* BR / target-BR head, Huber loss */
#define NFSP_ACT_SOFTMAX 1     /* AR head, categorical cross-entropy */
#define NFSP_ACT_LINEAR 2      /* BR head under NFSP_EXT_LINEAR_Q (the engine, nfsp_mlp_forward and
                                  nfsp_head_tables; no nfsp_mlp_fit) */

/* Reference quirks, reproduced by default (SURVEY.md §7 hard part (b)). */
#define NFSP_QUIRK_TERMINAL_BOOTSTRAP 1u  /* `t_batch[k] is True` never holds: terminal
                                             transitions bootstrap (agent/agent.py:227) */
#define NFSP_QUIRK_ROW0_TARGET 2u         /* TD targets overwrite row 0 only
                                             (agent/agent.py:240-241) */
#define NFSP_QUIRK_ALIAS_RL 4u            /* stored (s, a) of an RL tuple are views of
                                             env.s[p] / env.last_action[p]: every tuple of a
                                             hand ends up with p's LAST pre-action s and a
                                             (utils/replay_buffer.py:30-41 + newenv.py:119) */
#define NFSP_QUIRKS_REFERENCE 7u
/* Textbook-NFSP extensions of the batched engine (Heinrich & Silver 2016), in the same
 * cfg.quirks word.  NOT the reference's algorithm -- NFSP_QUIRKS_REFERENCE leaves them off.
 * They let the same engine run NFSP proper, e.g. for C5's exploitability -> 0 check
 * (DESIGN.md §9); quirks = NFSP_TEXTBOOK is that algorithm with every reference quirk off. */
#define NFSP_EXT_SL_ONEHOT 8u     /* M_SL stores one-hot(argmax) of the BR action, not its raw
                                     vector (the reference: agent/agent.py:147-151) */
#define NFSP_EXT_RESERVOIR 16u    /* M_SL is a true reservoir (Algorithm R): the k-th insert
                                     (k >= N, 0-based) takes slot j = U{0..k} iff j < N (the
                                     reference: utils/ReservoirBuffer.py:22-28) */
#define NFSP_EXT_LINEAR_Q 32u     /* BR / target nets with a linear Q head (the reference's is
                                     ReLU, agent/agent.py:103); Huber on the linear outputs */
#define NFSP_EXT_EPS_CONST 64u    /* eps stays at cfg.epsilon (the reference: eps / iteration
                                     after each BR update, agent/agent.py:253, which ends
                                     exploration within a few updates) */
#define NFSP_EXT_SAMPLE_AR 128u   /* an agent acting with its average policy samples the action
                                     from the AR softmax (Philox counter (lane, hand, 2^31 + k)
                                     for its k-th AR decision) and passes the one-hot vector:
                                     the reference passes the softmax itself, which the env
                                     executes as its argmax (agent/agent.py:143, newenv.py:135) */
#define NFSP_EXT_MSE_Q 256u       /* with NFSP_EXT_LINEAR_Q: the BR / target nets are fitted with
                                     mean squared error, not the reference's Huber loss
                                     (agent/agent.py:91-99).  Huber's clipped gradient makes Q a
                                     robust location estimate (between median and mean), so with
                                     bimodal returns (a +-2 showdown) Q(s, a) sits up to ~1 chip from
                                     the expected return and the greedy "best response" is not one
                                     (tests/studies/kuhn_diag.py).  Requires LINEAR_Q. */
#define NFSP_TEXTBOOK (NFSP_EXT_SL_ONEHOT | NFSP_EXT_RESERVOIR | NFSP_EXT_LINEAR_Q | \
                       NFSP_EXT_EPS_CONST | NFSP_EXT_SAMPLE_AR)
/* NFSP_TEXTBOOK with the expected-return (MSE) Q loss: NFSP as Heinrich & Silver train it */
#define NFSP_TEXTBOOK_MSE (NFSP_TEXTBOOK | NFSP_EXT_MSE_Q)
/* ... with epsilon decaying as the reference's (eps / iteration) instead of NFSP_EXT_EPS_CONST.
 * With SL_ONEHOT, a constant 0.06 stores argmax(rand(3)) -- a uniform action -- for 6 % of the
 * BR decisions, which mixes uniform play into the average policy: Kuhn's exploitability then
 * stops at 0.06-0.09 chips whatever the learning rates; decaying, it reaches 0.01-0.02
 * (profiles/r06/kuhn_*.jsonl). */
#define NFSP_TEXTBOOK_MSE_DECAY (NFSP_TEXTBOOK_MSE & ~NFSP_EXT_EPS_CONST)

typedef struct nfsp_ctx nfsp_ctx;

/* Record columns of an M_RL (utils/replay_buffer.py:30-41) or M_SL
 * (utils/ReservoirBuffer.py:18-28) memory; all device pointers, rows contiguous.
 * M_SL uses s and a only (r, s2, t = NULL). */
typedef struct nfsp_records {
  float* s;     /* [cap, 30] */
  float* a;     /* [cap, 3]  */
  float* r;     /* [cap]     */
  float* s2;    /* [cap, 30] */
  uint8_t* t;   /* [cap]     */
  int64_t cap;
} nfsp_records;

/* ---------------------------------------------------------------- lifecycle */
const char* nfsp_last_error(void);
int nfsp_version(void);
int nfsp_device_count(int* out);

/* Creates a ctx holding n_envs Leduc hands on HIP device `device`.
 * Replaces leduc/newenv.py:14-57 (Env.__init__), batched. */
int nfsp_create(nfsp_ctx** out, int n_envs, uint64_t seed, int game, int device);
int nfsp_destroy(nfsp_ctx* ctx);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream), 0 = null stream */
int nfsp_set_stream(nfsp_ctx* ctx, void* hip_stream);
int nfsp_synchronize(nfsp_ctx* ctx);
int nfsp_num_envs(const nfsp_ctx* ctx);

/* ---------------------------------------------------------------- env (batched newenv API) */
/* Stores deals (P0, P1, public rank; rank 0 = Ace is best) for the NEXT nfsp_env_reset.
 * Test/host injection of the deck (the reference shuffles the global `random`,
 * leduc/deck.py:42-50; the Python drop-in shuffles there and injects the result).
 * This is how the deal modes of SURVEY §8(b) reach the device.  PHILOX is
 * nfsp_env_reset's own draw.  PY3_MT and PY2_MT are CPython 3 / 2.7 shuffles of the
 * host's MT19937 stream (nfsp_amd.pyrandom.set_python_semantics(3 | 2)), drawn on the host
 * and injected here. */
int nfsp_env_set_deal(nfsp_ctx* ctx, const uint8_t* dev_ranks /* [n,3] */);
/* Deal modes (SURVEY §8(b) deal_mode) of nfsp_env_reset.  The reference reshuffles a fresh
 * 6-card deck with the global `random` at every Env.reset (leduc/deck.py:42-44) and pops
 * P0, P1 and the public card from its end.
 *   PHILOX  (default): the device draw keyed by (ctx seed, env, reset index);
 *   PY3_MT / PY2_MT:   that shuffle on the host, under CPython 3's / 2.7's random seeded
 *                      with random.seed(seed).  Every reset deals env 0, 1, ..., n-1 from
 *                      the one stream, and the deck is its only consumer.  The drop-in
 *                      Python Env shares the process's global random with the rest of
 *                      main.train instead (nfsp_amd.pyrandom).  Leduc only.
 * A pending nfsp_env_set_deal still takes precedence for the next reset. */
#define NFSP_DEAL_PHILOX 0
#define NFSP_DEAL_PY3_MT 1
#define NFSP_DEAL_PY2_MT 2
int nfsp_env_set_deal_mode(nfsp_ctx* ctx, int mode, uint64_t seed);
/* Host only (no device work): the first n deals (P0, P1, public rank) of deal mode PY3_MT or
 * PY2_MT from random.seed(seed), as nfsp_env_reset would draw them for n consecutive resets
 * of a 1-env ctx. */
int nfsp_deal_mt(int mode, uint64_t seed, int64_t n, uint8_t* out /* [n,3] */);
/* Env.reset(dealer) (leduc/newenv.py:76-114) for every env.  Deal = the pending
 * nfsp_env_set_deal if any, else a Philox draw keyed by (seed, env, reset index). */
int nfsp_env_reset(nfsp_ctx* ctx, const uint8_t* dev_dealer /* [n] */);
/* Env.get_state(p) (leduc/newenv.py:116-129).  Player = dev_players[i] if non-null, else p.
 * Any output may be NULL.  s = env.s[p] (obs recorded by p's last step), a =
 * env.last_action[p], r = reward if terminated else 0, s2 = current obs, t = terminated. */
int nfsp_env_get_state(nfsp_ctx* ctx, int p, const uint8_t* dev_players,
                       float* dev_s /*[n,30]*/, float* dev_a /*[n,3]*/, float* dev_r /*[n]*/,
                       float* dev_s2 /*[n,30]*/, uint8_t* dev_t /*[n]*/);
/* Env.step(action, p) (leduc/newenv.py:192-349).  Envs with dev_mask[i] == 0 are left
 * untouched (dev_mask may be NULL = all). */
int nfsp_env_step(nfsp_ctx* ctx, const float* dev_action /*[n,3]*/, int p,
                  const uint8_t* dev_players, const uint8_t* dev_mask);
/* Env.do_action(action, p) (leduc/newenv.py:131-178) alone: argmax, last_action, the
 * illegal-raise remap, then the action recorded (history, pot, actions_done; a fold too).
 * No round change, termination or reward (those are step()'s).  dev_fold[i] = its return
 * value (1 on a fold); dev_fold may be NULL. */
int nfsp_env_do_action(nfsp_ctx* ctx, const float* dev_action /*[n,3]*/, int p,
                       const uint8_t* dev_players, const uint8_t* dev_mask, uint8_t* dev_fold /*[n]*/);
/* Env.game_or_round_has_terminated() (leduc/newenv.py:180-190) on each env's actions_done:
 * 1 = True ([C,C] [R,C] [C,R,C] [R,R,C]), 0 = False (length other than 2 or 3),
 * -1 = None (the reference's fall-through for other length-2 / -3 sequences). */
int nfsp_env_round_status(nfsp_ctx* ctx, int8_t* dev_out /*[n]*/);
/* Env.round_index (leduc/newenv.py:59-61) */
int nfsp_env_round(nfsp_ctx* ctx, uint8_t* dev_round /*[n]*/);
/* Debug/introspection: the 64-byte per-env state (layout nfsp_device.h `Hand`). */
int nfsp_env_export(nfsp_ctx* ctx, void* dev_out /*[n,64] bytes*/);

/* ---------------------------------------------------------------- networks */
/* model.predict(x) (agent/agent.py:126,143,219,230) for B rows; bit-identical to the
 * oracle's fixed summation order for 0/1 inputs.  act: any NFSP_ACT_*; LINEAR is the ReLU head's
 * sums without the output activation. */
int nfsp_mlp_forward(nfsp_ctx* ctx, const float* dev_w, int hidden, int act,
                     const float* dev_x /*[B,30]*/, float* dev_y /*[B,3]*/, int64_t B);
/* model.fit(x, y, epochs, batch_size) with plain SGD (agent/agent.py:243,261): for each
 * epoch, rows dev_perm[e*n .. e*n+n) in slices of batch_size, one SGD step per slice.
 * act selects the loss (RELU -> Huber, SOFTMAX -> categorical cross-entropy).
 * Weights are updated in place.  batch_size <= 64, hidden == 64. */
int nfsp_mlp_fit(nfsp_ctx* ctx, float* dev_w, int hidden, int act,
                 const float* dev_x /*[n,30]*/, const float* dev_t /*[n,3]*/, int n,
                 const int32_t* dev_perm /*[epochs,n]*/, int epochs, int batch_size, float lr);
/* The TD-target construction of update_best_response_network (agent/agent.py:219-241):
 * target = Q_target(s); v_k = r_k + gamma * max Q_target(s2_k) (or r_k if terminal and the
 * TERMINAL_BOOTSTRAP quirk is off); expl = mean_k max target[k] (agent/agent.py:235-238,
 * before the overwrite); then target[row][argmax a_k] = v_k with row = 0 under
 * ROW0_TARGET (sequential, last k wins) else k.  dev_expl: one float64. */
int nfsp_br_targets(nfsp_ctx* ctx, const float* dev_target_w, int hidden,
                    const float* dev_s, const float* dev_a, const float* dev_r,
                    const float* dev_s2, const uint8_t* dev_t, int n, double gamma,
                    unsigned quirks, float* dev_target_out /*[n,3]*/, double* dev_expl);

/* ---------------------------------------------------------------- memories */
/* ReplayBuffer.add / ReservoirBuffer.add (utils/replay_buffer.py:30-41,
 * utils/ReservoirBuffer.py:18-28): copy n records src[i] -> dst[dev_slots[i]].  The slot
 * policy (FIFO head, reservoir j) is the caller's; duplicate slots: last i wins, for every
 * n and whatever the order the device works in (the result is the sequential loop's).  Only
 * the columns that are non-NULL in both tables are copied.  A record whose slot lies outside
 * [0, dst->cap) is skipped: nothing is read or written for it.  NFSP_EINVAL, with nothing
 * launched: a NULL argument, n < 0, dst->cap <= 0 or src->cap <= 0, n > src->cap.  n == 0
 * succeeds and launches nothing.  The ctx keeps one word per row of the largest dst seen. */
int nfsp_buf_insert(nfsp_ctx* ctx, const nfsp_records* dst, const nfsp_records* src,
                    const int64_t* dev_slots, int64_t n);
/* sample_batch (utils/replay_buffer.py:46-59, utils/ReservoirBuffer.py:33-43): gather
 * dst[i] = src[dev_idx[i]] for i < k (columns that are NULL in dst or in src are skipped;
 * indices may repeat).  A row whose index lies outside [0, src->cap) is skipped: nothing is
 * read, and dst[i] keeps what it held.  NFSP_EINVAL, with nothing launched: a NULL argument,
 * k < 0, dst->cap <= 0 or src->cap <= 0, k > dst->cap.  k == 0 succeeds and launches nothing. */
int nfsp_buf_sample(nfsp_ctx* ctx, const nfsp_records* src, const int64_t* dev_idx,
                    int64_t k, const nfsp_records* dst);

/* ---------------------------------------------------------------- batched self-play engine
 * The fused hot path (SURVEY.md §8a rows a1-a18 at scale): n_lanes concurrent hands,
 * one hand per lane per nfsp_rollout, both agents' memories and networks on device.
 *
 *   nfsp_rollout       main.train's hand loop (main.py:27-67) x n_lanes in ONE kernel:
 *                      deal (deck.py), eta draws, D/L/D scheduler, Agent.play
 *                      (agent/agent.py:130-156) with the AR / eps-greedy BR forwards,
 *                      env.step; then the RL/SL records are committed in canonical
 *                      order (lane, then play order) to the agents' memories.
 *   nfsp_engine_update the learner for the inserts of the last rollout: update_strategy
 *                      once per `inserts_per_update` RL inserts of an agent (the
 *                      reference's game_step % 128 trigger), each one =
 *                      update_avg_response_network + update_best_response_network with
 *                      the reference schedules; M_SL inserts are applied in stream order
 *                      between the AR updates they precede.
 * Randomness: Philox4x32-10 keyed by cfg.seed; counters (lane, hand, draw) for the
 * rollout and (agent, update, row) for the learner -- results do not depend on
 * scheduling.  Deviation from the sequential reference (declared): all hands of one
 * rollout act with the weights and epsilon at its start (policy lag <= one rollout);
 * repeated triggers while game_step stays on a multiple of 128 are not replayed. */
typedef struct nfsp_engine nfsp_engine;

typedef struct nfsp_engine_cfg {
  int32_t n_lanes;             /* hands in flight */
  int32_t hidden;              /* [Agent] HiddenLayer, must be 64 */
  int64_t rl_capacity;         /* M_RL size (reference: [Utils] Buffersize 40000) */
  int64_t sl_capacity;         /* M_SL size (reference: 40000); < 2^31 */
  int32_t batch;               /* [Agent] MiniBatchSize 128 */
  int32_t inserts_per_update;  /* 128: game_step % 128 (agent/agent.py:153) */
  int32_t target_every;        /* [Agent] TargetModelUpdateRate 150 */
  int32_t epochs;              /* fit epochs, 2 (agent/agent.py:243,261) */
  int32_t fit_batch;           /* Keras default batch_size 32 */
  uint32_t quirks;             /* NFSP_QUIRKS_REFERENCE */
  float eta, lr_br, lr_ar;     /* 0.1, 0.05, 0.1 */
  double gamma, epsilon;       /* 0.95, 0.06 */
  uint64_t seed;
  /* Lane slices (1 = off).  The n_lanes envs are advanced in `slices` equal slices of
   * n_lanes / slices lanes: nfsp_rollout plays one hand on every lane of the next slice, and
   * nfsp_engine_step = `slices` x (nfsp_rollout + nfsp_engine_update), i.e. one hand per lane
   * of all n_lanes, with the learner consuming each slice's inserts before the next slice
   * acts.  That bounds the declared policy lag by one slice instead of all n_lanes hands
   * (the reference has none: main.py:27-67 learns inside the hand loop,
   * agent/agent.py:153-154).  Philox counters and the dealer use the global lane id
   * (slice * n_lanes / slices + lane) and the lane's hand count (rollouts / slices), so a
   * lane's hand does not depend on the slicing.  Staging and learner buffers are sized for
   * one slice.  n_lanes must be a multiple of slices. */
  int32_t slices;
  /* Slice lag inside nfsp_engine_step (slices > 1): 1 = the learner of slice k completes
   * before slice k + 1 acts; 2 = pipelined: slice k + 1's rollout (and the host's plan and the
   * prep kernels of its learner) run while slice k's SGD chains do, so slice k + 1 acts with
   * the nets and epsilon as of the end of slice k - 1's learner (the first two slices of a step:
   * as of the step's start).  The policy lag is then two slices; the chains' streams never
   * wait for a rollout.  Each step starts from the nets as they are (nfsp_engine_weights
   * writes between steps are seen) and ends with every stream joined.  nfsp_rollout /
   * nfsp_engine_update called by themselves always run with lag 1.  Engine groups run their
   * slices one after another, and with slice_lag 2 each replica's slice j acts with the nets
   * and epsilon its learner left after slice j - 2 (snapshots on device): the same arithmetic
   * as a pipelined engine, not its overlap. */
  int32_t slice_lag;
  /* Scheduling flags (NFSP_SCHED_*; they change only the order of launches, never a result).
   * nfsp_engine_default_cfg takes them from the environment (NFSP_LEARNER_SERIAL=1), read at
   * that call; 0 = the production schedule. */
  uint32_t sched;
} nfsp_engine_cfg;
/* diagnostic: an engine's BR work waits for its AR chains, to time each alone */
#define NFSP_SCHED_LEARNER_SERIAL 1u

typedef struct nfsp_engine_stats {
  int64_t hands, rollouts;
  int64_t rl_total[2], sl_total[2];     /* inserts ever, per agent */
  int64_t rl_size[2], sl_size[2];       /* memory sizes (ReplayBuffer/ReservoirBuffer.size);
                                         * sl_size counts the reservoir rows as stored: a
                                         * rollout's SL inserts (in sl_total) are applied to
                                         * them by nfsp_engine_update */
  int64_t last_rl[2], last_sl[2];       /* inserts of the last rollout */
  int64_t br_updates[2], ar_updates[2];
  int64_t iteration[2], target_syncs[2];
  int64_t actions[2][3];                /* Agent.actions counters (agent/agent.py:155) */
  double reward[2];                     /* Agent.reward */
  double epsilon[2], temp[2], lr_br[2];
  double exploitability[2];             /* last BR update's proxy (agent/agent.py:235-238) */
} nfsp_engine_stats;

int nfsp_engine_default_cfg(nfsp_engine_cfg* out);
int nfsp_engine_create(nfsp_ctx* ctx, const nfsp_engine_cfg* cfg, nfsp_engine** out);
int nfsp_engine_destroy(nfsp_engine* e);
/* Device pointer to the packed weights of agent (0|1), net (0 = AR avg_strategy_model,
 * 1 = BR best_response_model, 2 = target_br_model); read or write them in place. */
int nfsp_engine_weights(nfsp_engine* e, int agent, int net, float** dev_w);
int nfsp_rollout(nfsp_engine* e);
/* Test hook: nfsp_rollout acting with the given nets (device [2 agents][3 nets][NP], the
 * target slots unused) and epsilons instead of the engine's -- what a pipelined slice does
 * with its snapshot (cfg.slice_lag 2); lets a test drive a lag-1 engine through the same
 * schedule and compare. */
int nfsp_rollout_with(nfsp_engine* e, const float* dev_w, const double* eps /*[2]*/);
int nfsp_engine_update(nfsp_engine* e);
int nfsp_engine_step(nfsp_engine* e);          /* nfsp_rollout + nfsp_engine_update */
/* After a non-OK return from nfsp_rollout / nfsp_engine_update / nfsp_engine_step the
 * engine's state is unspecified: part of the step's work may have run.  Destroy the
 * engine (nfsp_engine_destroy waits for all of its streams). */
int nfsp_engine_get_stats(nfsp_engine* e, nfsp_engine_stats* out);   /* synchronises */
/* Agent's memories in the reference's fp32 tuple layout (utils/replay_buffer.py:53-57),
 * expanded on the ctx stream at the call from the packed device records (M_RL: 32 B
 * {s bits, s2 bits, argmax|t|r, a[3]}, M_SL: 16 B {bits, a[3]}; the export buffers are
 * allocated on first use).  M_RL is a circular log of rl_log_cap rows whose record k
 * (k-th insert ever) sits at row k % rl_log_cap; the logical M_RL is the last
 * min(rl_total, rl_capacity) records.  sl: the reservoir (rows [0, sl_size)).
 * pending_sl (live views): the last rollout's M_SL records not yet applied by
 * nfsp_engine_update, in insert order, with rl_pos = the agent's RL insert count when each
 * was made. */
int nfsp_engine_memories(nfsp_engine* e, int agent, nfsp_records* rl, int64_t* rl_log_cap,
                         nfsp_records* sl, uint32_t** dev_pending_sl_obs,
                         float** dev_pending_sl_a, int64_t** dev_pending_sl_rl_pos);
/* Per-kernel timing with HIP events recorded around each launch on the stream it runs on:
 * ms / launches [11] = {k_rollout, k_scan1+k_scan2, k_commit, learner (whole
 * nfsp_engine_update), learner prep (k_br_prep..k_res_apply), k_br_targets,
 * k_chain3<BR>, k_chain3<AR>, BR stream of agent 0, BR stream of agent 1, the AR exchange
 * (nfsp_engine_set_exchange: delta, all-reduce, apply on the AR stream)}, accumulated since
 * the previous nfsp_engine_get_timings (which synchronises and resets them).  A "BR stream"
 * entry is the span of one learner call's BR work of that agent on its stream, from its
 * first k_br_targets to its last chain, gaps included (engine groups: their one BR stream in
 * slot 8) -- with k_chain3<AR> (one launch per call, both agents), the per-stream critical
 * path of the learner. */
int nfsp_engine_set_timing(nfsp_engine* e, int on);
/* Loss log (observability; the reference's TensorBoard callbacks on fit, agent/agent.py:
 * 84-88,243,264): when on, the SGD chains also record each update's Keras epoch losses
 * (BR: the py2 huber_loss of agent/agent.py:91-99, where 1 / 2 == 0; AR: categorical
 * cross-entropy), each minibatch's loss taken before its step.  nfsp_engine_losses gives, per
 * agent a and net n (0 = AR, 1 = BR), out[(2a + n) * 2 + 0] = the mean epoch loss over the last
 * nfsp_engine_update's updates and [.. + 1] = its last update's final-epoch loss (NaN: none). */
int nfsp_engine_set_loss_log(nfsp_engine* e, int on);
int nfsp_engine_losses(nfsp_engine* e, double* out /*[2][2][2]*/);
#define NFSP_TIMING_SLOTS 11
int nfsp_engine_get_timings(nfsp_engine* e, double* ms /*[NFSP_TIMING_SLOTS]*/,
                            int64_t* launches /*[NFSP_TIMING_SLOTS]*/);
/* Debug view of the last learner run: per agent and role (0 = AR, 1 = BR) the sampled
 * rows [batch] (int64) and fit permutations [epochs][batch] (int32) of its LAST update. */
int nfsp_engine_last_update(nfsp_engine* e, int agent, int role, int64_t** dev_rows,
                            int32_t** dev_perms);
/* Debug view of the last rollout's per-lane record counts [n_lanes / slices] (uint32, device;
 * local lane i of the slice that rollout played is global lane slice * n_lanes / slices + i):
 * rl0 | rl1 << 4 | sl0 << 8 | sl1 << 12 (RL / SL inserts of agents 0 and 1 by that lane's
 * hand).  Their exclusive prefix over lanes is each lane's first record in the canonical
 * insert order (lane, then play order) -- how a test finds one lane's records in M_RL. */
int nfsp_engine_lane_counts(nfsp_engine* e, uint32_t** dev_counts);

/* Debug view (cfg.slice_lag 2): the acting nets [2 agents][3 nets][NP] (target slots unused)
 * and epsilons of snapshot `parity` -- after a pipelined nfsp_engine_step of K slices, snapshot
 * (K - 1) & 1 holds what the step's last slice acted with. */
int nfsp_engine_snapshot(nfsp_engine* e, int parity, float** dev_w, double* eps /*[2]*/);

/* ---- cross-shard exchange of the average-policy nets (BASELINE C4) ----
 * The reference learns inside its hand loop (main.py:27-67; update_strategy every 128 RL
 * inserts, agent/agent.py:153-154, whose AR fit is agent/agent.py:255-264).  Sharded over N
 * GPUs, each shard's learner trains its own copy of both agents' AR nets; the exchange keeps
 * the copies one net: at the end of every `every`-th learner call (one call per lane slice:
 * every = 1 exchanges after every slice, every = cfg.slices once per step), right behind the
 * call's AR chain on the chain's own stream,
 *     D = W_AR - W0   (both agents, 2 x NP f32),   S = sum over shards of D,
 *     W_AR = W0 + S * scale,   W0 = W_AR
 * (scale 1 / N: the mean of the shards' gradient steps, i.e. data-parallel SGD of one net
 * over every shard's minibatches, exchanged per slice).  Before the AR snapshot of a
 * pipelined slice (cfg.slice_lag 2), so the rollout two slices on acts with the exchanged
 * nets.  Arithmetic: fp contract off, S summed from +0 -- with 2 shards bit-identical to an
 * engine group's on-device exchange (NFSP_GROUP_AVG_AR, nfsp_group_set_exchange).
 * Transports (exactly one):
 *   rccl_comm  an RCCL communicator (nfsp_rccl_comm_create): ncclAllReduce(SUM) of D in place
 *              on the AR chain stream -- stream-ordered, no host round trip;
 *   fn         a host callback, for transports that are not stream-ordered (gloo rehearsals
 *              and CPU-side tests): the engine synchronises the AR stream, calls
 *              fn(user, dev_D, 2 * NP), which must leave S in dev_D (device memory, complete
 *              on return) and return 0; anything else fails the step.
 * Every shard must make the same number of learner calls (the same slices per step).
 * nfsp_engine_set_exchange takes W0 = the AR nets as they are now (call it after the shards'
 * AR nets were made equal, e.g. broadcast from rank 0); every = 0 turns the exchange off. */
typedef int (*nfsp_exchange_fn)(void* user, float* dev_sum, int64_t n);
int nfsp_engine_set_exchange(nfsp_engine* e, int every, float scale, void* rccl_comm,
                             nfsp_exchange_fn fn, void* user);
/* exchanges made so far */
int nfsp_engine_exchanges(nfsp_engine* e, int64_t* out);
/* RCCL (librccl.so.1, loaded on first use): ncclGetUniqueId into out[128] (rank 0), and a
 * communicator of `world` ranks on HIP device `device` from that id (every rank, collectively:
 * ncclCommInitRank blocks until all ranks joined).  nfsp_rccl_ready loads RCCL and selects
 * `device` without joining anything: every rank calls it and the ranks agree (an all-reduce
 * MIN of the results) BEFORE any of them calls nfsp_rccl_comm_create, so a rank that cannot
 * use RCCL never leaves the others blocked in ncclCommInitRank. */
int nfsp_rccl_ready(int device);
int nfsp_rccl_unique_id(uint8_t* out /*[128]*/);
int nfsp_rccl_comm_create(const uint8_t* id /*[128]*/, int world, int rank, int device, void** comm);
int nfsp_rccl_comm_destroy(void* comm);

/* Test hook: from the next nfsp_engine_update on, each agent's AR and BR chains run only the
 * first max_updates updates of the learner call (0 = all).  Everything else still follows
 * the full plan: the prep kernels, the reservoir, and the counters and schedules in the
 * stats.  A test compares the weights with an oracle replay of the same update prefix.  The
 * engine is not meant to train on after that. */
int nfsp_engine_set_update_limit(nfsp_engine* e, int64_t max_updates);

/* ---- engine groups: several learners on one GPU ----
 * A group holds R replicas of the engine.  Each replica is an independent
 * main.train (main.py:21-75) over cfg.n_lanes lanes: its own hands, its own M_RL / M_SL, and
 * its own nets.  Replica r uses cfg.seed + r, and is bit-identical to a standalone engine
 * created with that seed and stepped as often.  nfsp_group_step does rollout + update for
 * every replica.  The SGD chains of all replicas run in shared launches: one AR launch of 2R
 * workgroups; the BR chains in rounds of one targets launch and one chain launch.  Unsliced,
 * round k holds every (replica, agent)'s k-th target-sync segment; sliced (cfg.slices > 1),
 * the replicas are split into 2 halves with their own rounds on their own streams, and a
 * round's pieces are at most 40 updates, paced by the half's busiest job (nfsp_group_sched;
 * DESIGN.md 4.5).  A piece
 * resumes from the weights in memory, so the SGD steps are a standalone engine's.  A chain
 * workgroup occupies one CU, so one learner pair's 4 CUs become 4R.  This is BASELINE C4's
 * shard model inside one GPU.
 * With NFSP_GROUP_AVG_AR, replica 0's AR nets are first copied to every replica.  After every
 * step, each AR net becomes W0 + sum_r (W_r - W0) / R, with W0 = the nets after the
 * previous exchange.  This is shards.AvgPolicyAllReduce's per-step exchange, done on device.
 * A replica's handle (nfsp_group_engine) serves weights, stats, memories, the loss log and
 * timing; nfsp_engine_update / nfsp_engine_step on it are refused. */
typedef struct nfsp_group nfsp_group;
#define NFSP_GROUP_MAX_REPLICAS 256
#define NFSP_GROUP_AVG_AR 1u
int nfsp_group_create(nfsp_ctx* ctx, const nfsp_engine_cfg* cfg, int replicas, unsigned flags,
                      nfsp_group** out);
/* Heterogeneous groups: a hyperparameter sweep in one launch.  Replica r is an
 * independent main.train with cfgs[r] exactly as given (its seed is NOT offset by r),
 * bit-identical to a standalone engine created with cfgs[r] and stepped as often.
 *   May differ between replicas: seed, eta, lr_br, lr_ar, gamma, epsilon, target_every, and
 * quirks outside NFSP_EXT_LINEAR_Q | NFSP_EXT_MSE_Q.  Each reaches the shared launches through
 * the replica's own rows of their device tables (the rollout's and the prep kernels' arguments,
 * the BR targets' jobs, the schedules), never through a launch-wide argument.
 *   Must be equal: n_lanes, hidden, rl_capacity, sl_capacity, batch, inserts_per_update, epochs,
 * fit_batch, slices, slice_lag, sched -- the shapes of the shared launches and of the buffers
 * behind them -- and the quirk bits NFSP_EXT_LINEAR_Q and NFSP_EXT_MSE_Q, which select the BR
 * chain kernel of a shared launch.  A difference is NFSP_EINVAL; nfsp_last_error names the field
 * and the replica.  Two replicas with identical cfgs, seed included, are legal.
 *   A group is uniform when every replica's cfg equals replica 0's apart from the seed
 * (nfsp_group_create(cfg, R) = nfsp_group_create_v with cfgs[r] = *cfg, seed + r); otherwise
 * it is heterogeneous, and has no exchange: NFSP_GROUP_AVG_AR here, nfsp_group_set_exchange with
 * every > 0 and nfsp_group_average_ar are NFSP_EINVAL (an average of nets trained under
 * different hyperparameters is not a sweep).  With sched.br_persist, a group whose replicas
 * differ in gamma, lr_br or quirks keeps the BR rounds (k_br_persist takes one of each per
 * launch). */
int nfsp_group_create_v(nfsp_ctx* ctx, const nfsp_engine_cfg* cfgs /*[replicas]*/, int replicas,
                        unsigned flags, nfsp_group** out);
/* Host only, no device: would nfsp_group_create_v accept these?  NFSP_EINVAL, with
 * nfsp_last_error naming the first offending field and replica (also a cfg that
 * nfsp_engine_create would refuse, and NFSP_GROUP_AVG_AR in flags on a heterogeneous list). */
int nfsp_group_cfgs_check(const nfsp_engine_cfg* cfgs /*[replicas]*/, int replicas, unsigned flags);
/* Replica's cfg as the group runs it. */
int nfsp_group_replica_cfg(nfsp_group* g, int replica, nfsp_engine_cfg* out);
int nfsp_group_destroy(nfsp_group* g);
int nfsp_group_engine(nfsp_group* g, int replica, nfsp_engine** out);
int nfsp_group_step(nfsp_group* g);
/* The exchange by itself (nfsp_group_step does it when NFSP_GROUP_AVG_AR is set or
 * nfsp_group_set_exchange configured one).  Its first call copies replica 0's exchanged nets
 * everywhere. */
int nfsp_group_average_ar(nfsp_group* g);
/* The group's exchange, as nfsp_engine_set_exchange's over shards: at the end of every
 * `every`-th learner call (slice) of the group, each net in `nets` (NFSP_XCHG_AR: both agents'
 * AR nets; NFSP_XCHG_BR: their BR nets) becomes W0 + (sum_r (W_r - W0)) * scale, summed in
 * replica order from +0, and W0 <- that.  every = 0: off.  NFSP_GROUP_AVG_AR at creation is
 * nets = AR, every = cfg.slices (once per step, after its last slice), scale = 1 / R.  The first
 * exchange of a net (or nfsp_group_average_ar) copies replica 0's net (with BR also its target
 * net) to every replica instead -- also the first after a call that turns the net on again.
 *   Resume: a group's blob holds W0 and which nets have one, not the cadence.  The first
 * nfsp_group_set_exchange after nfsp_group_load_state (no step or exchange in between) continues
 * the nets whose W0 the blob restored instead of starting them over: re-issuing the saved run's
 * exchange goes on bit-identical to the uninterrupted run, AR and BR alike.  (A broadcast there
 * would replace every replica's own target net by replica 0's: the BR nets are equal at a step
 * boundary, the target nets are not -- each replica syncs its own at its own update count.)
 * Any later call that turns a net on again broadcasts as above.
 *   tests/exchange_ref.py restates this rule and the group's bookkeeping around it in numpy. */
#define NFSP_XCHG_AR 1u
#define NFSP_XCHG_BR 2u
int nfsp_group_set_exchange(nfsp_group* g, unsigned nets, int every, float scale);
/* How a group schedules its BR rounds and slices.  None of these changes an SGD
 * step: a BR piece resumes from the weights in memory, and every partition's jobs run the same
 * pieces and targets (tests/test_gpu_group.py varies them within one process).
 *   br_cap      most updates per BR piece; -1: 40 for sliced groups, whole segments (0) else
 *   br_pace     1: a partition's busiest job splits each segment into equal pieces and the
 *               others follow its piece per round; 0: plain caps
 *   br_streams  BR partitions, each its own rounds on its own stream (1..4); -1: 2 for sliced
 *               groups, else 1 (always 1 when chains share CUs)
 *   serial      1: the slices of a pipelined group run one after another (no overlap)
 *   br_persist  0: BR rounds.  >= 1: a learner call's BR work in ONE launch of the persistent
 *               kernel k_br_persist -- a chain workgroup per (replica, agent) and 48 helper
 *               workgroups writing the targets from a device work queue (groups of <= 32
 *               replicas, the reference's BR net, no loss log; others keep the rounds).  Values
 *               > 1 bound every device wait at that many s_sleep 8 rounds (default 2^18); an
 *               expired wait ends the kernel and the error surfaces at the next learner call or
 *               nfsp_group_check.  br_cap / br_pace / br_streams do not apply to it.
 * nfsp_group_default_sched reads the environment's NFSP_GROUP_BR_CAP / _BR_PACE / _BR_STREAMS /
 * NFSP_GROUP_SERIAL / NFSP_GROUP_BR_PERSIST at that call (nfsp_group_create starts from it);
 * nfsp_group_set_sched applies from the next learner call. */
typedef struct nfsp_group_sched {
  int32_t br_cap, br_pace, br_streams, serial, br_persist;
} nfsp_group_sched;
int nfsp_group_default_sched(nfsp_group_sched* out);
int nfsp_group_set_sched(nfsp_group* g, const nfsp_group_sched* sched);
int nfsp_group_get_sched(nfsp_group* g, nfsp_group_sched* out);
int nfsp_group_set_timing(nfsp_group* g, int on);
/* nfsp_engine_get_timings summed over the replicas.  The shared chain and target launches
 * count once each. */
int nfsp_group_get_timings(nfsp_group* g, double* ms /*[NFSP_TIMING_SLOTS]*/,
                           int64_t* launches /*[NFSP_TIMING_SLOTS]*/);
/* BR rounds of the last learner call: the most any BR partition ran.  Sliced groups split the
 * replicas' BR jobs into 2 partitions (nfsp_group_sched.br_streams, 1..4), each with its own
 * rounds on its own stream; the SGD steps are the same as with one. */
int nfsp_group_rounds(nfsp_group* g, int64_t* out);
/* Synchronise the group's streams and report a k_br_persist wait that expired (NFSP_EHIP). */
int nfsp_group_check(nfsp_group* g);
/* Diagnostic trace of the learner calls' plans (tools/c4_slice_spread.py: the lockstep cost of
 * a per-slice exchange across C4 ranks).  on = 1 clears and starts it; every learner call then
 * appends, per replica r and agent a, its AR and BR update counts: [call][r][a][AR, BR].
 * nfsp_group_trace copies min(cap, size) int32 values and reports the size in *n. */
int nfsp_group_set_trace(nfsp_group* g, int on);
int nfsp_group_trace(nfsp_group* g, int32_t* out, int64_t cap, int64_t* n);

/* ---- checkpoint and resume (the reference has none: main.py:21-75 trains in one
 * process and keeps nothing) ----
 * A state blob is one contiguous host buffer, and that buffer is the file: a little-endian
 * header (magic, format version, sizes, section table, 128-bit digest of the payload) and the
 * payload -- cfg and game, the schedules, EngineDev, the six nets, the live M_RL records in
 * insert order and the M_SL rows.  Session settings are not stored (timing, the loss log, the
 * update limit, a group's schedule and trace, the exchange transport and cadence: re-issue
 * nfsp_engine_set_exchange after a load).  A run continued from a loaded blob is bit-identical
 * to the uninterrupted one.
 *   Save is legal at a step boundary only (else NFSP_EINVAL): no rollout awaiting its
 * nfsp_engine_update, every slice of the step played, no exchange pending, and with an exchange
 * configured its learner-call count a multiple of `every`.  It synchronises the engine's streams.
 *   Load checks everything on the host before it writes anything (magic, version, sizes, section
 * bounds, the digest; then n_lanes, hidden, both capacities, batch, inserts_per_update,
 * target_every, epochs, fit_batch, quirks, eta, lr_*, gamma, epsilon, seed and game against the
 * engine: NFSP_EINVAL, the engine untouched).  slices, slice_lag and sched may differ: the
 * payload does not depend on them.  After the copy the device state's digest is recomputed in
 * place (csrc/state.hip k_state_digest) and compared with the header's: NFSP_EHIP on a mismatch.
 * A replica of a group is saved and loaded with its group: the blob holds every replica's cfg
 * (nfsp_state_cfg), replica r's is checked against replica r's engine, and the message of a
 * mismatch names the replica. */
typedef struct nfsp_state_info {
  int32_t version, kind;                /* format version (1); 1 = an engine's blob, 2 = a group's */
  int32_t replicas, n_sections;
  int32_t slices, slice_lag;            /* the saving engine's cfg.slices / slice_lag / sched */
  uint32_t sched, group_flags;
  int64_t total_bytes, payload_offset, payload_bytes;
  uint64_t digest[2];                   /* of the payload */
} nfsp_state_info;
/* bytes a save would write now (synchronises) */
int nfsp_engine_state_bytes(nfsp_engine* e, int64_t* out);
int nfsp_engine_save_state(nfsp_engine* e, void* host_buf, int64_t cap, int64_t* written);
int nfsp_engine_load_state(nfsp_engine* e, const void* host_buf, int64_t n);
/* The digest a save at this point would put in its header, computed on the device state where
 * it lies: equal for two engines iff they hold the same training state, whatever their
 * slicing.  Step boundaries only; synchronises.  A group replica's handle is accepted. */
int nfsp_engine_state_digest(nfsp_engine* e, uint64_t out[2]);
/* The same, also reporting the digest kernels' time (HIP events around them) and the bytes
 * they read -- how profiles/ckpt/digest_c3.json was measured. */
int nfsp_engine_state_digest_timed(nfsp_engine* e, uint64_t out[2], double* ms, int64_t* bytes);
int nfsp_group_state_bytes(nfsp_group* g, int64_t* out);
int nfsp_group_save_state(nfsp_group* g, void* host_buf, int64_t cap, int64_t* written);
int nfsp_group_load_state(nfsp_group* g, const void* host_buf, int64_t n);
/* Host only, no device: parse a blob, check its bounds and its digest; info may be NULL. */
int nfsp_state_check(const void* buf, int64_t n, nfsp_state_info* info);
/* Host only: replica's (0 for an engine's blob) cfg, with the saver's slicing, and game. */
int nfsp_state_cfg(const void* buf, int64_t n, int replica, nfsp_engine_cfg* cfg, int32_t* game);
/* Host only: the digest of n bytes (whole 8-byte words) taken as a payload. */
int nfsp_state_digest(const void* payload, int64_t n, uint64_t out[2]);

/* ---- evaluation ----
 * Exact exploitability of two average-policy nets (packed weights, device pointers; e.g.
 * nfsp_engine_weights(e, a, 0, ..)) in this Leduc variant as main.train plays it
 * (main.py:21-67; the reference's proxy is agent/agent.py:235-238 summed at main.py:73,
 * its MC evaluator main.py:82-120, commented out).  mode 0: each net's softmax as a mixed
 * strategy (NFSP's average strategy; an illegal raise's mass goes to call); mode 1: the
 * argmax the env executes (leduc/newenv.py:135-145).  out[0] / out[1]: best-response value
 * of seat 0 / 1 against the other seat's policy, over both dealers and all deals;
 * out[2] = out[0] + out[1] (exploitability, chips); out[3] = seat 0's on-policy value.
 * The whole evaluation runs on the device (csrc/evaluate.hip k_evaluate, as nfsp_evaluate_batch
 * below with NFSP_POL_AR_SOFTMAX / NFSP_POL_AR_ARGMAX on both seats: the policies, reach
 * top-down and best-response values bottom-up over the public tree, in f64); only the 4
 * results come back.  Synchronises the ctx stream. */
int nfsp_exploitability(nfsp_ctx* ctx, const float* dev_w_ar0, const float* dev_w_ar1, int mode,
                        double* out /*[4]*/);
/* The same for n pairs of nets at once (one workgroup per pair; e.g. every replica of an
 * engine group): dev_w_ar0[k] / dev_w_ar1[k] are host arrays of device pointers, out[4k..4k+3]
 * pair k's results as above. */
int nfsp_exploitability_batch(nfsp_ctx* ctx, const float* const* dev_w_ar0, const float* const* dev_w_ar1,
                              int n, int mode, double* out /*[4n]*/);

/* ---- the evaluator's tree as data (host only: no device, no ctx) ----
 * The public tree both dealers' hands of `game` run through, exactly the tables the device
 * walks (csrc/exploit_tree.h), in depth order: a level's nodes are contiguous and a parent
 * precedes its children.  Replaces reading information sets out of the CPU oracle's Env
 * (tests/studies/kuhn_policy.py).  kind: 0 decision, 1 chance, 2 terminal.  p: the acting
 * seat (decision) or the seat of the ending step (terminal).  via: the executed action that
 * leads here from a decision parent, the public rank from a chance parent.  child: by executed
 * action (decision) or public rank (chance), -1 where there is none (an illegal raise).  row:
 * a decision's row of obs / legal / every policy table, a terminal's row of pay. */
typedef struct {
  int8_t kind, p, via, nchild;
  int32_t parent;                       /* -1 at the two roots */
  int32_t child[3];
  int32_t row;
} nfsp_tree_node;                       /* 24 bytes */
int nfsp_tree_size(int game, int32_t* nn, int32_t* ndec, int32_t* nterm, int32_t* nlev);
/* obs[d][r]: the acting seat's observation bits at decision row d holding rank r.  legal[d]:
 * bit 0 = a raise is executed as a raise there, bits 1.. = the acting seat.  pay[t][i][ri][ro]:
 * seat i's reward at terminal row t with rank ri against rank ro.  lev: level k is nodes
 * [lev[k], lev[k + 1]).  root: by dealer.  deal[a][b]: P(one seat's rank a, the other's b). */
int nfsp_tree_export(int game, nfsp_tree_node* nodes /*[nn]*/, uint32_t* obs /*[ndec][3]*/,
                     uint8_t* legal /*[ndec]*/, float* pay /*[nterm][2][3][3]*/, int32_t* lev /*[nlev+1]*/,
                     int32_t* root /*[2]*/, double* deal /*[3][3]*/);

/* ---- policies of any kind, scored exactly ----
 * A policy is a net read one of four ways or a table.  Replaces the CPU-only studies
 * (tests/studies/kuhn_diag.py br_gap / anticip, kuhn_policy.py) and builds the evaluator the
 * reference left commented out (main.py:82-120: the BR player against the AR player). */
#define NFSP_POL_AR_SOFTMAX 0        /* packed f32 net: as nfsp_exploitability mode 0 */
#define NFSP_POL_AR_ARGMAX 1         /* packed f32 net: as mode 1 */
#define NFSP_POL_BR_GREEDY 2         /* packed f32 net, ReLU Q head: one-hot argmax, first max wins (an
                                        all-zero head folds), an illegal raise becomes call: what
                                        k_rollout executes without the epsilon branch */
#define NFSP_POL_BR_GREEDY_LINEAR 3  /* the same with the linear head of NFSP_EXT_LINEAR_Q */
#define NFSP_POL_TABLE 4             /* f64 [ndec][3 ranks][3 actions], rows as nfsp_tree_export's; an
                                        illegal raise's mass goes to call */
typedef struct {
  int32_t kind;                         /* NFSP_POL_* */
  int32_t reserved;                     /* 0 */
  const void* dev;                      /* device pointer: the net or the table */
} nfsp_policy;
/* Pair k plays seat0[k] at seat 0 against seat1[k] at seat 1.  out[6k..6k+5]: seat 0's best-response
 * value against seat1[k], seat 1's against seat0[k], their sum, seat 0's on-policy value, and that
 * value over dealer-0 hands only and over dealer-1 hands only (value0 = half their sum).  One
 * workgroup per pair (csrc/evaluate.hip k_evaluate: three phases, f64, the sums of
 * csrc/tree_walk.h); with kinds 0 / 1 on both seats the first four are nfsp_exploitability's.
 * Synchronises the ctx stream. */
int nfsp_evaluate_batch(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1, int n,
                        double* out /*[6n]*/);
/* The policy as the walk executes it (after the remap), at every decision row and rank, into
 * dev_out[ndec][3][3] (f64, device); rows where the other seat acts are filled too.  Scoring the
 * table gives the bits scoring the policy gives.  Replaces kuhn_policy.py's per-information-set
 * read-out through the oracle's Env.  Synchronises the ctx stream. */
int nfsp_policy_table(nfsp_ctx* ctx, const nfsp_policy* policy, double* dev_out);
/* The exact best responses as a strategy, where nfsp_evaluate_batch only has their values: one
 * joint table dev_beta[ndec][3][3] (f64, device).  Rows where seat 0 acts hold seat 0's best
 * response against seat1, rows where seat 1 acts seat 1's against seat0; every row and rank is
 * one-hot, information sets the responder's own earlier actions never reach included.  The
 * argmax is over the legal children in ascending action order and a later action wins only if
 * strictly greater: a tie, and every information set the opponent never reaches, folds (then
 * calls); an illegal raise is never chosen.  dev_q[d][r][a] (or NULL): the counterfactual value
 * of the child under action a -- what k_evaluate's max runs over, summed over the opponent's
 * rank; 0 for an illegal raise.  dev_reach[d][r] (or NULL): the counterfactual reach of the
 * information set summed over the opponent's rank, so q / reach is the expected chips of each
 * action given that it is reached: the quantity the Q net is to learn.  Scoring the table
 * against the same opponent gives nfsp_evaluate_batch's br0 / br1.  Replaces the action-value
 * side of kuhn_diag.py's per-information-set read-out.  The outputs must not overlap either
 * policy's memory or each other (refused).  One workgroup (csrc/evaluate.hip k_best_response:
 * k_evaluate's walk for its first two evaluations).  Synchronises the ctx stream. */
int nfsp_best_response_table(nfsp_ctx* ctx, const nfsp_policy* seat0, const nfsp_policy* seat1,
                             double* dev_beta /*[ndec][3][3]*/, double* dev_q /*[ndec][3][3] or NULL*/,
                             double* dev_reach /*[ndec][3] or NULL*/);

/* ---- CFR+ on the evaluator's tree (csrc/cfr.hip k_cfr_plus) ----
 * A tabular equilibrium of the game as played here: the absolute anchor the Leduc variant lacked
 * (Kuhn's is analytic; the reference has no solver).  Alternating updates, regret-matching+,
 * linearly weighted average (Tammelin 2014).  One workgroup, all state in LDS as f64 during a
 * launch and in device memory between launches; a run is cut into launches of at most
 * NFSP_CFR_LAUNCH_ITERS iterations. */
#define NFSP_CFR_LAUNCH_ITERS 1024
typedef struct nfsp_cfr nfsp_cfr;
int nfsp_cfr_create(nfsp_ctx* ctx, nfsp_cfr** out);
int nfsp_cfr_run(nfsp_cfr* h, int64_t iters);          /* continues the run; synchronises */
int nfsp_cfr_iterations(nfsp_cfr* h, int64_t* out);
/* The average strategy after the last run (uniform over legal actions before any), a device
 * table usable as NFSP_POL_TABLE; owned by the handle. */
int nfsp_cfr_average(nfsp_cfr* h, const double** dev_table);
int nfsp_cfr_state(nfsp_cfr* h, double* host_R /*[ndec][3][3]*/, double* host_S /*[ndec][3][3]*/);
int nfsp_cfr_destroy(nfsp_cfr* h);

/* ---- full-width extensive-form fictitious play on the evaluator's tree (csrc/xfp.hip k_xfp) ----
 * XFP (Heinrich, Lanctot and Silver 2015), the algorithm NFSP samples and approximates: every
 * iteration both seats compute the exact best response (nfsp_best_response_table's tie rule) to
 * the current average strategy and mix it into the average in realisation weights.  Its curve
 * is what fictitious play itself does on this tree with a perfect best response and perfect
 * averaging, in nfsp_evaluate_batch's units: the ideal beside the engine's curves and the CFR+
 * anchor (the reference has neither).  With eta > 0 the response is to the per-hand mixture
 * (1 - eta) x average + eta x last best response: NFSP's anticipatory parameter.
 * A handle holds n independent runs, one workgroup per run in one launch -- a study is a sweep
 * over eta and the weighting.  Per run: S and B [ndec][3][3], the weighted sum of the best
 * responses' realisation plans and the last one's (0 / 1, so S holds exact integers), and the
 * weight sum W; all 0 at creation.  A run is cut into launches of at most NFSP_XFP_LAUNCH_ITERS. */
#define NFSP_XFP_WEIGHT_UNIFORM 0    /* w_t = 1: fictitious play's 1/t average */
#define NFSP_XFP_WEIGHT_LINEAR 1     /* w_t = t */
#define NFSP_XFP_LAUNCH_ITERS 1024
#define NFSP_XFP_MAX_RUNS 1024
typedef struct {
  double eta;                           /* in [0, 1) */
  int32_t weight;                       /* NFSP_XFP_WEIGHT_* */
  int32_t reserved;                     /* 0 */
} nfsp_xfp_cfg;                         /* 16 bytes */
typedef struct nfsp_xfp nfsp_xfp;
int nfsp_xfp_create(nfsp_ctx* ctx, const nfsp_xfp_cfg* cfgs /*[n]*/, int n, nfsp_xfp** out);
/* Continues every run by iters iterations; synchronises.  host_gaps[n][iters] (or NULL): per run
 * and iteration br_0 + br_1 of the strategy responded to -- with eta = 0 the exploitability of
 * the average after the iterations before it (the first ever is the uniform policy's). */
int nfsp_xfp_run(nfsp_xfp* h, int64_t iters, double* host_gaps);
int nfsp_xfp_iterations(nfsp_xfp* h, int64_t* out);
/* The average strategy of a run after the last launch: S normalised per row, uniform over the
 * legal actions where a row's sum is 0 (every row before any iteration).  A device table usable
 * as NFSP_POL_TABLE; owned by the handle. */
int nfsp_xfp_average(nfsp_xfp* h, int run, const double** dev_table);
int nfsp_xfp_state(nfsp_xfp* h, int run, double* host_S /*[ndec][3][3]*/, double* host_B /*[ndec][3][3]*/,
                   double* W);
int nfsp_xfp_destroy(nfsp_xfp* h);

/* ---- external-sampling MCCFR on the evaluator's tree (csrc/mccfr.hip k_mccfr_walk, k_mccfr_apply) ----
 * ES-MCCFR (Lanctot, Waugh, Zinkevich and Bowling 2009): the sampled counterpart of CFR+ as
 * tabular NFSP is XFP's -- a plain sampled tabular learner whose cost is counted in traversals
 * and terminals visited, the yardstick beside the engine's curves in hands (the reference has no
 * solver).  A handle holds n independent runs, each with a seed and W walkers (W even).
 * Per run: R and S [ndec][3][3], int64 fixed point with NFSP_MCCFR_Q per chip (R) or per unit of
 * probability (S), and t, the completed iterations; all 0 at creation.  The tables are integers,
 * so sums over walkers do not depend on their order and the tables are bit-reproducible whatever
 * the grid, as the memory tables are.
 * Iteration t + 1 is seat i = 0, then seat 1; the half-iteration index is h = 2 t + i.
 *   1. sigma from R, every row and rank: rp_a = (double)max(R_a, 0), 0 at an illegal raise;
 *      s = (rp_0 + rp_1) + rp_2; sigma_a = rp_a / s, uniform over the legal actions where s = 0.
 *      Plain regret matching: R itself is NOT floored.  sigma is frozen for the whole
 *      half-iteration and all W walkers share it: a declared mini-batch form of MCCFR.
 *   2. walker w = 0 .. W - 1: dealer = w & 1, from root[dealer].
 *      u(node) = (x >> 8) 2^-24, x the first word of philox4x32(counter = (h low 32, h high 32,
 *      w, node), key = (seed low 32, seed high 32)): the draw depends on the node id, not on the
 *      order of the visit (a traversal visits a node at most once).
 *      A choice among probabilities p_0 .. p_k with a draw u: the first j with u < c_j and
 *      p_j > 0, c the running double sum from 0 in ascending order; the last j with p_j > 0 if
 *      there is none.
 *      The deal: drawn at the pseudo-node id nn over deal[a][b] in row-major order; seat i holds
 *      rank a, the other seat rank b.
 *      Traverse(n):
 *        terminal             returns (double)pay[row][i][r_i][r_o];
 *        chance               the child chosen by u(n) over p_public(c, r_0, r_1), c ascending;
 *        the opponent's       for each a, dS[row][r_o][a] += llrint(sigma_a Q); the child chosen by
 *        decision             u(n) over sigma[row][r_o];
 *        seat i's decision    v_a = Traverse(child_a) for the legal a, ascending; v = 0, then
 *                             v = v + sigma_a v_a, ascending, no contraction;
 *                             dR[row][r_i][a] += llrint((v_a - v) Q); returns v.
 *   3. R += dR, S += dS.
 * Two counts per run: traversals (2 W t) and terminals visited -- a traversal touches a whole
 * own-action subtree, not one hand.  |v_a - v| <= 2 max|pay| (10 chips on Leduc's tables, 4 on
 * Kuhn's), so a run whose W x (iterations done + to come) could carry an entry past 2^62 is
 * refused: W x iterations <= 2^62 / (NFSP_MCCFR_Q x 2 max|pay|), and the message names the bound.
 * One lane runs one traversal, NFSP_MCCFR_WG_WALKERS of them per workgroup, which adds into int64
 * tables in LDS and flushes its non-zero entries with 64-bit atomic adds; k_mccfr_apply, one
 * small launch per half-iteration, does step 3, zeroes the deltas and writes the next sigma and
 * the average.  No workgroup waits for another: the order is the stream's.  tests/mccfr_ref.py
 * restates the rule in numpy, and R, S and the counts agree to the bit. */
#define NFSP_MCCFR_Q 16777216        /* 2^24 */
#define NFSP_MCCFR_MAX_RUNS 64
#define NFSP_MCCFR_MAX_WALKERS 4194304   /* 2^22 */
#define NFSP_MCCFR_WG_WALKERS 1024   /* traversals of one workgroup (256 lanes, 4 each in turn) */
typedef struct {
  uint64_t seed;
  int32_t walkers;                      /* W: even, 2 .. NFSP_MCCFR_MAX_WALKERS */
  int32_t reserved;                     /* 0 */
} nfsp_mccfr_cfg;                       /* 16 bytes */
typedef struct nfsp_mccfr nfsp_mccfr;
/* Host only (no device, no ctx): every cfg's fields, n in 1 .. NFSP_MCCFR_MAX_RUNS, and that
 * every run may reach `iters` iterations in all on `game`'s tables without overflow. */
int nfsp_mccfr_cfgs_check(int game, const nfsp_mccfr_cfg* cfgs /*[n]*/, int n, int64_t iters);
int nfsp_mccfr_create(nfsp_ctx* ctx, const nfsp_mccfr_cfg* cfgs /*[n]*/, int n, nfsp_mccfr** out);
/* Continues every run by iters iterations: 2 iters (walk, apply) pairs on the ctx stream, then
 * one synchronisation. */
int nfsp_mccfr_run(nfsp_mccfr* h, int64_t iters);
int nfsp_mccfr_iterations(nfsp_mccfr* h, int64_t* out);
/* out[0] traversals (2 W t), out[1] terminals visited.  Synchronises the ctx stream. */
int nfsp_mccfr_counts(nfsp_mccfr* h, int run, int64_t* out /*[2]*/);
/* The average strategy of a run: S normalised per row, uniform over the legal actions where a
 * row's sum is 0 (every row before any iteration).  A device table usable as NFSP_POL_TABLE;
 * owned by the handle. */
int nfsp_mccfr_average(nfsp_mccfr* h, int run, const double** dev_table);
int nfsp_mccfr_state(nfsp_mccfr* h, int run, int64_t* host_R /*[ndec][3][3]*/, int64_t* host_S /*[ndec][3][3]*/);
int nfsp_mccfr_destroy(nfsp_mccfr* h);

/* ---- outcome-sampling MCCFR on the same handle (csrc/mccfr.hip k_mccfr_os_walk, k_mccfr_apply) ----
 * OS-MCCFR (the same paper): one traversal is one sampled hand and one terminal, the regret-
 * minimising tabular learner that consumes exactly what NFSP consumes, a trajectory per sample --
 * the rung of the ladder counted in the engine's own unit, hands.
 * A run has a seed, W walkers (even) and an exploration rate epsilon.  R, S, t and NFSP_MCCFR_Q,
 * step 1 (sigma from R by plain regret matching, frozen for the half-iteration), step 3 and
 * k_mccfr_apply, the draw u(node), the choice rule, the dealer w & 1 and the deal at the
 * pseudo-node nn are exactly external sampling's, above.  Step 2 for walker w of half-iteration
 * h = 2 t + i is one path; all f64, no FMA contraction, the operations in the order written:
 *   start with q = 1.0;
 *   chance               the child chosen by u(n) over p_public(c, r_0, r_1), c ascending;
 *   the opponent's       winv = Q / q (one division); for each a,
 *   decision             dS[row][r_o][a] += llrint(sigma_a * winv); then the child chosen by u(n)
 *                        over sigma[row][r_o];
 *   seat i's decision,   xi_a = eps / (double)L + (1.0 - eps) * sigma_a for the legal a, 0 at an
 *   L legal actions      illegal raise; a* = choice(xi, u(n)); push the frame (row, a*);
 *                        q = q * xi_{a*}; go to child a*;
 *   terminal             c = (double)pay[row][i][r_i][r_o] / q and x = 1.0;
 *   then the frames, deepest first:
 *                        s = sigma[row][r_i][a*] and g = c * x; for the legal a ascending,
 *                        dR[row][r_i][a] += llrint((g * (1.0 - s)) * Q) if a == a*,
 *                        dR[row][r_i][a] += llrint((-(g * s)) * Q) otherwise; then x = x * s.
 * The standard estimator with chance and the opponent sampled on-policy: their probabilities
 * cancel, and only seat i's sampling product q remains.  The average is the "simple" one external
 * sampling uses, at the opponent's nodes, with 1 / q undoing seat i's exploration above the node.
 * Traversals are 2 W t and terminals visited are 2 W t: equal by construction.
 * Overflow.  Let omega(game, eps) be the largest, over both seats and all root-to-terminal paths,
 * of the product of L_k / eps over that seat's decisions on the path (in doubles: from 1.0,
 * times ((double)L_k / eps) from the root down; computed on the host from the tree, not taken as
 * (3 / eps)^4).  1 / q <= omega, so per traversal an R entry moves by at most max|pay| omega Q and
 * an S entry by at most omega Q, and a run is refused when
 *   W x iterations > floor(2^62 / ((Q x max(max|pay|, 1)) x omega)),
 * the message naming the bound.  This is a worst-case bound and it is tight on budget: Leduc
 * (omega = 36 / eps^4, max|pay| = 5) at eps = 0.6 allows 197,912,092 walker-iterations, at
 * eps = 0.0625 23,301; Kuhn (omega = 6 / eps^2, max|pay| = 2) 8,246,337,208 and 89,478,485.
 * There is one NFSP_MCCFR_Q; small eps costs budget, not a second fixed point.
 * epsilon must lie in [NFSP_MCCFR_OS_EPS_MIN, 1]; NaN is refused.
 * A lane runs one path: the frames are packed into one 64-bit scalar (no scratch), sigma is
 * re-read from LDS by row on the way back, and the one pay entry of a traversal is read from
 * device memory, so the workgroup's LDS holds sigma, dR, dS and the node table only.
 * tests/mccfr_os_ref.py restates the rule in numpy, and R, S and the counts agree to the bit. */
#define NFSP_MCCFR_OS_EPS_MIN 0.0625
typedef struct {
  uint64_t seed;
  int32_t walkers;                      /* W: even, 2 .. NFSP_MCCFR_MAX_WALKERS */
  int32_t reserved;                     /* 0 */
  double epsilon;                       /* in [NFSP_MCCFR_OS_EPS_MIN, 1] */
} nfsp_mccfr_os_cfg;                    /* 24 bytes */
/* Host only, as nfsp_mccfr_cfgs_check, with outcome sampling's fields and overflow bound. */
int nfsp_mccfr_os_cfgs_check(int game, const nfsp_mccfr_os_cfg* cfgs /*[n]*/, int n, int64_t iters);
/* The handle is an nfsp_mccfr: nfsp_mccfr_run / _iterations / _counts / _average / _state /
 * _destroy serve it unchanged, and run re-checks outcome sampling's own bound. */
int nfsp_mccfr_os_create(nfsp_ctx* ctx, const nfsp_mccfr_os_cfg* cfgs /*[n]*/, int n, nfsp_mccfr** out);
/* out: 0 external sampling (nfsp_mccfr_create), 1 outcome sampling (nfsp_mccfr_os_create),
 * 2 outcome sampling with baselines (nfsp_mccfr_vr_create). */
int nfsp_mccfr_sampling(nfsp_mccfr* h, int* out);

/* ---- baseline-corrected outcome sampling on the same handle (csrc/mccfr.hip k_mccfr_vr_walk,
 * k_mccfr_apply, k_mccfr_vr_apply) ----
 * VR-MCCFR (Schmid et al. 2019; Davis, Schmid and Bowling 2020): outcome sampling with a control
 * variate ("baseline") at every decision of the sampled path.  Still one trajectory and one
 * terminal per sample; the pay / q estimate is replaced by values corrected on the way back up --
 * the tabular analogue of what a critic does for a sampled learner.
 * State per run: R and S as above, and the baseline sums Bs [ndec][3][3] (int64, NFSP_MCCFR_Q per
 * chip) and counts Bn [ndec][3][3] (int64); all 0 at creation.  The baseline of a half-iteration
 * is frozen as sigma is:
 *   B[row][r][a] = clamp((double)Bs / ((double)Bn * Q), -P, P), and 0 where Bn == 0,
 * P = max|pay| of the game's table.  B is in the perspective of the seat that acts at row, r that
 * seat's rank.  Every true value lies in [-P, P], so the clamp costs nothing and keeps the
 * overflow bound usable.
 * Step 1 (sigma from R), step 3, the draw u(node), the choice rule, the dealer w & 1, the deal at
 * the pseudo-node nn, xi_a = eps / (double)L + (1.0 - eps) * sigma_a at seat i's decisions, the
 * on-policy sampling of chance and the opponent, q, and winv = Q / q with
 * dS[row][r_o][a] += llrint(sigma_a * winv) at the opponent's decisions are outcome sampling's,
 * above: with the same seed, eps and R the path of walker w, its deal and its dS are outcome
 * sampling's bit for bit.  What changes is the pass back up; all f64, no FMA contraction, the
 * operations in the order written:
 *   on the way down      push a frame at every decision, both seats'.  At seat i's keep xi_{a*}
 *                        and qk, the value of q before it is multiplied by xi_{a*}.
 *   terminal             v = (double)pay[row][i][r_i][r_o].  No division.
 *   then the frames, deepest first:
 *   the opponent's       b_a = -B[row][r_o][a] for the legal a (seat i's perspective), 0 at an
 *   (row, r_o, a*)       illegal raise;
 *                        dBs[row][r_o][a*] += llrint((-v) * Q) and dBn[row][r_o][a*] += 1;
 *                        v = ((sigma_0 * b_0 + sigma_1 * b_1) + sigma_2 * b_2) + (v - b_{a*}).
 *                        No division by sigma: the opponent is sampled on-policy and it cancels.
 *   seat i's             b_a = B[row][r_i][a];
 *   (row, r_i, a*,       dBs[row][r_i][a*] += llrint(v * Q) and dBn[row][r_i][a*] += 1;
 *    xi_{a*}, qk)        u_a = b_a for the legal a != a*, u_{a*} = b_{a*} + (v - b_{a*}) / xi_{a*};
 *                        vbar = 0, then vbar = vbar + sigma_a * u_a for the legal a ascending;
 *                        dR[row][r_i][a] += llrint(((u_a - vbar) / qk) * Q) for each legal a;
 *                        then v = vbar.
 *   chance               passes v through: no baseline at chance nodes.
 *   3. R += dR, S += dS, Bs += dBs, Bn += dBn, then the next sigma and the next B.
 * ANY baseline leaves the estimator unbiased: E over a* of u_a is the value below a whatever b
 * is.  The acting seat's perspective and the sign flip at the opponent's nodes serve only the
 * baseline's quality on a zero-sum table -- one table then learns from both seats' half-iterations.
 * Traversals are 2 W t and terminals visited are 2 W t, as outcome sampling's.
 * Overflow.  With |B| <= P the host computes from the tree, for either seat as seat i, Vmax(n), a
 * bound on |v| at node n:
 *   terminal P; chance the most of its children's; the opponent's decision 2 P + the most of its
 *   children's; seat i's decision with L legal actions P + (the most of its children's + P) *
 *   ((double)L / eps).
 * One traversal moves an R entry at seat i's node n by at most Rmax = (2 Vmax(n)) * (the product
 * of L_k / eps over seat i's decisions above n), a Bs entry by at most Bmax = Vmax of a decision's
 * child, and an S entry by omega (outcome sampling's), all times Q and each the most over nodes
 * and seats.  A run is refused when
 *   W x iterations > floor(2^62 / (Q x max(Rmax, Bmax, omega))),
 * the message naming the bound.  Leduc at eps = 0.6 (Rmax = 9432.2 chips) allows 29,142,433
 * walker-iterations, at eps = 0.0625 5,479; Kuhn 1,264,775,645 and 21,047,312: a seventh to a
 * quarter of outcome sampling's, since a corrected value is bounded by the baseline's range at
 * every level, not by one pay.  Bn grows by at most 1 per traversal and entry.
 * A lane runs one path: up to 8 frames of 16 bits are two 64-bit scalars, qk for seat i's second
 * to fourth decision are three registers chosen by compares, and xi_{a*} is formed again from
 * sigma and eps on the way back by the same operations (no scratch).  The workgroup's LDS holds
 * sigma, B, dR, dS, dBs, dBn and the node table.  k_mccfr_vr_apply, a third small launch per
 * half-iteration, does the baseline's part of step 3.  tests/mccfr_vr_ref.py restates the rule in
 * numpy, and R, S, Bs, Bn and the counts agree to the bit. */
typedef struct {
  uint64_t seed;
  int32_t walkers;                      /* W: even, 2 .. NFSP_MCCFR_MAX_WALKERS */
  int32_t reserved;                     /* 0 */
  double epsilon;                       /* in [NFSP_MCCFR_OS_EPS_MIN, 1] */
} nfsp_mccfr_vr_cfg;                    /* 24 bytes */
/* Host only, as nfsp_mccfr_os_cfgs_check, with the overflow bound above. */
int nfsp_mccfr_vr_cfgs_check(int game, const nfsp_mccfr_vr_cfg* cfgs /*[n]*/, int n, int64_t iters);
/* The handle is an nfsp_mccfr: nfsp_mccfr_run / _iterations / _counts / _average / _state /
 * _destroy serve it unchanged, run re-checks this kind's own bound, nfsp_mccfr_sampling gives 2. */
int nfsp_mccfr_vr_create(nfsp_ctx* ctx, const nfsp_mccfr_vr_cfg* cfgs /*[n]*/, int n, nfsp_mccfr** out);
/* The baseline's sums and counts of a run.  Synchronises the ctx stream.  Refused for a handle of
 * another sampling kind. */
int nfsp_mccfr_baseline(nfsp_mccfr* h, int run, int64_t* host_Bs /*[ndec][3][3]*/, int64_t* host_Bn /*[ndec][3][3]*/);
/* Replaces the baseline's sums and counts of a run and recomputes its B: how a test pins an
 * arbitrary baseline and how a user installs an informed one (a table of action values in the
 * acting seat's perspective times Q, with count 1).  Refused: a negative count, a non-zero sum at
 * a zero count, a sum or count beyond 2^61 (the run's budget is counted from 0), and a handle of
 * another sampling kind.  R, S and the iteration count are left as they are. */
int nfsp_mccfr_set_baseline(nfsp_mccfr* h, int run, const int64_t* host_Bs /*[ndec][3][3]*/,
                            const int64_t* host_Bn /*[ndec][3][3]*/);

/* ---- regret matching+ and linear averaging on the same handle (csrc/mccfr.hip k_mccfr_x_apply) ----
 * Two of CFR+'s three ingredients (Tammelin 2014; the third, alternating updates, every kind here
 * has) on any of the three sampling kinds; with sampling 2 this is VR-MCCFR+ (Schmid et al. 2019).
 * A fourth way to create an nfsp_mccfr.  `sampling` is the handle's: one walk kernel serves a
 * launch, so every run of a handle names the same one.  `regret` and `average` are per run.
 * Steps 1 and 2 are exactly the sampling kind's, above: the draws, the choices, the dealer, the
 * deal, dR, dS, dBs, dBn and the counts, bit for bit.  Step 3 of a half-iteration changes.  t is
 * the number of iterations completed before the one in progress, the same for both of its
 * half-iterations.  Per entry, by the one thread that owns it, in this order:
 *   R = R + dR                                int64; under NFSP_MCCFR_REGRET_PLUS then
 *   R = max(R, 0)                             int64.  The floor is applied once per half-iteration,
 *                                             to the sum over the W walkers: the declared
 *                                             mini-batch form, sigma was frozen for them all.
 *   S = S + dS                                int64, as before.
 *   Sw = Sw + (double)(t + 1) * (double)dS    f64, one multiplication and one addition, no FMA
 *                                             contraction.  Sw [ndec][3][3] is 0.0 at creation.
 *   for sampling 2: Bs += dBs, Bn += dBn, the next B, as k_mccfr_vr_apply does.
 * The next sigma comes from the new R by the unchanged step 1.  Two averages, both by the rule of
 * nfsp_mccfr_average (normalised per row, uniform where the row's sum is 0): the uniform one from
 * (double)S, the linear one from Sw.  nfsp_mccfr_average returns the one cfg.average names,
 * nfsp_mccfr_average_of either, so one run scores both on identical sample paths.  Sw and both
 * averages are kept whatever `average` is.
 * Why Sw is f64: a linearly weighted int64 sum would carry the worst-case bound W omega Q T^2 / 2,
 * which on Leduc at eps = 0.6 allows about 1,390 iterations at W = 2^10.  dS is an integer sum and
 * does not depend on the grid, and the f64 accumulation over half-iterations is done by a single
 * owner in stream order: Sw is bit-reproducible whatever the grid.  It is deterministic, not
 * exact: its relative error is of order T 2^-53 after T iterations, and it needs no refusal.
 * Overflow is the sampling kind's own bound, unchanged, and nfsp_mccfr_run re-checks it:
 * |max(R + dR, 0)| <= |R + dR| <= |R| + |dR|, so by induction |R| stays within the sum of |dR|
 * over the half-iterations so far, which is what that bound bounds.
 * k_mccfr_x_apply is the one apply launch of a half-iteration of this kind, the baseline's part
 * included: an iteration is 4 launches where nfsp_mccfr_vr_create's is 6.  One thread per
 * (row, rank); no workgroup waits for another.  tests/mccfr_x_ref.py restates the rule in numpy;
 * R, S, Bs, Bn, the counts and Sw (as its 64 bits) agree to the bit. */
#define NFSP_MCCFR_REGRET_PLAIN 0
#define NFSP_MCCFR_REGRET_PLUS 1
#define NFSP_MCCFR_AVG_UNIFORM 0
#define NFSP_MCCFR_AVG_LINEAR 1
typedef struct {
  uint64_t seed;
  int32_t walkers;                      /* W: even, 2 .. NFSP_MCCFR_MAX_WALKERS */
  int32_t sampling;                     /* 0 external, 1 outcome, 2 outcome with baselines: nfsp_mccfr_sampling's numbers */
  double epsilon;                       /* sampling 1, 2: in [NFSP_MCCFR_OS_EPS_MIN, 1]; sampling 0: must be 0.0 */
  int32_t regret;                       /* NFSP_MCCFR_REGRET_* */
  int32_t average;                      /* NFSP_MCCFR_AVG_*: the table nfsp_mccfr_average returns */
} nfsp_mccfr_x_cfg;                     /* 32 bytes */
/* Host only, as nfsp_mccfr_cfgs_check: every field of every cfg (a message names
 * nfsp_mccfr_x_cfg.<field>; a run whose sampling differs from run 0's is named with its run), then
 * the sampling kind's own overflow bound. */
int nfsp_mccfr_x_cfgs_check(int game, const nfsp_mccfr_x_cfg* cfgs /*[n]*/, int n, int64_t iters);
/* The handle is an nfsp_mccfr: nfsp_mccfr_run / _iterations / _counts / _average / _state /
 * _sampling / _destroy serve it unchanged, and _baseline / _set_baseline where sampling is 2. */
int nfsp_mccfr_x_create(nfsp_ctx* ctx, const nfsp_mccfr_x_cfg* cfgs /*[n]*/, int n, nfsp_mccfr** out);
/* out[0] regret, out[1] average of a run; (0, 0) for a handle of nfsp_mccfr_create / _os_create /
 * _vr_create, whose rule that is. */
int nfsp_mccfr_rule(nfsp_mccfr* h, int run, int32_t out[2]);
/* The uniform (NFSP_MCCFR_AVG_UNIFORM) or the linear (NFSP_MCCFR_AVG_LINEAR) average of a run, a
 * device table as nfsp_mccfr_average's.  Refused for a handle not made by nfsp_mccfr_x_create:
 * the other kinds keep no Sw. */
int nfsp_mccfr_average_of(nfsp_mccfr* h, int run, int average, const double** dev_table);
/* Sw of a run.  Synchronises the ctx stream.  Refused as nfsp_mccfr_average_of. */
int nfsp_mccfr_weighted(nfsp_mccfr* h, int run, double* host_Sw /*[ndec][3][3]*/);

/* ---- regret nets on the same handle (csrc/mccfr.hip k_mccfr_net_apply, after k_mccfr_x_apply) ----
 * Regression CFR (Waugh, Morrill, Bagnell and Bowling 2015) with sampled regrets: the learner
 * holds its regrets in two packed 30-64-3 nets, the engine's own shape, and the walkers' sigma is
 * the nets', not the table's.  With sampled regrets it is Deep CFR (Brown, Lerer, Gross and
 * Sandholm 2019) in the limit of an unbounded memory and a full-batch fit.  A fifth way to create
 * an nfsp_mccfr.  The cfg holds nfsp_mccfr_x_cfg's fields with the same meaning and the same
 * checks, and adds `target`, `fit_steps` (K), `loss`, `lr` and `momentum`, all per run.
 * Each run has two nets w[seat] (NP f32, linear heads: NFSP_ACT_LINEAR) and their momentum states
 * v[seat], 0.0 at creation; the caller gives the initial nets, which are copied.
 * Steps 1 to 3 of the sampling kind and of nfsp_mccfr_x_create are unchanged, bit for bit: the
 * draws, the choices, dR, dS, dBs, dBn, the counts, R, its floor, S, Sw, both averages and B.  One
 * thing changes: the sigma a half-iteration's walkers read is not regret matching on R.  After the
 * tables of a half-iteration of seat i are applied, for seat i, with tw = (double)(t + 1) as above:
 *   targets   f64, per (d, r) of the seat's rows and action a:
 *             NFSP_MCCFR_NET_TARGET_AVG     y_a = (double)R_a / (((double)W * Q) * tw)
 *             NFSP_MCCFR_NET_TARGET_ROWMAX  m = the largest |R_b| over the legal b, as int64;
 *                                           y_a = (double)R_a / (double)m, and 0.0 where m = 0
 *             An illegal raise has y = 0.0, and the default mask of nfsp_fit_tables removes it.
 *   fit       K steps of nfsp_fit_tables' step exactly as stated below: f32, contraction off, the
 *             same orders, t = (float)y, uniform weights what = (float)(1.0 / N) with N the seat's
 *             (d, r) rows, the legal actions' mask, the linear head and the cfg's loss.  It starts
 *             from w[i] and v[i], and both carry over to the seat's next fit.  The loss before the
 *             first step and at the final weights (one more forward; the same number where K = 0)
 *             is kept per (run, seat), summed as nfsp_fit_tables' host_loss is.
 *   head      z[d][r][.] (f32): the net's three head sums at the seat's rows, by the step's forward
 *   sigma     rp_a = max((double)z_a, 0.0), 0.0 at an illegal raise; sigma[d][r] is rp normalised by
 *             the rule of step 1 (s = (rp_0 + rp_1) + rp_2, rp_a / s, uniform over the legal
 *             actions where s = 0): the function that turns R into sigma for the other kinds.
 * The other seat's rows of z and sigma keep their bits: its net did not change, and its head is
 * formed again from it by the same operations.  A net written through nfsp_mccfr_net_weights
 * between runs therefore reaches z and sigma at the first apply after it, the fitted seat's after
 * its fit.
 * At creation both seats take this step once with R = 0 and tw = 1: K steps toward zero regrets.
 * Declared property: the first sigma is the nets', not uniform.
 * The regret-matching table on R is still computed and kept beside: sigma_tab.  The distance of
 * the two tables is the epsilon of regression CFR's bound.  Overflow is the sampling kind's own
 * bound, re-checked by nfsp_mccfr_run: the bound on the sum of |dR| does not depend on sigma.
 * k_mccfr_net_apply follows k_mccfr_x_apply in every half-iteration on the ctx stream: an
 * iteration is 6 launches.  Grid (2 seats, n runs), 512 threads, the net, v, the seat's rows and
 * the workspace in LDS as k_fit_tables holds them, all K steps inside the launch; no atomics, no
 * workgroup waits for another.  Determinism: a run's nets, z and sigma are functions of the run
 * alone, not of its place in the handle or of n.  tests/mccfr_net_ref.py restates the rule in
 * numpy; the integer tables agree to the bit when the restatement reads the device's sigma, the
 * nets within nfsp_fit_tables' own bar. */
#define NFSP_MCCFR_NET_TARGET_AVG 0
#define NFSP_MCCFR_NET_TARGET_ROWMAX 1
#define NFSP_MCCFR_NET_MAX_STEPS 4096
typedef struct {
  uint64_t seed;
  int32_t walkers;                      /* W: even, 2 .. NFSP_MCCFR_MAX_WALKERS */
  int32_t sampling;                     /* the handle's, as nfsp_mccfr_x_cfg.sampling */
  double epsilon;                       /* as nfsp_mccfr_x_cfg.epsilon */
  int32_t regret;                       /* NFSP_MCCFR_REGRET_* */
  int32_t average;                      /* NFSP_MCCFR_AVG_* */
  int32_t target;                       /* NFSP_MCCFR_NET_TARGET_* */
  int32_t fit_steps;                    /* K: 0 .. NFSP_MCCFR_NET_MAX_STEPS */
  int32_t loss;                         /* NFSP_FIT_MSE or NFSP_FIT_HUBER */
  float lr;                             /* finite, >= 0 */
  float momentum;                       /* in [0, 1) */
  int32_t reserved;                     /* must be 0 */
} nfsp_mccfr_net_cfg;                   /* 56 bytes */
/* Host only, as nfsp_mccfr_x_cfgs_check: every field of every cfg (a message names
 * nfsp_mccfr_net_cfg.<field> and the run), then the sampling kind's own overflow bound. */
int nfsp_mccfr_net_cfgs_check(int game, const nfsp_mccfr_net_cfg* cfgs /*[n]*/, int n, int64_t iters);
/* dev_w0[2 k + seat]: run k's initial net of that seat, NP f32 on the device; copied, and refused
 * unless every value is finite.  The handle is an nfsp_mccfr: nfsp_mccfr_run / _iterations /
 * _counts / _average / _average_of / _weighted / _state / _rule / _sampling / _destroy serve it
 * unchanged, and _baseline / _set_baseline where sampling is 2. */
int nfsp_mccfr_net_create(nfsp_ctx* ctx, const nfsp_mccfr_net_cfg* cfgs /*[n]*/, int n,
                          const float* const* dev_w0 /*[n][2]*/, nfsp_mccfr** out);
/* The three tables of a run on the device: the sigma the walkers read, regret matching on R
 * (f64 [ndec][3][3] each) and the heads z (f32 [ndec][3][3]).  Any of the three may be NULL.
 * This and the two calls below are refused for a handle not made by nfsp_mccfr_net_create. */
int nfsp_mccfr_net_tables(nfsp_mccfr* h, int run, const double** dev_sigma, const double** dev_sigma_tab,
                          const float** dev_z);
/* nfsp_mccfr_net_create with nets of hidden width `hidden` (one of 16, 32, 64, 128; one width per
 * handle): dev_w0[2 k + seat] is NP(hidden) f32 (nfsp_net_params), nfsp_mccfr_net_weights hands
 * out NP(hidden) floats, the fit is nfsp_fit_tables_h's at that width, and everything else of the
 * handle is unchanged.  hidden 64 is nfsp_mccfr_net_create, bit for bit.  A width that is not
 * built, or whose rows do not fit in LDS for the game, is NFSP_EINVAL (nfsp_fit_width_check). */
int nfsp_mccfr_net_create_h(nfsp_ctx* ctx, int hidden, const nfsp_mccfr_net_cfg* cfgs /*[n]*/, int n,
                            const float* const* dev_w0 /*[n][2]*/, nfsp_mccfr** out);
/* The nets' hidden width: 64 for a handle of nfsp_mccfr_net_create.  Refused for the other kinds. */
int nfsp_mccfr_net_hidden(nfsp_mccfr* h, int* out);
/* A seat's net and momentum state, NP f32 each on the device: may be read, and written between
 * runs (on the ctx stream, or synchronised with it).  Either of the two may be NULL. */
int nfsp_mccfr_net_weights(nfsp_mccfr* h, int run, int seat, float** dev_w, float** dev_v);
/* out[seat][0] / [1]: the loss of the seat's last fit before its first step / at its final
 * weights.  Synchronises the ctx stream. */
int nfsp_mccfr_net_loss(nfsp_mccfr* h, int run, double out[2][2]);
/* Timing of a handle of any kind, off at creation.  While it is on, nfsp_mccfr_run records three
 * HIP events per half-iteration on the ctx stream (before the walk, after it, after the applies;
 * at most NFSP_MCCFR_TIMED_ITERS iterations per call) and adds the elapsed times up after its
 * synchronisation.  nfsp_mccfr_set_timing sets the sums to 0; nfsp_mccfr_get_timings gives
 * out_ms[0] the walks', out_ms[1] the applies', and the iterations they cover.  The tables do
 * not depend on it. */
#define NFSP_MCCFR_TIMED_ITERS 4096
int nfsp_mccfr_set_timing(nfsp_mccfr* h, int enable);
int nfsp_mccfr_get_timings(nfsp_mccfr* h, double out_ms[2], int64_t* iterations);

/* ---- the memories as tables (csrc/memtab.hip k_memtab, k_memtab_sum) ----
 * M_SL (utils/ReservoirBuffer.py:18-28) and M_RL (utils/replay_buffer.py:30-41) counted per
 * information set where they lie, from the packed device records (SlRec 16 B {obs bits, a[3]},
 * RlRec 32 B {s, s2, argmax | t << 8 | r << 16, a[3], pad}).  The reference can
 * only sample its memories; M_SL per information set IS NFSP's tabular average strategy, and the
 * AR net a fit of it.
 * A record belongs to (seat, observation), one (row, rank) of nfsp_tree_export's rows; agent i
 * is seat i.  out[ndec][3 ranks][3 actions][3 fields], int64 -- integers only, so the bits do not
 * depend on the order of accumulation:
 *   NFSP_MEM_SL  [k][0] records of the set whose argmax3(a) is k (the rollout's first-maximum
 *                rule, before the raise-to-call remap); [k][1] the sum over ALL records of the set
 *                of fix(a_k); [k][2] 0
 *   NFSP_MEM_RL  [k][0] records of the set whose stored argmax (meta & 0xff) is k; [k][1] the sum
 *                of their r in half units (the int8 in meta); [k][2] how many of them have t set.
 *                The key is the stored s: under NFSP_QUIRK_ALIAS_RL the stored s and a of every
 *                tuple of a hand are that hand's LAST ones, and the table reports
 *                the records as stored.  A stored argmax above 2 matches no information set.
 * fix(x) = rint((double)x * 2^NFSP_MEMTAB_FIX_SHIFT) as int64, ties to even: exact for one-hot rows
 * and for the 24-bit uniform draws.  A component with |x| >= 256 or not finite is saturated to
 * +-(2^32 - 1) (NaN: 0) and counted in `clamped`, so with fewer than 2^31 records per table no sum
 * overflows; more are NFSP_EINVAL.
 * A call for `seat` writes every value of every row where that seat acts and leaves the other
 * seat's rows untouched: two calls into one buffer give the joint table.  Records whose observation
 * is no information set of the seat add to `unmatched` only.  Every call synchronises its stream. */
#define NFSP_MEM_SL 0
#define NFSP_MEM_RL 1
#define NFSP_MEMTAB_FIX_SHIFT 24
#define NFSP_MEMTAB_MAX_SEGMENTS 8
typedef struct { const void* dev_recs; int64_t n; } nfsp_mem_segment;   /* packed SlRec (16 B) / RlRec (32 B), 16-byte aligned */
typedef struct { int64_t records, matched, unmatched, clamped; } nfsp_memtab_info;
/* Host only: row * 3 + rank of the information set in which `seat` observes `obs`, -1 if there is
 * none -- read from the very lookup table the kernel stages. */
int nfsp_memtab_lookup(int game, int seat, uint32_t obs);
/* Host only: fix(x), the one host definition (the kernel shares its source). */
int64_t nfsp_memtab_fix(float x);
/* Raw form: the records of up to NFSP_MEMTAB_MAX_SEGMENTS device segments, on the ctx stream. */
int nfsp_memory_table(nfsp_ctx* ctx, int game, int kind, int seat, const nfsp_mem_segment* segs, int nsegs,
                      int64_t* dev_out, nfsp_memtab_info* info);
/* An engine's memories, both agents in one launch into the joint table: M_SL rows [0, sl_size),
 * the live M_RL records as the at most two pieces of the circular log.  Requires what
 * nfsp_engine_state_digest requires (a step boundary, so no pending M_SL list; else NFSP_EINVAL)
 * and synchronises the engine's streams first.  A group replica's handle is accepted. */
int nfsp_engine_memory_table(nfsp_engine* e, int kind, int64_t* dev_out /*[ndec][3][3][3]*/,
                             nfsp_memtab_info info[2]);
/* Every replica's joint table in ONE launch, through a device job table (2R jobs). */
int nfsp_group_memory_tables(nfsp_group* g, int kind, int64_t* dev_out /*[R][ndec][3][3][3]*/,
                             nfsp_memtab_info* info /*[R][2]*/);
/* The two kernels' time in this thread's last table call (HIP events around them): how
 * profiles/memtab/ was measured. */
int nfsp_memtab_last_ms(double* ms);

/* ---- what the BR net is fitted to, and what it holds (csrc/memtab.hip k_memtab's third kind,
 *      csrc/head_tables.hip k_head_tables) ----
 * update_best_response_network (agent/agent.py:219-241) fits the BR net to one TD value per
 * sampled M_RL tuple: v = r + gamma * max Q_target(s2), or r for a terminal tuple when
 * NFSP_QUIRK_TERMINAL_BOOTSTRAP is off, written at the tuple's argmax(a).  The reference never
 * sees these values outside a minibatch.  NFSP_MEM_TD counts them per information set over ALL
 * live records where they lie, with k_br_targets' arithmetic operation for operation (the same
 * forward, fwd_lds, of the target net in LDS; r as float, the product and the sum in double, one
 * rounding to float), keyed as NFSP_MEM_RL by the stored s and the stored argmax k:
 *   [k][0] records whose stored argmax is k; [k][1] the sum of fix(v); [k][2] the sum of
 *   fix(max Q_target(s2)) over the records that bootstrap (a terminal-treated record adds 0).
 * fix, the saturation and `clamped` are the memory tables' (every fix of a matched record that
 * saturates counts); integers only, so the bits do not depend on the order of accumulation.  s2 may
 * be any 30-bit word (a terminal observation is no decision row).  The head of the target net is
 * ReLU, or linear with NFSP_EXT_LINEAR_Q in `quirks`; no other bit but TERMINAL_BOOTSTRAP is read.
 * Two caveats the table does not hide: under NFSP_QUIRK_ALIAS_RL the key is the hand's LAST s
 * (DESIGN.md §3), and under NFSP_QUIRK_ROW0_TARGET the net is fitted to one of these values per
 * 128 sampled rows (agent/agent.py:240-241) -- the table states what is stored, whatever the quirks. */
#define NFSP_MEM_TD 2
typedef struct { const float* dev_target_w; double gamma; uint32_t quirks, reserved; } nfsp_td_args;   /* reserved: 0 */
/* Raw form, as nfsp_memory_table: RlRec segments of `seat` against the packed target net. */
int nfsp_td_table(nfsp_ctx* ctx, int game, int seat, const nfsp_mem_segment* segs, int nsegs,
                  const nfsp_td_args* td, int64_t* dev_out, nfsp_memtab_info* info);
/* An engine's live M_RL records, both agents in one launch, each against its own target net
 * (NET_TARGET) with cfg.gamma and cfg.quirks; requires what nfsp_engine_memory_table requires. */
int nfsp_engine_td_table(nfsp_engine* e, int64_t* dev_out /*[ndec][3][3][3]*/, nfsp_memtab_info info[2]);
/* Every replica's in ONE launch: gamma, quirks and the target net ride in each table's device
 * job, so the replicas of a heterogeneous group (nfsp_group_create_v) keep their own. */
int nfsp_group_td_tables(nfsp_group* g, int64_t* dev_out /*[R][ndec][3][3][3]*/,
                         nfsp_memtab_info* info /*[R][2]*/);
/* The raw head outputs of n packed nets at every (row, rank) of nfsp_tree_export's rows, into
 * dev_out[n][ndec][3 ranks][3] (f32, device): what a BR net holds as Q values, where
 * nfsp_policy_table only has its one-hot argmax.  All three outputs are written, an illegal
 * raise's too; the remap is the caller's.  dev_w: a host array of n device pointers; act[k]:
 * NFSP_ACT_RELU, _LINEAR or _SOFTMAX of net k.  One workgroup per net, the net in LDS and one
 * observation per lane through fwd_lds: the bits the rollout acts on and k_br_targets bootstraps
 * from (agent/agent.py:126,219,230).  game must be the ctx's.  At most 64 nets per launch; the
 * host loops beyond.  Synchronises the ctx stream. */
int nfsp_head_tables(nfsp_ctx* ctx, int game, const float* const* dev_w, const int* act, int n,
                     float* dev_out /*[n][ndec][3][3]*/);
/* The same for n packed nets of hidden width `hidden` (16, 32, 64 or 128; NP(hidden) f32 each): per
 * hidden unit the set bits' W1 entries ascending from +0, plus b1, ReLU; the units ascending into
 * the three head sums, plus b2, then the activation.  That is fwd_lds' order, so at 64 the ReLU
 * and linear heads have nfsp_head_tables' bits.  A plain kernel: one workgroup per net, the net in
 * LDS in packed order, one observation per lane. */
int nfsp_head_tables_h(nfsp_ctx* ctx, int game, int hidden, const float* const* dev_w, const int* act, int n,
                       float* dev_out /*[n][ndec][3][3]*/);

/* ---- tables that act (csrc/act_table.hip; csrc/rollout.hip k_rollout_t, k_rollout_gt) ----
 * Any of an engine's four (agent, role) slots can be acted by a table over nfsp_tree_export's
 * rows instead of its net: where Agent.play calls avg_strategy_model.predict (role 0) or
 * best_response_model.predict (role 1) for seat `agent` (agent/agent.py:124-151), the rollout
 * looks the seat's observation up (the memory tables' lookup, nfsp_memtab_lookup) and takes the
 * row's three f32 values, bit for bit, as the vector the net would have output.  Nothing else of
 * Agent.play changes: the epsilon draw and its counter, the epsilon-random vector,
 * NFSP_EXT_SAMPLE_AR's sampling from the vector, the env's raise-to-call remap, the all-zero rule
 * (a fold that leaves no RL record), the SL record (the vector raw, or one-hot under
 * NFSP_EXT_SL_ONEHOT) and the action counters.  A row is an action vector, not necessarily a
 * distribution.  Slots mix freely; an engine with no table launches the kernels it always did.
 * Every decision of a hand is a row of the tree, so a lookup cannot miss; if one does, the vector
 * is all-zero and the slot's miss counter counts it.
 * Deviation (declared, beside the policy lag): a table is not snapshotted.  With cfg.slice_lag 2,
 * and under nfsp_rollout_with, the table installed at the step boundary acts in every slice of
 * the step, whatever weights or snapshot the rollout is given.
 * The engine copies the table (the caller may free its own) and reads only the rows where seat
 * `agent` acts; those are copied to the host once and must be finite (NFSP_EINVAL names the row).
 * Setting requires what nfsp_engine_state_digest requires (a step boundary), else NFSP_EINVAL.
 * A group replica's handle is refused by the engine's set call: use the group call, which rewrites
 * the replicas' rollout table.  Tables are session settings, like timing and the loss log: they
 * are in neither the state blob (format version 1 still) nor the digest, and nfsp_engine_load_state
 * leaves them alone.  The agent's BR chain trains on M_RL as before.
 * role: 0 = AR (avg_strategy_model), 1 = BR (best_response_model), as nfsp_engine_weights' net. */
int nfsp_engine_set_act_table(nfsp_engine* e, int agent, int role,
                              const float* dev_rows /* [ndec][3][3] f32, or NULL: the net acts again */);
/* dev_rows: the engine's copy, NULL if none; misses: lookups of the slot that found no
 * information set since its table was installed (synchronises).  Either may be NULL. */
int nfsp_engine_get_act_table(nfsp_engine* e, int agent, int role, const float** dev_rows, int64_t* misses);
int nfsp_group_set_act_table(nfsp_group* g, int replica, int agent, int role, const float* dev_rows);

/* ---- tabular NFSP: Q tables from M_RL, M_SL tables as rows (csrc/memtab.hip k_memtab's fourth
 *      kind; csrc/tabq.hip k_table_rows) ----
 * Learners without function approximation that see exactly the nets' data, for the tables that act
 * above: the BR role's net replaced by a Q table fitted to the live M_RL records, the AR role's by
 * M_SL's own table.  Neither is the reference's algorithm; both are diagnostics.
 *
 * Tabular Q by fitted-Q sweeps over one seat's M_RL records.  Q is f32 [ndec][3][3] over
 * nfsp_tree_export's rows, the act-table layout.  One sweep is Q_{j+1} = rows(TDQ(M_RL; Q_j), fill).
 * TDQ is NFSP_MEM_TD with the target net replaced by the table.  For a matched record (its stored s
 * an information set of the seat, its stored argmax k <= 2): sid2 = the lookup of (seat, s2), the
 * same staged hash; qmax = sid2 < 0 ? 0.0f : fmaxf(fmaxf(Q[sid2][0], Q[sid2][1]), Q[sid2][2]) --
 * all three entries count, an illegal raise's too, exactly as the net's three outputs do;
 * terminal = t && !(quirks & NFSP_QUIRK_TERMINAL_BOOTSTRAP); v = r for a terminal record, else
 * r + gamma * qmax with NFSP_MEM_TD's arithmetic (r as float, the product and the sum in double,
 * each rounded, one rounding to float).  Fields as NFSP_MEM_TD: [k][0] the count, [k][1] the sum of
 * fix(v), [k][2] the sum of fix(qmax) over the records that bootstrap; info and `clamped` as there.
 * No quirk bit but TERMINAL_BOOTSTRAP is read.  A terminal s2 is no information set and bootstraps
 * 0 (it counts in field 0 and adds 0 to field 2): the table is immune to the terminal-bootstrap
 * quirk's value where the net is not.
 * rows, stat NFSP_ROWS_TD_MEAN, per entry with count c and sum S = field 1:
 * (float)(((double)S / (double)c) * 2^-24) if c > 0, else fill[entry]; fill == NULL means 0.  An
 * unseen (set, action) therefore stays at fill through every sweep, and Q_0 = fill.
 * Sweeps are Jacobi: sweep j reads buffer j & 1 and writes the other, never in place.  The sums are
 * integers, so the bits depend neither on the order of accumulation nor on the grid.
 * Convergence: without NFSP_QUIRK_ALIAS_RL a record's s2 is a strictly later decision of the same
 * hand, so the successor relation on a seat's information sets is acyclic and no deeper than the
 * tree's nlev (nfsp_tree_size): sweeps = nlev reaches the fixed point of the sample-mean Bellman
 * operator exactly, and a further sweep changes no bit.  Under ALIAS_RL the key is the hand's LAST
 * s and nothing is promised beyond "K sweeps of the stated operator".
 *
 * M_SL rows, per (row, rank) from an NFSP_MEM_SL table, with m_a = field 1 of action a,
 * M = (m0 + m1) + m2 in int64, c_a = field 0 and n = c0 + c1 + c2:
 *   NFSP_ROWS_SL_MASS    out[a] = (float)((double)m_a / (double)M)
 *   NFSP_ROWS_SL_ARGMAX  out[a] = (float)((double)c_a / (double)n)
 * For both the whole row is fill's row (0 with fill == NULL) where n == 0, where M <= 0 or where any
 * m_a < 0: the memory tables' two strategies before the raise-to-call remap, with a declared value
 * where M_SL is empty or holds no mass. */
#define NFSP_MEM_TDQ 3
#define NFSP_ROWS_SL_MASS 0
#define NFSP_ROWS_SL_ARGMAX 1
#define NFSP_ROWS_TD_MEAN 2
#define NFSP_TABQ_MAX_SWEEPS 64
#define NFSP_TABLE_ROWS_MAX 65535
/* Raw form, one sweep's sums: RlRec segments of `seat` against the joint Q table dev_q (only the
 * seat's rows are read), as nfsp_td_table otherwise.  Synchronises the ctx stream. */
int nfsp_tdq_table(nfsp_ctx* ctx, int game, int seat, const nfsp_mem_segment* segs, int nsegs,
                   const float* dev_q /*[ndec][3][3]*/, double gamma, uint32_t quirks, int64_t* dev_out,
                   nfsp_memtab_info* info);
/* n joint int64 tables -> n f32 row tables, one workgroup each, on the ctx stream; synchronises.
 * dev_changed[t] (if given): the entries of table t whose f32 bits differ from dev_prev's (0
 * without dev_prev).  dev_prev may be dev_rows itself: an entry is compared before it is stored.
 * At most NFSP_TABLE_ROWS_MAX tables. */
int nfsp_table_rows(nfsp_ctx* ctx, int game, int stat, const int64_t* dev_tab /*[n][ndec][3][3][3]*/,
                    const float* dev_fill /*[n][ndec][3][3] or NULL*/, const float* dev_prev /*or NULL*/, int n,
                    float* dev_rows /*[n][ndec][3][3]*/, int32_t* dev_changed /*[n] or NULL*/);
/* `sweeps` (1..NFSP_TABQ_MAX_SWEEPS) fitted-Q sweeps over an engine's live M_RL records, each
 * agent against its own rows of the joint table with its cfg.gamma and cfg.quirks: 3 launches per
 * sweep on the ctx stream, the two Q buffers in the library's workspace, ONE synchronisation and
 * one info copy at the end.  dev_q: the final table; dev_tab (or NULL): the last sweep's sums;
 * info: the last sweep's (only `clamped` depends on the sweep); *changed: the entries the last sweep
 * changed.  Requires what nfsp_engine_memory_table requires (a step boundary); a group replica's
 * handle is accepted.  Neither the engine's state nor its digest changes. */
int nfsp_engine_tabular_q(nfsp_engine* e, int sweeps, const float* dev_fill /*[ndec][3][3] or NULL*/,
                          float* dev_q /*[ndec][3][3]*/, int64_t* dev_tab /*[ndec][3][3][3] or NULL*/,
                          nfsp_memtab_info info[2], int32_t* changed);
/* Every replica's in the same launches (2R jobs per sweep), each replica with its own gamma and
 * quirks: arrays as above with a leading [R]. */
int nfsp_group_tabular_q(nfsp_group* g, int sweeps, const float* dev_fill, float* dev_q, int64_t* dev_tab,
                         nfsp_memtab_info* info /*[R][2]*/, int32_t* changed /*[R]*/);

/* ---- nets fitted to tables (csrc/fit_tables.hip k_fit_tables) ----
 * The other direction of everything above: a [ndec][3][3] table over nfsp_tree_export's rows put
 * into a packed 30-64-3 net, by deterministic, weighted, full-batch gradient descent with momentum.
 * The reference only ever fits sampled minibatches (agent/agent.py:209-264; nfsp_mlp_fit above is
 * that: one net, <= 64 rows, no weights, no mask).  Diagnostics: the approximation
 * floors of the AR and Q nets, and warm starts of self-play from a solved table.
 *
 * Rows.  A job's rows are the (d, r) with legal[d] >> 1 == seat, ascending in (d, r): 195 per seat
 * for Leduc, 12 for Kuhn.  A row's input is obs[d][r] expanded to 0/1, its target
 * t = (float)dev_target[d][r][.], its weight what = (float)(w / W) with w = dev_weight[d][r] (1
 * without) and W the sum of the seat's w in row order, both in double; its mask m_a = dev_mask's
 * entry != 0, or without a mask 1 for a legal action (the raise 0 where legal[d] bit 0 is clear).
 *
 * One step, all f32 with fp contract off, every gradient from the weights before the step:
 *   forward   z1_j = (sum over the inputs i ascending of x_i W1[i][j]) + b1_j, h = relu(z1),
 *             z_a = (sum over j ascending of h_j W2[j][a]) + b2_a -- nfsp_mlp_fit's order
 *   CE        c_a = z_a - max(max(z_0, z_1), z_2), e_a = expf(c_a), s = (e_0 + e_1) + e_2,
 *             p_a = e_a / s, T = (t_0 + t_1) + t_2;  dz_a = what (p_a T - t_a);
 *             row loss = what * -((t_0 l_0 + t_1 l_1) + t_2 l_2) with l_a = c_a - logf(s).
 *             No clipping: this is NOT Keras' clipped cross-entropy that nfsp_mlp_fit and the
 *             chains reproduce (p clipped to [1e-7, 1 - 1e-7]); l_a is finite for every finite z.
 *   MSE/Huber y_a = z_a (linear head) or relu(z_a), e = y_a - t_a, g = e (MSE) or e clamped to
 *             [-1, 1] (Huber, delta 1);  dz_a = (what m_a) g, and 0 where the ReLU head has
 *             z_a <= 0;  row loss = what ((m_0 l_0 + m_1 l_1) + m_2 l_2), l = e e / 2, or |e| - 1/2
 *             where Huber clamps.
 *   backward  dW2[j][a] = sum over the rows ascending of h_j dz_a, db2_a = sum of dz_a;
 *             dz1_j = z1_j > 0 ? (dz_0 W2[j][0] + dz_1 W2[j][1]) + dz_2 W2[j][2] : 0;
 *             dW1[i][j] = sum over the rows ascending of x_i dz1_j, db1_j = sum of dz1_j
 *   update    v <- momentum v + g,  w <- w - lr v
 * Every sum starts at +0.  The kernel skips the inputs and rows with x_i = 0, which for finite
 * values gives the bits of the full sums.  A row of weight 0 and a masked entry contribute +-0.
 * Determinism: one thread owns one parameter and sums its rows in the order above, so a job's
 * result is a function of the job alone -- not of the grid, the job's place in the list or their
 * number; no atomics.  `steps` split over calls with dev_v carried gives the bits of one call.
 * host_loss[k][0] / [1]: the sum of the row losses (f32 terms, summed in double in row order) at
 * the weights before step 1 / at the final weights (one more forward).
 *
 * nfsp_fit_jobs_check is the validation that needs no device: n and steps >= 0, each job's seat,
 * head and loss, their pairing (CE with the softmax head only, MSE and Huber with the ReLU or
 * linear head), no mask with CE, lr finite and >= 0, 0 <= momentum < 1, dev_w and dev_target set.
 * nfsp_fit_tables repeats it, requires game to be the ctx's, copies every job's net, momentum
 * state, table and weights to the host once and checks, before anything is launched: every value
 * finite (a target as float too), the seat's weights >= 0 with a positive sum, CE targets >= 0, no
 * two jobs sharing dev_w / dev_v memory.  A violation is NFSP_EINVAL, nfsp_last_error names the
 * job and the row, and nothing was changed.  The hidden width is 64 (nfsp_fit_tables_h: 16, 32,
 * 64 or 128, see below).  One workgroup per job, all
 * `steps` inside the launch, the net, v, the rows and the workspace in LDS; at most
 * NFSP_FIT_MAX_JOBS jobs per launch, the host loops beyond.  Synchronises the ctx stream. */
#define NFSP_FIT_CE 0      /* softmax head only */
#define NFSP_FIT_MSE 1     /* ReLU or linear head */
#define NFSP_FIT_HUBER 2   /* ReLU or linear head, delta 1 */
#define NFSP_FIT_MAX_JOBS 64
typedef struct {
  float* dev_w;              /* packed net, NP f32, in and out */
  float* dev_v;              /* momentum state, NP f32, in and out; NULL: zero at the call's start, dropped at its end */
  const double* dev_target;  /* [ndec][3][3], rows of nfsp_tree_export */
  const double* dev_weight;  /* [ndec][3] >= 0; NULL: 1 at every information set of the seat */
  const uint8_t* dev_mask;   /* [ndec][3][3], 1 = this entry has a target; NULL: the legal actions.  Must be NULL with NFSP_FIT_CE */
  int32_t seat, head, loss;  /* seat 0/1: the rows where that seat acts; head NFSP_ACT_*; loss NFSP_FIT_* */
  float lr, momentum;        /* lr finite >= 0, 0 <= momentum < 1 */
} nfsp_fit_job;
int nfsp_fit_jobs_check(const nfsp_fit_job* jobs, int n, int64_t steps);   /* host only, no device */
int nfsp_fit_tables(nfsp_ctx* ctx, int game, const nfsp_fit_job* jobs, int n, int64_t steps,
                    double* host_loss /*[n][2] or NULL*/);
/* The hidden width as a parameter.  A packed net of width H is W1[30][H] | b1[H] | W2[H][3] | b2[3]:
 * NP(H) = 34 H + 3 floats at the offsets 0, 30 H, 31 H, 34 H.  Built: H = 16, 32, 64, 128, each its
 * own instantiation of the step above, operation for operation with H free (one thread owns one
 * parameter: 3 H + 3 <= 512 threads for W2 and b2).  128 is the widest whose job fits a
 * workgroup's LDS on Leduc: 4 (2 NPP + nm (16 + H)) bytes, NPP = NP rounded up to 4 and nm = 3 x
 * the larger seat's rows rounded up to 4 (Leduc 196: 29,472 / 46,368 / 80,160 / 147,744 B).
 * nfsp_net_params: *np = NP(hidden); another width is NFSP_EINVAL, and nfsp_last_error lists the
 *   widths built.  Host only.
 * nfsp_fit_width_check: the dynamic LDS a job of `game` needs at that width into *lds_bytes (may
 *   be NULL); a width whose rows do not fit is NFSP_EINVAL naming the bytes and the bound, a width
 *   that is not built as nfsp_net_params refuses it.  Host only.
 * nfsp_fit_tables_h: nfsp_fit_tables with every job's dev_w / dev_v holding NP(hidden) floats (the
 *   overlap and finiteness checks use that length).  hidden 64 is nfsp_fit_tables: same kernel,
 *   same bits. */
int nfsp_net_params(int hidden, int64_t* np);
int nfsp_fit_width_check(int game, int hidden, int64_t* lds_bytes);
int nfsp_fit_tables_h(nfsp_ctx* ctx, int game, int hidden, const nfsp_fit_job* jobs, int n, int64_t steps,
                      double* host_loss /*[n][2] or NULL*/);

#ifdef __cplusplus
}
#endif
#endif /* NFSP_H */
