// Engine groups (nfsp_group_*): R replicas stepped together, their chains in shared launches.
// Host code only: the group object, its cfg rules, exchange, scheduling knobs and trace, the
// group brought to rest with its replicas' views (group_rest, group_view: mem_view.h), and
// the group's learner call (group_update), which plans the BR work with group_plan.h and
// launches learner.hip's kernels through its launchers (learner_internal.h) -- or, opted in
// (sched.br_persist), the persistent BR kernel through br_persist.h, at five marked call sites.
// Built with the default flags: nothing here is on the SGD chains' path.
#include <stdlib.h>
#include <string.h>

#include <string>

#include "br_persist.h"
#include "mem_view.h"

namespace nn = nfsp::nn;
namespace plan = nfsp::plan;
using namespace nfsp::eng;
using namespace nfsp::chain;

constexpr int GROUP_BR_STREAMS = 4;   // at most; nfsp_group_sched.br_streams (group_update)

struct nfsp_group {
  nfsp_ctx* ctx = nullptr;
  int R = 0;
  unsigned flags = 0;
  // nfsp_group_create_v: some replica's cfg differs from replica 0's in more than the seed (no
  // exchange then); br_uniform: gamma, lr_br and quirks are the same everywhere (group_br_sched)
  bool hetero = false, br_uniform = true;
  std::vector<nfsp_engine*> eng;
  hipStream_t s_ar = nullptr, s_br = nullptr;
  // further BR streams: a sliced group's BR jobs run in up to GROUP_BR_STREAMS partitions,
  // each its own rounds on its own stream (partition 0 on s_br); created on first use, so a
  // group with one partition holds no extra stream (and no extra hardware queue)
  hipStream_t s_brp[GROUP_BR_STREAMS - 1] = {};
  void* d_roll = nullptr;        // the replicas' rollout arguments (static device table)
  // per learner call: job / prep / final tables, host (pinned) staging -> device, one copy;
  // two sets by slice parity (a pipelined step's slice j + 1 fills its set while slice j's
  // chains still read theirs)
  char* h_tab[2] = {nullptr, nullptr};
  char* d_tab[2] = {nullptr, nullptr};
  size_t tab_cap[2] = {0, 0};
  hipEvent_t snap_ev[2][2] = {};  // pipelined step: [parity][AR, BR stream] snapshot copies done
  // the replicas' EngineDev, gathered on device and read back in one copy
  EngineDev** d_stp = nullptr;   // [R] -> each replica's state
  EngineDev* d_st = nullptr;     // [R]
  EngineDev* h_st = nullptr;     // [R] pinned
  float** d_war = nullptr;       // [3 nets][R][2] weight pointers (k_group_xchg)
  float* w0 = nullptr;           // [3][2][NP] the exchanged nets after the last exchange
  unsigned w0_valid = 0;         // nets (NFSP_XCHG_*) broadcast from replica 0 already
  unsigned w0_loaded = 0;        // nets whose W0 nfsp_group_load_state restored, until the next
                                 // nfsp_group_set_exchange, exchange or step
  unsigned xchg_nets = 0;        // nfsp_group_set_exchange
  int xchg_every = 0;
  float xchg_scale = 1.f;
  int64_t calls = 0;             // learner calls (slices) so far
  int64_t rounds = 0;            // BR rounds of the last learner call (stats)
  nfsp_group_sched sched{};      // nfsp_group_set_sched (from nfsp_group_default_sched)
  int32_t* h_err = nullptr;      // br_persist.h: the bail flags
  int chain_lds = 0;             // LDS per chain workgroup: 4R chains on the device's CUs
  bool trace_on = false;         // nfsp_group_set_trace: per call [R][2][AR, BR] update counts
  std::vector<int32_t> trace;
};

// every stream the group enqueues on, idle
static int group_sync(const nfsp_group* g) {
  if (g->ctx) NFSP_HIP(hipStreamSynchronize(g->ctx->stream));
  for (hipStream_t st : {g->s_ar, g->s_br, g->s_brp[0], g->s_brp[1], g->s_brp[2]})
    if (st) NFSP_HIP(hipStreamSynchronize(st));
  static_assert(GROUP_BR_STREAMS == 4, "group_sync names every BR stream");
  return NFSP_OK;
}

extern "C" int nfsp_group_destroy(nfsp_group* g) {
  if (!g) return NFSP_OK;
  (void)group_sync(g);
  for (nfsp_engine* e : g->eng) nfsp_engine_destroy(e);
  for (int p = 0; p < 2; ++p) {
    if (g->h_tab[p]) (void)hipHostFree(g->h_tab[p]);
    if (g->d_tab[p]) (void)hipFree(g->d_tab[p]);
    for (hipEvent_t ev : g->snap_ev[p])
      if (ev) (void)hipEventDestroy(ev);
  }
  if (g->h_st) (void)hipHostFree(g->h_st);
  brp_flags_free(g->h_err);                        // br_persist.h
  for (void* p : {(void*)g->d_war, (void*)g->w0, g->d_roll, (void*)g->d_stp, (void*)g->d_st})
    if (p) (void)hipFree(p);
  for (hipStream_t st : {g->s_ar, g->s_br})
    if (st) (void)hipStreamDestroy(st);
  for (hipStream_t st : g->s_brp)
    if (st) (void)hipStreamDestroy(st);
  delete g;
  return NFSP_OK;
}

namespace {
// The first field in which b differs from a, or nullptr (engine_cfg.h's field classes): of those
// the replicas of a group must share (with quirks' two bits that select the BR chain kernel of a
// shared launch), and of those that may differ, the seed apart.
const char* group_uniform_diff(const nfsp_engine_cfg& a, const nfsp_engine_cfg& b) {
  return cfg_first_diff(a, b, CFG_SHAPE | CFG_SESSION);
}
const char* group_free_diff(const nfsp_engine_cfg& a, nfsp_engine_cfg b) {
  b.seed = a.seed;
  return cfg_first_diff(a, b, CFG_HYPER);
}
bool group_br_same(const nfsp_engine_cfg& a, const nfsp_engine_cfg& b) {
  return !memcmp(&a.gamma, &b.gamma, sizeof(double)) && !memcmp(&a.lr_br, &b.lr_br, sizeof(float)) &&
         a.quirks == b.quirks;
}

// nfsp_group_cfgs_check's rules; hetero / br_uniform (may be null): see nfsp_group
int group_cfgs_scan(const nfsp_engine_cfg* cfgs, int replicas, unsigned flags, bool* hetero, bool* br_uniform) {
  NFSP_REQUIRE(cfgs, "null argument");
  NFSP_REQUIRE(replicas >= 1 && replicas <= NFSP_GROUP_MAX_REPLICAS, "replicas must be in [1, 256]");
  NFSP_REQUIRE((flags & ~NFSP_GROUP_AVG_AR) == 0, "unknown group flags");
  bool het = false, bru = true;
  for (int r = 0; r < replicas; ++r) {
    if (const char* f = group_uniform_diff(cfgs[0], cfgs[r]))
      return nfsp::fail(NFSP_EINVAL, std::string("group cfgs: ") + f + " of replica " + std::to_string(r) +
                                         " differs from replica 0's (the replicas of a group share it)");
    if (nfsp::eng::engine_cfg_check(&cfgs[r]) != NFSP_OK)
      return nfsp::fail(NFSP_EINVAL, "group cfgs: replica " + std::to_string(r) + ": " + nfsp_last_error());
    const char* d = group_free_diff(cfgs[0], cfgs[r]);
    if (d && (flags & NFSP_GROUP_AVG_AR))
      return nfsp::fail(NFSP_EINVAL, std::string("group cfgs: NFSP_GROUP_AVG_AR on a heterogeneous group (") + d +
                                         " of replica " + std::to_string(r) +
                                         " differs from replica 0's): nets trained under different "
                                         "hyperparameters are not averaged");
    het = het || d != nullptr;
    bru = bru && group_br_same(cfgs[0], cfgs[r]);
  }
  if (hetero) *hetero = het;
  if (br_uniform) *br_uniform = bru;
  return NFSP_OK;
}
}  // namespace

extern "C" int nfsp_group_cfgs_check(const nfsp_engine_cfg* cfgs, int replicas, unsigned flags) {
  return group_cfgs_scan(cfgs, replicas, flags, nullptr, nullptr);
}

extern "C" int nfsp_group_create(nfsp_ctx* ctx, const nfsp_engine_cfg* cfg, int replicas, unsigned flags,
                                 nfsp_group** out) {
  NFSP_REQUIRE(ctx && cfg && out, "null argument");
  NFSP_REQUIRE(replicas >= 1 && replicas <= NFSP_GROUP_MAX_REPLICAS, "replicas must be in [1, 256]");
  std::vector<nfsp_engine_cfg> cfgs((size_t)replicas, *cfg);
  for (int r = 0; r < replicas; ++r) cfgs[r].seed = cfg->seed + (uint64_t)r;
  return nfsp_group_create_v(ctx, cfgs.data(), replicas, flags, out);
}

extern "C" int nfsp_group_replica_cfg(nfsp_group* g, int replica, nfsp_engine_cfg* out) {
  NFSP_REQUIRE(g && out && replica >= 0 && replica < g->R, "bad argument");
  *out = g->eng[replica]->cfg;
  return NFSP_OK;
}

extern "C" int nfsp_group_create_v(nfsp_ctx* ctx, const nfsp_engine_cfg* cfgs, int replicas, unsigned flags,
                                   nfsp_group** out) {
  NFSP_REQUIRE(ctx && cfgs && out, "null argument");
  bool hetero = false, br_uniform = true;
  int ck = group_cfgs_scan(cfgs, replicas, flags, &hetero, &br_uniform);
  if (ck != NFSP_OK) return ck;
  const nfsp_engine_cfg* cfg = &cfgs[0];   // the fields every replica shares
  *out = nullptr;
  // up to 4R chain workgroups run at once (2R AR + a BR round's 2R): past one per CU they
  // share CUs, each with an equal share of the LDS
  int dev = 0, cus = 0;
  NFSP_HIP(hipGetDevice(&dev));
  NFSP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  nfsp_group* g = new nfsp_group();
  g->ctx = ctx;
  g->R = replicas;
  g->flags = flags;
  g->hetero = hetero;
  g->br_uniform = br_uniform;
  if (flags & NFSP_GROUP_AVG_AR) {     // the per-step AR exchange
    g->xchg_nets = NFSP_XCHG_AR;
    g->xchg_every = cfg->slices;
    g->xchg_scale = 1.0f / (float)replicas;
  }
  g->chain_lds = chain_lds_shared((4 * replicas + cus - 1) / (cus > 0 ? cus : 1));
  nfsp_group_default_sched(&g->sched);
  for (int r = 0; r < replicas; ++r) {
    nfsp_engine* e = nullptr;
    const int rc = nfsp::eng::engine_create(ctx, &cfgs[r], false, &e);
    if (rc != NFSP_OK) {
      nfsp_group_destroy(g);
      return rc;
    }
    g->eng.push_back(e);
  }
  for (hipStream_t* st : {&g->s_ar, &g->s_br}) {
    const hipError_t sr = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    if (sr != hipSuccess) {
      nfsp_group_destroy(g);
      return nfsp::hip_fail(sr, "nfsp_group_create: hipStreamCreate");
    }
  }
  for (auto& pe : g->snap_ev)
    for (hipEvent_t& ev : pe) {
      const hipError_t er = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (er != hipSuccess) {
        nfsp_group_destroy(g);
        return nfsp::hip_fail(er, "nfsp_group_create: hipEventCreate");
      }
    }
  int rc = nfsp::eng::group_rollout_table(g->eng.data(), replicas, &g->d_roll);
  if (rc != NFSP_OK) {
    nfsp_group_destroy(g);
    return rc;
  }
  std::vector<float*> war(3 * 2 * replicas);
  std::vector<EngineDev*> stp(replicas);
  for (int r = 0; r < replicas; ++r) {
    for (int n = 0; n < 3; ++n)
      for (int a = 0; a < 2; ++a) war[((size_t)n * replicas + r) * 2 + a] = g->eng[r]->w + (a * 3 + n) * nn::NP;
    stp[r] = g->eng[r]->st;
  }
  hipError_t r = hipMalloc((void**)&g->d_war, sizeof(float*) * war.size());
  if (r == hipSuccess) r = hipMalloc((void**)&g->w0, sizeof(float) * 3 * 2 * nn::NP);
  if (r == hipSuccess) r = hipMemcpy(g->d_war, war.data(), sizeof(float*) * war.size(), hipMemcpyHostToDevice);
  if (r == hipSuccess) r = hipMalloc((void**)&g->d_stp, sizeof(EngineDev*) * replicas);
  if (r == hipSuccess) r = hipMalloc((void**)&g->d_st, sizeof(EngineDev) * replicas);
  if (r == hipSuccess) r = hipHostMalloc((void**)&g->h_st, sizeof(EngineDev) * replicas, hipHostMallocDefault);
  if (r == hipSuccess) r = brp_flags_alloc(&g->h_err);   // br_persist.h
  if (r == hipSuccess) r = hipMemcpy(g->d_stp, stp.data(), sizeof(EngineDev*) * replicas, hipMemcpyHostToDevice);
  if (r != hipSuccess) {
    nfsp_group_destroy(g);
    return nfsp::hip_fail(r, "nfsp_group_create");
  }
  *out = g;
  return NFSP_OK;
}

namespace nfsp {
namespace eng {
int group_state(nfsp_group* g, GroupState* out) {
  NFSP_REQUIRE(g && out, "null argument");
  *out = GroupState{g->ctx, g->R, g->flags, g->eng.data(), g->w0, &g->w0_valid, &g->w0_loaded, &g->calls, g->xchg_every};
  return NFSP_OK;
}

// mem_view.h: the group at a step boundary, its streams idle
int group_rest(nfsp_group* g, const char* what, bool for_load) {
  for (const nfsp_engine* e : g->eng)
    if (e->pending_update ||
        (!for_load && (e->rollouts % (uint64_t)e->slices != 0 || e->rollouts != g->eng[0]->rollouts)))
      return nfsp::fail(NFSP_EINVAL, std::string(what) + ": not at a step boundary");
  if (!for_load && g->xchg_every > 0 && g->calls % g->xchg_every != 0)
    return nfsp::fail(NFSP_EINVAL, std::string(what) + ": not at a step boundary (the exchange is due only after further learner calls)");
  return group_sync(g);
}

int group_view(nfsp_group* g, const char* what, GroupState* G, std::vector<MemView>* v) {
  int rc = group_state(g, G);
  if (rc != NFSP_OK) return rc;
  if ((rc = group_rest(g, what)) != NFSP_OK) return rc;
  v->resize(g->R);
  for (int r = 0; r < g->R; ++r)
    if ((rc = engine_view(g->eng[r], what, &(*v)[r])) != NFSP_OK) return rc;
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_group_engine(nfsp_group* g, int r, nfsp_engine** out) {
  NFSP_REQUIRE(g && out && r >= 0 && r < g->R, "bad argument");
  *out = g->eng[r];
  return NFSP_OK;
}

// A replica's slot acted by a table (act_table.hip), at a step boundary of the group; the
// replicas' rollout table is rewritten, the table pointers ride in the replica's row
extern "C" int nfsp_group_set_act_table(nfsp_group* g, int replica, int agent, int role, const float* dev_rows) {
  NFSP_REQUIRE(g, "null argument");
  NFSP_REQUIRE(replica >= 0 && replica < g->R, "nfsp_group_set_act_table: bad replica");
  int rc = group_rest(g, "nfsp_group_set_act_table");
  if (rc != NFSP_OK) return rc;
  if ((rc = act_table_install(g->eng[replica], agent, role, dev_rows, "nfsp_group_set_act_table")) != NFSP_OK) return rc;
  return group_rollout_table(g->eng.data(), g->R, &g->d_roll);
}

// the group's exchange (k_group_xchg) on stream `s`
static int group_xchg_launch(nfsp_group* g, hipStream_t s) {
  const unsigned nets = g->xchg_nets ? g->xchg_nets : NFSP_XCHG_AR;
  g->w0_loaded = 0;
  // nets not broadcast yet take replica 0's (a BR net with its target net)
  unsigned bc = nets & ~g->w0_valid;
  if (bc & NFSP_XCHG_BR) bc |= 4u;
  const float scale = g->xchg_nets ? g->xchg_scale : 1.0f / (float)g->R;
  const int rc = launch_group_xchg(g->d_war, g->w0, g->R, nets, bc, scale, s);
  if (rc != NFSP_OK) return rc;
  g->w0_valid |= nets;
  return NFSP_OK;
}

extern "C" int nfsp_group_average_ar(nfsp_group* g) {
  NFSP_REQUIRE(g, "null argument");
  NFSP_REQUIRE(!g->hetero,
               "nfsp_group_average_ar: the replicas' cfgs differ (a heterogeneous group has no exchange)");
  return group_xchg_launch(g, g->ctx->stream);
}

extern "C" int nfsp_group_set_exchange(nfsp_group* g, unsigned nets, int every, float scale) {
  NFSP_REQUIRE(g, "null argument");
  NFSP_REQUIRE((nets & ~(NFSP_XCHG_AR | NFSP_XCHG_BR)) == 0, "nets: NFSP_XCHG_AR | NFSP_XCHG_BR");
  NFSP_REQUIRE(every >= 0 && (every == 0 || nets), "every >= 0 (and nets when on)");
  NFSP_REQUIRE(every == 0 || !g->hetero,
               "nfsp_group_set_exchange: the replicas' cfgs differ (a heterogeneous group has no exchange)");
  // a net this call turns on starts like the rank path's (AvgPolicyExchange broadcasts rank 0's
  // nets, then nfsp_engine_set_exchange takes them as W0): its next exchange copies replica 0's
  // net everywhere instead of applying deltas against a W0 from before the exchange was off.
  // Not the first call after nfsp_group_load_state: the cadence is a session setting, so a
  // resumed run re-issues it, and the nets whose W0 the blob restored go on from that W0 -- a
  // broadcast would replace the replicas' own target nets by replica 0's.
  const unsigned on = every ? nets : 0;
  g->w0_valid &= ~(on & ~g->xchg_nets & ~g->w0_loaded);
  g->w0_loaded = 0;
  g->xchg_nets = on;
  g->xchg_every = every;
  g->xchg_scale = scale;
  g->calls = 0;
  return NFSP_OK;
}

// ---------------------------------------------------------------------------
// group_update: one learner call of every replica, a sequence of stages over a GroupCall
// ---------------------------------------------------------------------------
// How the call's BR work is scheduled (nfsp_group_sched and the group's shape)
struct BrSched {
  int64_t cap;         // updates per piece of a segment at most (0: whole segments)
  bool pace;           // paced pieces (group_plan.h)
  bool shared_cus;     // the chains share CUs (R > 64)
  bool persist;        // k_br_persist instead of the rounds
  int nbs;             // partitions (BR streams)
};

static BrSched group_br_sched(const nfsp_group* g, bool loss_log) {
  const nfsp_engine* e0 = g->eng[0];
  BrSched sc{};
  // Capped pieces (group_plan.h plan_rounds): sliced groups only, whose rounds are short
  sc.cap = g->sched.br_cap >= 0 ? g->sched.br_cap : (e0->slices > 1 ? 40 : 0);
  sc.pace = g->sched.br_pace != 0;
  sc.shared_cus = g->chain_lds < CHAIN_LDS;
  // The persistent BR kernel (sched.br_persist) instead of the rounds: one launch, one stream,
  // the reference's BR net (k_chain3<1>), no loss log, its 2R chains and BRP_HELPERS helpers
  // (br_persist.hip) a CU each beside the 2R AR chains (R <= 32, no CU sharing), and one gamma,
  // lr_br and quirks for the launch: replicas that differ in them keep the rounds
  sc.persist = g->sched.br_persist && !loss_log && !(e0->cfg.quirks & NFSP_EXT_LINEAR_Q) && g->R <= 32 &&
               !sc.shared_cus && g->br_uniform;
  // Partitions: replicas [part_begin(p), part_begin(p + 1)) are partition p, whose BR jobs run
  // their own rounds on their own stream, followed (pipelined) by the partition's BR results and
  // BR snapshot on that stream.  A round then waits only for the longest piece among its
  // partition's jobs, and one partition's targets overlap the others' chains.  Partitions
  // 1.. go on into the next slice without waiting for the others; partition 0 runs on s_br,
  // which joins every partition at the end of the call (group_finish), so its next-slice rounds
  // wait for the slowest partition: the overlap is asymmetric.  Sliced groups only (their rounds
  // are short: the targets between them were ~10% of c4_emul_r8's BR stream); groups whose
  // chains share CUs keep one stream.
  int nbs = g->sched.br_streams > 0 ? g->sched.br_streams : (e0->slices > 1 ? 2 : 1);
  nbs = nbs > GROUP_BR_STREAMS ? GROUP_BR_STREAMS : nbs;
  nbs = nbs > g->R ? g->R : nbs;
  if (sc.shared_cus || sc.persist) nbs = 1;
  sc.nbs = nbs;
  return sc;
}

// the call's tables on device (one copy from the pinned host set; TabCursor: learner_internal.h)
struct GroupTabs {
  size_t bytes = 0;
  const PrepArgs* prep = nullptr;   // [R]
  const FinalArgs* fin = nullptr;   // [R]
  const ChainJob* ar = nullptr;     // the AR chains
  const ChainJob* br = nullptr;     // the rounds' pieces
  const TargetJob* tg = nullptr;    // the rounds' targets
};

struct GroupCall {
  nfsp_group* g;
  bool pipelined;
  int par;
  bool snap_after;
  bool loss_log = false;
  std::vector<LearnPlan> L;         // [R]
  std::vector<ChainJob> ar_jobs;    // every (replica, agent) with AR updates: 2R workgroups, one launch
  bool ar_launched = false;
  BrSched sc{};
  plan::RoundsPlan rounds;          // the BR work: rounds of pieces and targets, or
  plan::PersistPlan pq;             //   (sc.persist) k_br_persist's segments and work queue
  GroupTabs T;
  BrpTabs PT{};                     // (sc.persist) its tables' offsets in the set
  hipEvent_t fork_br = nullptr, fork = nullptr;   // the BR rows / the AR records are prepared
  hipStream_t sp[GROUP_BR_STREAMS] = {};          // the partitions' streams
};

// stage 1a: the trigger plans need every replica's insert counts: one gather, one readback
static int group_readback(nfsp_group* g) {
  hipStream_t s = g->ctx->stream;
  for (int r = 0; r < g->R; ++r) NFSP_REQUIRE(g->eng[r]->pending_update, "group replica without a rollout");
  const int rc = launch_gather_st(g->d_stp, g->d_st, g->R, s);
  if (rc != NFSP_OK) return rc;
  NFSP_HIP(hipMemcpyAsync(g->h_st, g->d_st, sizeof(EngineDev) * g->R, hipMemcpyDeviceToHost, s));
  NFSP_HIP(hipStreamSynchronize(s));
  // br_persist.h: the ctx stream has waited for every earlier slice's BR stream, so a persistent
  // kernel that bailed has completed
  return brp_flags_take(g->h_err);
}

// stage 1b: every replica's plan.  Replica 0's cfg stands for the fields every replica shares
// (batch, epochs, the LINEAR_Q / MSE_Q quirk bits; group_uniform_diff).  What may differ --
// target_every, lr_*, gamma, epsilon, eta, the other quirks, the seed -- is read from each
// replica's own cfg: by plan_update (the segments and schedules, PrepArgs) and br_target_job
// (the targets' gamma, lr0, quirks)
static int group_plans(GroupCall& c) {
  nfsp_group* g = c.g;
  const int R = g->R;
  c.L.resize(R);
  c.loss_log = g->eng[0]->log_loss;
  int rc;
  for (int r = 0; r < R; ++r) {
    nfsp_engine* e = g->eng[r];
    NFSP_REQUIRE(e->log_loss == c.loss_log, "the loss log must be on in all replicas of a group or none");
    if ((rc = plan_update(e, c.par, g->h_st[r], c.L[r])) != NFSP_OK) return rc;
  }
  // every plan succeeded: the rollouts are consumed and the schedules advance (a failed
  // plan leaves every replica as it was -- pending, schedules untouched -- so they stay in step)
  for (int r = 0; r < R; ++r) commit_plan(g->eng[r], c.L[r]);
  if (g->trace_on)
    for (int r = 0; r < R; ++r)
      for (int a = 0; a < 2; ++a) {
        g->trace.push_back((int32_t)c.L[r].P.A[a].U);
        g->trace.push_back((int32_t)c.L[r].P.A[a].U_br);
      }
  for (int r = 0; r < R; ++r)
    for (int a = 0; a < 2; ++a)
      if (c.L[r].P.A[a].U > 0) c.ar_jobs.push_back(ar_job(g->eng[r], c.L[r], a));
  c.ar_launched = c.ar_jobs.empty();
  return NFSP_OK;
}

// stage 2: the BR work (group_plan.h): rounds per partition, or k_br_persist's queue
static int group_plan_br(GroupCall& c) {
  nfsp_group* g = c.g;
  c.sc = group_br_sched(g, c.loss_log);
  plan::Jobs jobs((size_t)2 * g->R);
  for (int r = 0; r < g->R; ++r)
    for (int a = 0; a < 2; ++a) jobs[2 * r + a] = &c.L[r].seg[a];
  if (c.sc.persist) {
    const char* msg = nullptr;
    if (plan::plan_persist(jobs, g->R, BRP_CHUNK, c.pq, &msg) != 0) return nfsp::fail(NFSP_EINVAL, msg);
    g->rounds = c.pq.jseg0.size() > 1 ? 1 : 0;
  } else {
    plan::plan_rounds(jobs, g->R, c.sc.nbs, c.sc.cap, c.sc.pace, c.rounds);
    g->rounds = c.rounds.max_rounds;
  }
  return NFSP_OK;
}

// Table set `par` with room for `need` bytes.  Every earlier use of the set has completed:
// serially, the call starts with the readback's sync; pipelined, the ctx stream waited for slice
// j - 2's snapshot events (after its chains) before this slice's rollout.  A grown set is freed
// and reallocated: the device free synchronises the device.
static int group_tab_reserve(nfsp_group* g, int par, size_t need) {
  if (need <= g->tab_cap[par]) return NFSP_OK;
  char*& h_tab = g->h_tab[par];
  char*& d_tab = g->d_tab[par];
  if (h_tab) NFSP_HIP(hipHostFree(h_tab));
  if (d_tab) NFSP_HIP(hipFree(d_tab));
  h_tab = nullptr;
  d_tab = nullptr;
  g->tab_cap[par] = 0;
  NFSP_HIP(hipHostMalloc((void**)&h_tab, need * 2, hipHostMallocDefault));
  NFSP_HIP(hipMalloc((void**)&d_tab, need * 2));
  g->tab_cap[par] = need * 2;
  return NFSP_OK;
}

// stage 3: lay out the call's table set `par` and fill its host side: prep / final args per
// replica, the AR chains, per BR round its chains' and targets' jobs, k_br_persist's tables
static int group_fill_tables(GroupCall& c) {
  nfsp_group* g = c.g;
  const int R = g->R;
  const std::vector<plan::Piece>& pc = c.rounds.pieces;
  const std::vector<plan::SegRef>& tg = c.rounds.targets;
  TabCursor cur;
  const size_t o_prep = cur.take<PrepArgs>(R), o_fin = cur.take<FinalArgs>(R);
  const size_t o_ar = cur.take<ChainJob>(c.ar_jobs.size()), o_br = cur.take<ChainJob>(pc.size());
  const size_t o_tg = cur.take<TargetJob>(tg.size());
  c.PT = brp_tabs_take(cur, c.pq);               // br_persist.h (an empty plan unless sc.persist)
  const size_t need = cur.off;
  int rc;
  if ((rc = group_tab_reserve(g, c.par, need)) != NFSP_OK) return rc;
  char* h_tab = g->h_tab[c.par];
  char* d_tab = g->d_tab[c.par];
  auto seg_of = [&](const plan::SegRef& t) -> const Segment& { return c.L[t.r].seg[t.a][t.seg]; };
  for (int r = 0; r < R; ++r) {
    tab_at<PrepArgs>(h_tab, o_prep)[r] = c.L[r].P;
    tab_at<FinalArgs>(h_tab, o_fin)[r] = c.L[r].F;
  }
  if (!c.ar_jobs.empty()) memcpy(h_tab + o_ar, c.ar_jobs.data(), sizeof(ChainJob) * c.ar_jobs.size());
  for (size_t i = 0; i < pc.size(); ++i)
    tab_at<ChainJob>(h_tab, o_br)[i] =
        br_chain_job(g->eng[pc[i].r], c.L[pc[i].r], pc[i].a, Segment{pc[i].u, pc[i].v, pc[i].sync});
  for (size_t i = 0; i < tg.size(); ++i)
    tab_at<TargetJob>(h_tab, o_tg)[i] = br_target_job(g->eng[tg[i].r], c.L[tg[i].r], tg[i].a, seg_of(tg[i]));
  if (c.sc.persist) brp_tabs_fill(h_tab, c.PT, c.pq, g->eng.data(), c.L.data());   // br_persist.h
  GroupTabs& T = c.T;
  T.bytes = need;
  T.prep = tab_at<const PrepArgs>(d_tab, o_prep);
  T.fin = tab_at<const FinalArgs>(d_tab, o_fin);
  T.ar = tab_at<const ChainJob>(d_tab, o_ar);
  T.br = tab_at<const ChainJob>(d_tab, o_br);
  T.tg = tab_at<const TargetJob>(d_tab, o_tg);
  return NFSP_OK;
}

// stage 5: the AR chains (one launch) on the AR stream, behind the AR prep and `after` (if any)
static int group_launch_ar(GroupCall& c, hipEvent_t after) {
  nfsp_group* g = c.g;
  NFSP_HIP(hipStreamWaitEvent(g->s_ar, c.fork, 0));
  if (after) NFSP_HIP(hipStreamWaitEvent(g->s_ar, after, 0));
  c.ar_launched = true;
  KTimer kc(g->eng[0], KT_CHAIN_AR, g->s_ar);
  return launch_chain_ar(chain_args(g->eng[0]->cfg, c.T.ar, g->chain_lds), (int)c.ar_jobs.size(), c.loss_log,
                         g->s_ar);
}

// the partitions' streams (created on first use), each behind the BR prep
static int group_fork_br(GroupCall& c) {
  nfsp_group* g = c.g;
  for (int p = 1; p < c.sc.nbs; ++p)
    if (!g->s_brp[p - 1]) NFSP_HIP(hipStreamCreateWithFlags(&g->s_brp[p - 1], hipStreamNonBlocking));
  c.sp[0] = g->s_br;
  for (int p = 1; p < GROUP_BR_STREAMS; ++p) c.sp[p] = g->s_brp[p - 1];
  for (int p = 0; p < c.sc.nbs; ++p) NFSP_HIP(hipStreamWaitEvent(c.sp[p], c.fork_br, 0));
  return NFSP_OK;
}

// stage 6, persist: the whole BR call in one launch on s_br (br_persist.h)
static int group_launch_persist(GroupCall& c) {
  nfsp_group* g = c.g;
  if (!g->rounds) return NFSP_OK;               // no BR work (group_plan_br): nothing to time
  KTimer kc(g->eng[0], KT_CHAIN_BR, g->s_br);
  return brp_launch(g->d_tab[c.par], c.PT, c.pq, g->eng[0]->cfg, g->sched.br_persist, g->h_err, g->s_br);
}

// stage 6, rounds: per round its targets launch and its chain launch on the partition's stream.
// When chains share CUs (R > 64), the first round's BR targets run before the AR chains
// start: alone they take the chip's issue slots instead of competing with 2R resident AR
// chains, and the BR stream is the longer one at that size.  (No data dependency.)
static int group_launch_rounds(GroupCall& c) {
  nfsp_group* g = c.g;
  nfsp_engine* e0 = g->eng[0];
  const nfsp_engine_cfg& cfg = e0->cfg;
  int rc;
  for (const plan::Round& rd : c.rounds.rounds) {
    hipStream_t st = c.sp[rd.p];
    const int nj = (int)(rd.b1 - rd.b0);
    const int nt = (int)(rd.t1 - rd.t0);
    if (nt > 0) {
      {
        KTimer kt2(e0, KT_TARGETS, st);
        rc = launch_br_targets(c.T.tg + rd.t0, TargetJob{}, rd.rn, nt, cfg.batch, cfg.epochs, st);
      }
      if (rc != NFSP_OK) return rc;
    }
    if (!c.ar_launched) {                    // (one partition: shared_cus)
      hipEvent_t t0 = take_event(e0);
      NFSP_HIP(hipEventRecord(t0, st));
      if ((rc = group_launch_ar(c, t0)) != NFSP_OK) return rc;
      e0->pool.push_back(t0);
    }
    KTimer kc(e0, KT_CHAIN_BR, st);
    if ((rc = launch_br_chain(chain_args(cfg, c.T.br + rd.b0, g->chain_lds), nj, cfg.quirks, c.loss_log, st)) !=
        NFSP_OK)
      return rc;
  }
  return NFSP_OK;
}

// stage 7.  Each partition's stream: (pipelined) its replicas' BR results, then (snap_after)
// their BR / target nets and epsilons into snapshot `par`; then the partitions are joined on
// s_br.  Pipelined, nothing joins the ctx stream; else the learner streams do and the results
// are published on it.
static int group_finish(GroupCall& c) {
  nfsp_group* g = c.g;
  nfsp_engine* e0 = g->eng[0];
  const int R = g->R, par = c.par;
  int rc;
  for (int p = 0; p < c.sc.nbs; ++p) {
    const int r0 = plan::part_begin(p, R, c.sc.nbs), rn = plan::part_begin(p + 1, R, c.sc.nbs) - r0;
    if (c.pipelined && rn > 0) {
      if ((rc = launch_finalize_table(c.T.fin + r0, rn, 6, c.sp[p])) != NFSP_OK) return rc;
      if (c.snap_after &&
          (rc = group_snap_part_launch(g->eng.data() + r0, rn, g->d_roll, par, 1, c.sp[p], r0)) != NFSP_OK)
        return rc;
    }
    if (p > 0 && (rc = join_into(e0, g->s_br, {c.sp[p]})) != NFSP_OK) return rc;
  }
  if (c.pipelined) {
    if (c.snap_after) NFSP_HIP(hipEventRecord(g->snap_ev[par][1], g->s_br));
    // AR stream: the exchange when due (after this call's AR chains; AR nets only, so no other
    // stream touches what it writes), then the AR nets into snapshot `par`
    NFSP_HIP(hipStreamWaitEvent(g->s_ar, c.fork, 0));
    if (g->xchg_every > 0 && (++g->calls) % g->xchg_every == 0 && (rc = group_xchg_launch(g, g->s_ar)) != NFSP_OK)
      return rc;
    if (c.snap_after) {
      if ((rc = group_snap_part_launch(g->eng.data(), R, g->d_roll, par, 0, g->s_ar)) != NFSP_OK) return rc;
      NFSP_HIP(hipEventRecord(g->snap_ev[par][0], g->s_ar));
    }
    e0->pool.push_back(c.fork);
    e0->pool.push_back(c.fork_br);
    return NFSP_OK;
  }
  if ((rc = join_into(e0, g->ctx->stream, {g->s_ar, g->s_br})) != NFSP_OK) return rc;
  e0->pool.push_back(c.fork);
  e0->pool.push_back(c.fork_br);
  return launch_finalize_table(c.T.fin, R, 7, g->ctx->stream);
}

// One learner call of every replica for their pending rollouts.  par: the learner-buffer and
// table set (slice parity; 0 unless pipelined).  pipelined (nfsp_group_step at slice_lag 2):
// nothing joins the ctx stream -- the counters are published on it after the prep, the BR
// results on the BR stream after the last round; the exchange (when due) follows the AR chains
// on the AR stream; with snap_after each learner stream then copies its nets into snapshot
// `par` and records snap_ev[par] for the rollout two slices on.
static int group_update(nfsp_group* g, bool pipelined = false, int par = 0, bool snap_after = false) {
  hipStream_t s = g->ctx->stream;
  nfsp_engine* e0 = g->eng[0];
  int rc;
  if ((rc = group_readback(g)) != NFSP_OK) return rc;
  KTimer kt(e0, KT_LEARNER);
  GroupCall c{g, pipelined, par, snap_after};
  if ((rc = group_plans(c)) != NFSP_OK) return rc;
  if ((rc = group_plan_br(c)) != NFSP_OK) return rc;
  if ((rc = group_fill_tables(c)) != NFSP_OK) return rc;
  c.fork_br = take_event(e0);
  c.fork = take_event(e0);
  {                                    // stage 4: the tables' copy and the prep, on the ctx stream
    KTimer kprep(e0, KT_PREP);
    NFSP_HIP(hipMemcpyAsync(g->d_tab[par], g->h_tab[par], c.T.bytes, hipMemcpyHostToDevice, s));
    if ((rc = launch_prep_table(g->eng.data(), c.L.data(), g->R, c.T.prep, c.fork_br, c.fork, s)) != NFSP_OK)
      return rc;
  }
  // the counters, before the next rollout's commit
  if (pipelined && (rc = launch_finalize_table(c.T.fin, g->R, 1, s)) != NFSP_OK) return rc;
  // the AR chains first, unless the chains share CUs (group_launch_rounds)
  if (!c.sc.shared_cus && !c.ar_launched && (rc = group_launch_ar(c, nullptr)) != NFSP_OK) return rc;
  if ((rc = group_fork_br(c)) != NFSP_OK) return rc;
  KTimer kspan(e0, KT_BR_STREAM0, g->s_br);     // the group's BR streams, end to end (joined on s_br)
  if ((rc = c.sc.persist ? group_launch_persist(c) : group_launch_rounds(c)) != NFSP_OK) return rc;
  if (!c.ar_launched && (rc = group_launch_ar(c, nullptr)) != NFSP_OK) return rc;
  return group_finish(c);
}

extern "C" int nfsp_group_set_timing(nfsp_group* g, int on) {
  NFSP_REQUIRE(g, "null argument");
  for (nfsp_engine* e : g->eng) e->timing = on != 0;
  return NFSP_OK;
}

// the replicas' rollout / prep marks and the group's shared launches (kept on replica 0)
extern "C" int nfsp_group_get_timings(nfsp_group* g, double* ms, int64_t* launches) {
  NFSP_REQUIRE(g && ms && launches, "null argument");
  for (int k = 0; k < KT_N; ++k) { ms[k] = 0.0; launches[k] = 0; }
  for (nfsp_engine* e : g->eng) {
    double m[KT_N];
    int64_t n[KT_N];
    const int rc = nfsp_engine_get_timings(e, m, n);
    if (rc != NFSP_OK) return rc;
    for (int k = 0; k < KT_N; ++k) { ms[k] += m[k]; launches[k] += n[k]; }
  }
  return NFSP_OK;
}

// Every slice: rollout, then its learner, then (when due) the exchange.  With slice_lag 2 the
// slices run one after another, but slice j acts with snapshot j & 1: the nets and epsilon as
// slice j - 2's learner (and exchange) left them, the step's start for j < 2 -- a pipelined
// engine's arithmetic (step_pipelined).
extern "C" int nfsp_group_step(nfsp_group* g) {
  NFSP_REQUIRE(g, "null argument");
  int rc;
  g->w0_loaded = 0;                     // the nets move on: a later set_exchange starts over
  if (g->xchg_nets & ~g->w0_valid)      // common nets before the first exchange
    if ((rc = nfsp_group_average_ar(g)) != NFSP_OK) return rc;
  const int K = g->eng[0]->slices;
  const bool lag2 = g->eng[0]->slice_lag == 2 && K > 1;
  // Pipelined (as step_pipelined): slice j's rollout waits only for the snapshot copies of
  // slice j - 2, so the rollout, readback, plan and prep of slice j + 1 overlap slice j's
  // chains.  The same arithmetic as the serial loop below.  Not with a BR exchange (it would
  // need both learner streams joined after every exchange) or sched.serial.
  if (lag2 && !(g->xchg_nets & NFSP_XCHG_BR) && !g->sched.serial) {
    hipStream_t s = g->ctx->stream;
    if ((rc = nfsp::eng::group_snap_launch(g->eng.data(), g->R, g->d_roll, -1)) != NFSP_OK) return rc;
    for (int j = 0; j < K; ++j) {
      const int par = j & 1;
      if (j >= 2)
        for (hipEvent_t ev : g->snap_ev[par]) NFSP_HIP(hipStreamWaitEvent(s, ev, 0));
      if ((rc = nfsp::eng::group_rollout_launch(g->eng.data(), g->R, g->d_roll, par)) != NFSP_OK) return rc;
      if ((rc = group_update(g, true, par, j + 2 < K)) != NFSP_OK) return rc;
    }
    return join_into(g->eng[0], s, {g->s_ar, g->s_br});    // the step ends with every stream joined
  }
  if (lag2 && (rc = nfsp::eng::group_snap_launch(g->eng.data(), g->R, g->d_roll, -1)) != NFSP_OK) return rc;
  for (int j = 0; j < K; ++j) {
    if ((rc = nfsp::eng::group_rollout_launch(g->eng.data(), g->R, g->d_roll, lag2 ? (j & 1) : -1)) != NFSP_OK)
      return rc;
    if ((rc = group_update(g)) != NFSP_OK) return rc;
    if (g->xchg_every > 0 && (++g->calls) % g->xchg_every == 0 && (rc = nfsp_group_average_ar(g)) != NFSP_OK)
      return rc;
    if (lag2 && j + 2 < K && (rc = nfsp::eng::group_snap_launch(g->eng.data(), g->R, g->d_roll, j & 1)) != NFSP_OK)
      return rc;
  }
  return NFSP_OK;
}

namespace {
int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}
}  // namespace

extern "C" int nfsp_group_default_sched(nfsp_group_sched* out) {
  NFSP_REQUIRE(out, "null argument");
  out->br_cap = env_int("NFSP_GROUP_BR_CAP", -1);
  out->br_pace = env_int("NFSP_GROUP_BR_PACE", 1) != 0;
  out->br_streams = env_int("NFSP_GROUP_BR_STREAMS", -1);
  out->serial = env_int("NFSP_GROUP_SERIAL", 0) != 0;
  out->br_persist = env_int("NFSP_GROUP_BR_PERSIST", 0);
  return NFSP_OK;
}

extern "C" int nfsp_group_set_sched(nfsp_group* g, const nfsp_group_sched* sc) {
  NFSP_REQUIRE(g && sc, "null argument");
  NFSP_REQUIRE(sc->br_cap >= -1, "br_cap must be >= -1");
  NFSP_REQUIRE(sc->br_streams == -1 || (sc->br_streams >= 1 && sc->br_streams <= GROUP_BR_STREAMS),
               "br_streams must be -1 or in [1, 4]");
  NFSP_REQUIRE(sc->br_persist >= 0, "br_persist must be >= 0");
  g->sched = *sc;
  g->sched.br_pace = sc->br_pace != 0;
  g->sched.serial = sc->serial != 0;
  return NFSP_OK;
}

extern "C" int nfsp_group_get_sched(nfsp_group* g, nfsp_group_sched* out) {
  NFSP_REQUIRE(g && out, "null argument");
  *out = g->sched;
  return NFSP_OK;
}


extern "C" int nfsp_group_check(nfsp_group* g) {
  NFSP_REQUIRE(g, "null argument");
  const int rc = group_sync(g);
  return rc != NFSP_OK ? rc : brp_flags_take(g->h_err);   // br_persist.h
}

extern "C" int nfsp_group_rounds(nfsp_group* g, int64_t* out) {
  NFSP_REQUIRE(g && out, "null argument");
  *out = g->rounds;
  return NFSP_OK;
}

extern "C" int nfsp_group_set_trace(nfsp_group* g, int on) {
  NFSP_REQUIRE(g, "null argument");
  g->trace_on = on != 0;
  g->trace.clear();
  return NFSP_OK;
}

extern "C" int nfsp_group_trace(nfsp_group* g, int32_t* out, int64_t cap, int64_t* n) {
  NFSP_REQUIRE(g && n && cap >= 0 && (out || cap == 0), "bad argument");
  const int64_t m = (int64_t)g->trace.size();
  for (int64_t i = 0; i < m && i < cap; ++i) out[i] = g->trace[i];
  *n = m;
  return NFSP_OK;
}
