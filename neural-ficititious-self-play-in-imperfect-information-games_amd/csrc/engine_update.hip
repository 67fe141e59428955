// One engine's learner call (nfsp_engine_update; nfsp_engine_step's slices): the plan of the
// call (learn_plan.h) wired to the engine's buffers, the jobs of its chains and targets, and
// the sequence of launches on the engine's four streams.  Host code only: the kernels and their
// launchers are learner.hip's (learner_internal.h), the group's form of the call is group.hip.
#include "learner_internal.h"

namespace nn = nfsp::nn;
using namespace nfsp::eng;
using namespace nfsp::chain;

namespace nfsp {
namespace eng {

int plan_update(const nfsp_engine* e, int par, const EngineDev& h, LearnPlan& L) {
  const nfsp_engine_cfg& cfg = e->cfg;
  const LearnBufs& LB = e->LBs[par];
  L.par = par;
  PrepArgs& P = L.P;
  P = PrepArgs{};
  P.M = e->M;
  P.LB = LB;
  P.st = e->st;
  P.c = cfg.inserts_per_update;
  P.rl_cap = cfg.rl_capacity;
  P.B = cfg.batch;
  P.E = cfg.epochs;
  P.k0 = (uint32_t)cfg.seed;
  P.k1 = (uint32_t)(cfg.seed >> 32);
  P.tag = e->learn_tag + 1;
  P.lr_ar = cfg.lr_ar;
  P.quirks = cfg.quirks;
  FinalArgs& F = L.F;
  F = FinalArgs{};
  F.st = e->st;
  F.br_expl = LB.br_expl;
  F.umax = LB.umax;
  F.sl_cap = cfg.sl_capacity;
  const plan::Cadence cad{cfg.inserts_per_update, cfg.batch, cfg.target_every, cfg.epsilon, cfg.lr_br,
                          (cfg.quirks & NFSP_EXT_EPS_CONST) != 0};
  L.maxU = L.maxUbr = L.maxSL = 0;
  for (int a = 0; a < 2; ++a) {
    // the schedules from the host's mirror (the device copy in EngineDev, written by
    // k_finalize, may still be in flight with cfg.slice_lag 2)
    const plan::AgentSched hs{e->hs.iteration[a], e->hs.target_count[a], e->hs.target_syncs[a], e->hs.epsilon[a]};
    plan::AgentLearn al;
    NFSP_REQUIRE(plan::plan_agent({h.rl_total[a], h.last_rl[a], h.sl_total[a], h.last_sl[a]}, hs, cad, LB.umax,
                                  e->update_limit, al),
                 "update plan exceeds the learner buffers");
    const AgentPlan& pl = P.A[a] = al.A;
    L.maxU = pl.U > L.maxU ? pl.U : L.maxU;
    L.maxUbr = pl.U_br > L.maxUbr ? pl.U_br : L.maxUbr;
    L.maxSL = pl.n_sl > L.maxSL ? pl.n_sl : L.maxSL;
    L.seg[a] = al.seg;
    L.ar_u1[a] = al.ar_u1;
    L.it0[a] = al.it0;
    F.n_rl[a] = h.last_rl[a];
    F.n_sl[a] = pl.n_sl;
    F.U_br[a] = pl.U_br;
    F.iteration[a] = L.hs.iteration[a] = al.after.iteration;
    F.tcount[a] = L.hs.target_count[a] = al.after.target_count;
    F.syncs[a] = L.hs.target_syncs[a] = al.after.target_syncs;
    F.eps[a] = L.hs.epsilon[a] = al.after.epsilon;
    F.temp[a] = al.temp;
    F.lr[a] = al.lr;
  }
  return NFSP_OK;
}

void commit_plan(nfsp_engine* e, const LearnPlan& L) {
  e->learn_tag = L.P.tag;
  e->hs = L.hs;
  e->last_par = L.par;
  for (int a = 0; a < 2; ++a) {
    e->last_U[a] = L.P.A[a].U;
    e->last_Ubr[a] = L.P.A[a].U_br;
  }
  e->pending_update = false;
}

static int64_t recs_per_update(const nfsp_engine* e) { return engine_sizes(e->cfg).steps; }

ChainJob ar_job(const nfsp_engine* e, const LearnPlan& L, int a) {
  const LearnBufs& LB = L.P.LB;
  const int64_t um = LB.umax;
  ChainJob j{};
  j.w = e->w + (a * 3 + 0) * nn::NP;
  j.sync_to = nullptr;
  j.snap_to = nullptr;
  j.rec = LB.ar_rec + a * um * recs_per_update(e);
  j.active = LB.ar_active + a * um;
  j.loss_out = e->log_loss ? LB.ar_loss + a * um * e->cfg.epochs : nullptr;
  j.u0 = 0;
  j.u1 = L.ar_u1[a];
  return j;
}

TargetJob br_target_job(const nfsp_engine* e, const LearnPlan& L, int a, const Segment& sg) {
  const LearnBufs& LB = L.P.LB;
  const int64_t um = LB.umax, B = e->cfg.batch, E = e->cfg.epochs;
  TargetJob t{};
  t.rows = LB.br_rows + a * um * B;
  t.perm = LB.br_perm + a * um * E * B;
  t.expl = LB.br_expl + a * um;
  t.rec = LB.br_rec + a * um * recs_per_update(e);
  t.tw = e->w + (a * 3 + 2) * nn::NP;
  t.u0 = sg.u;
  t.n = sg.v - sg.u;
  t.it0 = L.it0[a];
  t.gamma = e->cfg.gamma;
  t.lr0 = e->cfg.lr_br;
  t.quirks = e->cfg.quirks;
  return t;
}

ChainJob br_chain_job(const nfsp_engine* e, const LearnPlan& L, int a, const Segment& sg) {
  const LearnBufs& LB = L.P.LB;
  const int64_t um = LB.umax;
  ChainJob j{};
  j.w = e->w + (a * 3 + 1) * nn::NP;
  j.sync_to = sg.sync ? e->w + (a * 3 + 2) * nn::NP : nullptr;
  j.snap_to = nullptr;
  j.rec = LB.br_rec + a * um * recs_per_update(e);
  j.active = nullptr;
  j.loss_out = e->log_loss ? LB.br_loss + a * um * e->cfg.epochs : nullptr;
  j.u0 = sg.u;
  j.u1 = sg.v;
  return j;
}

int join_into(nfsp_engine* e, hipStream_t dst, std::initializer_list<hipStream_t> streams) {
  for (hipStream_t st : streams) {
    hipEvent_t j = take_event(e);
    NFSP_HIP(hipEventRecord(j, st));
    NFSP_HIP(hipStreamWaitEvent(dst, j, 0));
    e->pool.push_back(j);      // reusable once the wait is enqueued
  }
  return NFSP_OK;
}

}  // namespace eng
}  // namespace nfsp

// `count` nets from net `first` of the engine's [2 agents][3: AR, BR, target] as they are now
// -> snapshot `par`, on stream s
static int snap_nets(nfsp_engine* e, int par, int first, int count, hipStream_t s) {
  NFSP_HIP(hipMemcpyAsync(e->snap + ((size_t)par * 6 + first) * nn::NP, e->w + (size_t)first * nn::NP,
                          sizeof(float) * count * nn::NP, hipMemcpyDeviceToDevice, s));
  return NFSP_OK;
}

// The exchange a pipelined learner call left pending (nfsp_engine_set_exchange), enqueued on
// the AR stream behind that call's AR chain, then the AR snapshot it feeds and its event.
static int flush_exchange(nfsp_engine* e) {
  if (!e->xchg_pending) return NFSP_OK;
  e->xchg_pending = false;
  int rc;
  {
    KTimer kx(e, KT_XCHG, e->s_ar);
    if ((rc = exchange_enqueue(e, e->s_ar)) != NFSP_OK) return rc;
  }
  if (e->xchg_pend_snap) {
    for (int a = 0; a < 2; ++a)
      if ((rc = snap_nets(e, e->xchg_pend_par, a * 3 + 0, 1, e->s_ar)) != NFSP_OK) return rc;
    NFSP_HIP(hipEventRecord(e->snap_ev[e->xchg_pend_par][0], e->s_ar));
  }
  return NFSP_OK;
}

// One learner call for the pending rollout, as a sequence of stages over this struct.  par: the
// learner-buffer set (slice parity; 0 unless cfg.slice_lag 2).  pipelined: leave the chains
// running (no join into the ctx stream; each BR stream publishes its agent's results itself),
// and when snap_after, copy the nets into snapshot `par` after the chains and record
// snap_ev[par] for the rollout two slices on (step_pipelined).
struct UpdateCall {
  nfsp_engine* e;
  bool pipelined;
  int par;
  bool snap_after;
  LearnPlan L;
  bool xchg = false;         // the cross-shard exchange follows this call's AR chain
  bool serial_ar = false;    // diagnostic (cfg.sched NFSP_SCHED_LEARNER_SERIAL): BR work waits for
                             // the AR chains, to time them alone
  hipEvent_t fork_br = nullptr, fork = nullptr;   // the BR rows / the AR records are prepared
  hipEvent_t ar_done = nullptr;                   // serial_ar: the AR chains have run
  float* snap() const { return e->snap + (size_t)par * 6 * nn::NP; }
};

// stage 1: the trigger plan needs the rollout's insert counts: one small readback
static int update_readback(nfsp_engine* e, EngineDev& h) {
  hipStream_t s = e->ctx->stream;
  NFSP_HIP(hipMemcpyAsync(&h, e->st, sizeof(h), hipMemcpyDeviceToHost, s));
  NFSP_HIP(hipStreamSynchronize(s));
  return NFSP_OK;
}

// stage 2: the plan; the rollout is consumed and the schedules advance
static int update_plan(UpdateCall& c, const EngineDev& h) {
  nfsp_engine* e = c.e;
  const int rc = plan_update(e, c.par, h, c.L);
  if (rc != NFSP_OK) return rc;
  commit_plan(e, c.L);
  c.xchg = e->xchg_every > 0 && (++e->xchg_calls) % e->xchg_every == 0;
  c.serial_ar = (e->cfg.sched & NFSP_SCHED_LEARNER_SERIAL) != 0;
  if (c.pipelined && c.snap_after)     // the rollout two slices on acts with this epsilon
    for (int a = 0; a < 2; ++a) e->snap_eps[c.par][a] = e->hs.epsilon[a];
  return NFSP_OK;
}

// stage 3: parallel prep on the ctx stream (launch_prep): the BR streams fork behind the BR rows
// (agent 0's BR segments are the learner's critical path), the AR stream behind the AR records.
// Pipelined: then the counters, before the next rollout's commit
static int update_prep(UpdateCall& c) {
  nfsp_engine* e = c.e;
  hipStream_t s = e->ctx->stream;
  c.fork_br = take_event(e);
  c.fork = take_event(e);
  int rc;
  {
    KTimer kprep(e, KT_PREP);
    if ((rc = launch_prep(e, c.L, c.fork_br, c.fork, s)) != NFSP_OK) return rc;
  }
  return c.pipelined ? launch_finalize(c.L.F, 1, s) : NFSP_OK;
}

// stage 4: the AR chains (both agents, one launch) on their own stream.  With the exchange on and
// the slices pipelined, this call's exchange (and the AR snapshot it feeds) is enqueued by
// the NEXT call, after its prep and BR chains and right before its AR chain (or at the
// step's end): an exchange may hold the host until the AR stream reaches it (RCCL's world-1
// path synchronises the stream), and this way the host has enqueued everything the other
// streams need before it can wait -- the AR stream's next chain needs the exchange anyway.
static int update_ar(UpdateCall& c) {
  nfsp_engine* e = c.e;
  const LearnPlan& L = c.L;
  int r;
  if (c.pipelined && (r = flush_exchange(e)) != NFSP_OK) return r;
  NFSP_HIP(hipStreamWaitEvent(e->s_ar, c.fork, 0));
  if (L.maxU > 0) {
    ChainArgs C = chain_args(e->cfg);
    for (int a = 0; a < 2; ++a) {
      C.job[a] = ar_job(e, L, a);
      if (c.snap_after && !c.xchg) C.job[a].snap_to = c.snap() + (a * 3 + 0) * nn::NP;   // written by the chain
    }
    KTimer kc(e, KT_CHAIN_AR, e->s_ar);
    if ((r = launch_chain_ar(C, 2, e->log_loss, e->s_ar)) != NFSP_OK) return r;
  }
  if (c.xchg) {
    e->xchg_pending = true;
    e->xchg_pend_par = c.par;
    e->xchg_pend_snap = c.snap_after;
    if (!c.pipelined && (r = flush_exchange(e)) != NFSP_OK) return r;
  } else if (c.snap_after) {
    if (L.maxU == 0)                   // no AR chain this call: copy the nets as they are
      for (int a = 0; a < 2; ++a)
        if ((r = snap_nets(e, c.par, a * 3 + 0, 1, e->s_ar)) != NFSP_OK) return r;
    NFSP_HIP(hipEventRecord(e->snap_ev[c.par][0], e->s_ar));
  }
  if (c.serial_ar) {
    c.ar_done = take_event(e);
    NFSP_HIP(hipEventRecord(c.ar_done, e->s_ar));
  }
  return NFSP_OK;
}

// stage 5: BR, per agent on its own stream: segments between target syncs = targets + chain
static int update_br(UpdateCall& c) {
  nfsp_engine* e = c.e;
  const nfsp_engine_cfg& cfg = e->cfg;
  const LearnPlan& L = c.L;
  int r;
  for (int a = 0; a < 2; ++a) {
    hipStream_t sa = e->s_br[a];
    NFSP_HIP(hipStreamWaitEvent(sa, c.serial_ar ? c.ar_done : c.fork_br, 0));
    KTimer kspan(e, KT_BR_STREAM0 + a, sa);     // this agent's BR stream, end to end
    for (size_t gi = 0; gi < L.seg[a].size(); ++gi) {
      const Segment& sg = L.seg[a][gi];
      {
        KTimer kt2(e, KT_TARGETS, sa);
        r = launch_br_targets(nullptr, br_target_job(e, L, a, sg), sg.v - sg.u, 1, cfg.batch, cfg.epochs, sa);
      }
      if (r != NFSP_OK) return r;
      ChainArgs C = chain_args(cfg);
      C.job[0] = br_chain_job(e, L, a, sg);
      if (c.snap_after && gi + 1 == L.seg[a].size())            // the last segment writes the snapshot
        C.job[0].snap_to = c.snap() + (a * 3 + 1) * nn::NP;
      KTimer kc(e, KT_CHAIN_BR, sa);
      if ((r = launch_br_chain(C, 1, cfg.quirks, e->log_loss, sa)) != NFSP_OK) return r;
    }
    // this agent's learner results, after its chain
    if (c.pipelined && (r = launch_finalize(L.F, 2 << a, sa)) != NFSP_OK) return r;
    if (c.snap_after) {
      if (L.seg[a].empty())             // no BR chain this call: copy the net as it is
        if ((r = snap_nets(e, c.par, a * 3 + 1, 1, sa)) != NFSP_OK) return r;
      NFSP_HIP(hipEventRecord(e->snap_ev[c.par][1 + a], sa));
    }
  }
  return NFSP_OK;
}

static int update_impl(nfsp_engine* e, bool pipelined, int par, bool snap_after) {
  if (!e->pending_update) return NFSP_OK;
  EngineDev h;
  int rc = update_readback(e, h);
  if (rc != NFSP_OK) return rc;
  KTimer kt(e, KT_LEARNER);
  UpdateCall c{e, pipelined, par, snap_after};
  if ((rc = update_plan(c, h)) != NFSP_OK) return rc;
  if ((rc = update_prep(c)) != NFSP_OK) return rc;
  // with the exchange on, the BR chains first (they never wait for an exchange), then the AR
  // chain and the exchange (pipelined: the previous call's exchange, then this call's AR chain;
  // else this call's, whose host transport synchronises the AR stream -- the BR streams are
  // busy by then instead of waiting for the host)
  const bool br_first = e->xchg_every > 0 && !c.serial_ar;
  if ((rc = br_first ? update_br(c) : update_ar(c)) != NFSP_OK) return rc;
  if ((rc = br_first ? update_ar(c) : update_br(c)) != NFSP_OK) return rc;
  e->pool.push_back(c.fork);
  e->pool.push_back(c.fork_br);
  if (c.ar_done) e->pool.push_back(c.ar_done);
  if (pipelined) return NFSP_OK;
  // join and publish the schedules
  hipStream_t s = e->ctx->stream;
  if ((rc = join_into(e, s, {e->s_ar, e->s_br[0], e->s_br[1]})) != NFSP_OK) return rc;
  return launch_finalize(c.L.F, 7, s);
}

extern "C" int nfsp_engine_update(nfsp_engine* e) {
  NFSP_REQUIRE(e, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is stepped by nfsp_group_step");
  return update_impl(e, false, 0, false);
}

namespace nfsp {
namespace eng {
// nfsp_engine_step with cfg.slice_lag 2.  Slice j's rollout acts with snapshot j & 1: the
// nets as of the step's start for j < 2, else as the chains of slice j - 2 left them (copied
// on each chain stream right after its chain, so slice j - 1's chains may already run).  The
// ctx stream waits only for those copies, never for the running chains: rollout, readback,
// plan and prep of slice j overlap slice j - 1's chains, which the chain streams follow
// without a gap.  The step ends with every stream joined (stats, weights and the next step
// see all of it).
int step_pipelined(nfsp_engine* e) {
  hipStream_t s = e->ctx->stream;
  const int K = e->slices;
  int rc;
  for (int p = 0; p < 2; ++p) {
    if ((rc = snap_nets(e, p, 0, 6, s)) != NFSP_OK) return rc;
    for (int a = 0; a < 2; ++a) e->snap_eps[p][a] = e->hs.epsilon[a];
  }
  for (int j = 0; j < K; ++j) {
    const int par = j & 1;
    if (j >= 2)
      for (hipEvent_t ev : e->snap_ev[par]) NFSP_HIP(hipStreamWaitEvent(s, ev, 0));
    if ((rc = rollout_launch_with(e, e->snap + (size_t)par * 6 * nn::NP, e->snap_eps[par])) != NFSP_OK)
      return rc;
    if ((rc = update_impl(e, true, par, j + 2 < K)) != NFSP_OK) return rc;
  }
  if ((rc = flush_exchange(e)) != NFSP_OK) return rc;    // the last slice's
  return join_into(e, s, {e->s_ar, e->s_br[0], e->s_br[1]});   // the side streams' work so far
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_engine_snapshot(nfsp_engine* e, int parity, float** dev_w, double* eps) {
  NFSP_REQUIRE(e && dev_w && eps && (parity == 0 || parity == 1), "bad argument");
  NFSP_REQUIRE(e->snap, "the engine has no snapshots (cfg.slice_lag 1)");
  *dev_w = e->snap + (size_t)parity * 6 * nn::NP;
  if (e->snap_eps_dev) {               // a group replica: its snapshots' epsilons are on device
    NFSP_HIP(hipMemcpyAsync(eps, e->snap_eps_dev + 2 * parity, 2 * sizeof(double), hipMemcpyDeviceToHost,
                            e->ctx->stream));
    NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
    return NFSP_OK;
  }
  eps[0] = e->snap_eps[parity][0];
  eps[1] = e->snap_eps[parity][1];
  return NFSP_OK;
}

extern "C" int nfsp_engine_set_update_limit(nfsp_engine* e, int64_t max_updates) {
  NFSP_REQUIRE(e && max_updates >= 0, "bad argument");
  e->update_limit = max_updates;
  return NFSP_OK;
}
