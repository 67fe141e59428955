// What learner.hip (the learner's kernels and their host launchers) shares with the host code
// of a learner call -- engine_update.hip (one engine) and group.hip (an engine group): the plain
// structs a call's arguments and tables are built from, the plan of one engine's call and its
// jobs (engine_update.hip), and the launchers.  (The persistent group BR kernel: br_persist.h.)
#pragma once
#include <initializer_list>
#include <vector>

#include "engine_internal.h"
#include "chain3.h"
#include "group_plan.h"

namespace nfsp {
namespace eng {

using AgentPlan = plan::AgentPlan;   // learn_plan.h

struct PrepArgs {
  Memories M;
  LearnBufs LB;
  EngineDev* st;
  AgentPlan A[2];
  int64_t c, rl_cap;
  int B, E;
  uint32_t k0, k1, tag;
  float lr_ar;
  uint32_t quirks;
};

// One (engine, agent) segment: the agent's learner buffers (update u of the learner call at
// index u), the target net, and the segment's update range [u0, u0 + n).
struct TargetJob {
  const BrRow* rows;   // [umax][B]
  const uint8_t* perm; // [umax][E][B]
  double* expl;        // [umax]
  StepRec* rec;        // [umax][E][B / 32]
  const float* tw;     // target net
  int64_t u0, n;
  int64_t it0;         // the agent's iteration count before the learner call
  // the replica's own cfg.gamma / lr_br / quirks: the replicas of a group may differ in them
  // (nfsp_group_create_v), so they travel with the job, not with the launch
  double gamma, lr0;
  unsigned quirks;
};

// bump-allocate n items of T in a call's host / device table pair (16-byte aligned offsets)
struct TabCursor {
  size_t off = 0;
  template <class T>
  size_t take(size_t n) {
    const size_t o = (off + 15) & ~(size_t)15;
    off = o + sizeof(T) * n;
    return o;
  }
};
template <class T>
static T* tab_at(char* base, size_t off) { return reinterpret_cast<T*>(base + off); }

// schedule state after the learner (host-computed values + device-side counters)
struct FinalArgs {
  EngineDev* st;
  const double* br_expl;
  int64_t umax;
  int64_t n_rl[2], n_sl[2], U_br[2];
  int64_t iteration[2], tcount[2], syncs[2];
  double eps[2], temp[2];
  float lr[2];
  int64_t sl_cap;
};

// ---------------------------------------------------------------------------
// host side: one learner call = plan (from the rollout's insert counts) + prep launches +
// chain launches + finalize.  nfsp_engine_update runs them for one engine, the group for
// R engines with their chains in shared launches.
// ---------------------------------------------------------------------------
using Segment = plan::Segment;   // BR updates [u, v) of the learner call; sync: ends with a target sync

struct LearnPlan {
  int par;                   // the learner-buffer set of the call: P.LB = LBs[par]
  PrepArgs P;
  int64_t maxU = 0, maxUbr = 0, maxSL = 0;
  std::vector<Segment> seg[2];
  int64_t ar_u1[2];          // the AR chains' update bound: U, or what the update limit leaves
  int64_t it0[2];
  FinalArgs F;
  nfsp_engine::Sched hs;     // the schedules after this call (commit_plan publishes them)
};

// The learner call's plan (learn_plan.h) from the rollout's insert counts and the host's schedule
// mirror, wired to the engine's memories and its learner-buffer set `par` (slice parity; 0 unless
// cfg.slice_lag 2).  Leaves the engine untouched: commit_plan(e, L) adopts it once every plan of
// the call (a group's replicas) has succeeded, so a failed plan changes no replica's schedules.
int plan_update(const nfsp_engine* e, int par, const EngineDev& h, LearnPlan& L);
void commit_plan(nfsp_engine* e, const LearnPlan& L);

// The jobs read the buffer set from the plan (L.P.LB).
// the AR chain of agent a over the whole learner call
chain::ChainJob ar_job(const nfsp_engine* e, const LearnPlan& L, int a);
// a BR segment of agent a: its targets and its chain
TargetJob br_target_job(const nfsp_engine* e, const LearnPlan& L, int a, const Segment& sg);
chain::ChainJob br_chain_job(const nfsp_engine* e, const LearnPlan& L, int a, const Segment& sg);

// a chain launch's arguments: the cfg's batch and epochs; jobs / lds: a group's device job table
// and LDS per workgroup (one engine: the jobs go into C.job, a CU each)
inline chain::ChainArgs chain_args(const nfsp_engine_cfg& cfg, const chain::ChainJob* jobs = nullptr, int lds = 0) {
  chain::ChainArgs C{};
  C.jobs = jobs;
  C.B = cfg.batch;
  C.E = cfg.epochs;
  C.lds = lds;
  return C;
}

// (engine_update.hip) The work of `streams` so far joined into `dst`: per stream an event of e's
// pool, recorded on it, awaited by dst and returned to the pool (reusable once the wait is enqueued).
int join_into(nfsp_engine* e, hipStream_t dst, std::initializer_list<hipStream_t> streams);

// ---- launchers (learner.hip).  The one-engine form of a kernel takes its arguments by value,
// the table form (_table: engine groups) reads entry blockIdx.z / blockIdx.x of a device table;
// each pair is one function template in learner.hip.
// The parallel prep of a learner call on `s`, in the order the chains need it: the BR rows
// first (the BR segments are the learner's critical path), then fork_br is recorded for the BR
// streams; then the AR records, fork is recorded for the AR stream; the final reservoir last
// (only the next rollout reads it, and it must follow k_ar_prep, which reads the reservoir as
// it was).  With the loss log on, each log is reset (NaN = no fit recorded) behind its prep.
int launch_prep(nfsp_engine* e, const LearnPlan& L, hipEvent_t fork_br, hipEvent_t fork, hipStream_t s);
int launch_prep_table(nfsp_engine* const* eng, const LearnPlan* L, int R, const PrepArgs* tab, hipEvent_t fork_br,
                      hipEvent_t fork, hipStream_t s);
// k_finalize (mode bits: see there) of one engine, or of n table entries
int launch_finalize(const FinalArgs& F, int mode, hipStream_t s);
int launch_finalize_table(const FinalArgs* tab, int n, int mode, hipStream_t s);
// the targets of `njobs` segments of at most `n` updates (jobs: device table; null: `one`)
int launch_br_targets(const TargetJob* jobs, const TargetJob& one, int64_t n, int njobs, int B, int E, hipStream_t s);
int launch_br_chain(const chain::ChainArgs& C, int blocks, unsigned quirks, bool loss_log, hipStream_t s);
// engine groups: the replicas' EngineDev gathered into one array; the exchange (k_group_xchg)
int launch_gather_st(EngineDev* const* src, EngineDev* dst, int R, hipStream_t s);
int launch_group_xchg(float* const* wtab, float* w0, int R, unsigned nets, unsigned bcast, float scale, hipStream_t s);

}  // namespace eng
}  // namespace nfsp
