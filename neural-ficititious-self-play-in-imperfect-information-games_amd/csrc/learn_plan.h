// The plan of one agent's part of a learner call (engine_update.hip plan_update), as a pure host
// function of the rollout's insert counters, the host's schedule mirror and the cfg's cadence:
// which triggers fall in the rollout, which of them have a BR update, where the BR chain is cut
// at target syncs, what the update limit leaves of it, and the schedules after the call
// (agent/agent.py:153, 245-253, 266-273, in the reference's double arithmetic).  Standard
// headers only, so it is tested without a GPU (tests/test_learn_plan.py).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace nfsp {
namespace plan {

struct Segment {
  int64_t u, v;        // BR updates [u, v) of the learner call
  bool sync;           // ends with a target sync
};

struct AgentPlan {
  int64_t P0;          // agent's RL inserts before the last rollout
  int64_t m_first;     // first trigger index (trigger m at RL stream position m * c)
  int64_t U;           // triggers in the last rollout
  int64_t m_br0;       // first trigger with a BR update (position > batch)
  int64_t U_br;
  int64_t n_sl;        // SL records of the last rollout
  int64_t sl_total0;   // SL inserts before the last rollout
};

struct Inserts {       // an agent's EngineDev counters after the rollout, before the learner
  int64_t rl_total, last_rl, sl_total, last_sl;
};
struct AgentSched {    // an agent's schedules (nfsp_engine::Sched)
  int64_t iteration, target_count, target_syncs;
  double epsilon;
};
struct Cadence {       // of the cfg
  int64_t inserts_per_update;
  int32_t batch, target_every;
  double epsilon;
  float lr_br;
  bool eps_const;      // NFSP_EXT_EPS_CONST
};

struct AgentLearn {
  AgentPlan A;
  std::vector<Segment> seg;   // the BR chain between target syncs, what the update limit leaves of it
  int64_t ar_u1;              // the AR chain runs updates [0, ar_u1): U, what the limit leaves of it
  int64_t it0;                // the iteration count before the call
  AgentSched after;           // the schedules after the call: over the whole plan, limit or not
  double temp;                // what k_finalize publishes with them
  float lr;
};

// limit > 0 (test hook, nfsp_engine_set_update_limit): only the first `limit` BR and AR updates
// run.  false, with `out` unspecified: the rollout has more triggers than the learner buffers
// hold (umax).
inline bool plan_agent(const Inserts& n, const AgentSched& s, const Cadence& cfg, int64_t umax, int64_t limit,
                       AgentLearn& out) {
  const int64_t c = cfg.inserts_per_update;
  AgentPlan& pl = out.A;
  pl.P0 = n.rl_total;
  pl.m_first = pl.P0 / c + 1;
  const int64_t m_last = (pl.P0 + n.last_rl) / c;
  pl.U = m_last >= pl.m_first ? m_last - pl.m_first + 1 : 0;
  // BR update iff min(p_m, cap) > batch  <=>  m * c > batch
  pl.m_br0 = pl.m_first > cfg.batch / c + 1 ? pl.m_first : cfg.batch / c + 1;
  pl.U_br = m_last >= pl.m_br0 ? m_last - pl.m_br0 + 1 : 0;
  pl.n_sl = n.last_sl;
  pl.sl_total0 = n.sl_total;
  if (pl.U > umax) return false;
  int64_t it = s.iteration, tc = s.target_count, syncs = s.target_syncs;
  double eps = s.epsilon;
  out.it0 = it;
  // BR segments between target syncs: [u, v) ends after the first update whose
  // target_count % every == 0 (agent/agent.py:266-273)
  out.seg.clear();
  for (int64_t u = 0; u < pl.U_br;) {
    int64_t v = u;
    bool sync = false;
    while (v < pl.U_br) {
      const bool s_here = (tc + v) % cfg.target_every == 0;
      ++v;
      if (s_here) { sync = true; break; }
    }
    out.seg.push_back({u, v, sync});
    u = v;
  }
  // schedules (agent/agent.py:245-253, 266-273) in the reference's double arithmetic
  for (int64_t k = 0; k < pl.U_br; ++k) {
    if (tc % cfg.target_every == 0) syncs++;
    tc++;
    it += 2;
    eps = cfg.eps_const ? cfg.epsilon : eps / (double)it;
  }
  out.ar_u1 = pl.U;
  if (limit > 0) {                     // only a prefix of the updates runs
    std::vector<Segment> kept;
    for (const Segment& sg : out.seg) {
      if (sg.u >= limit) break;
      kept.push_back(sg.v <= limit ? sg : Segment{sg.u, limit, false});
    }
    out.seg = kept;
    if (out.ar_u1 > limit) out.ar_u1 = limit;
  }
  out.after = {it, tc, syncs, eps};
  out.temp = 1.0 / (1.0 + 0.02 * sqrt((double)it));
  out.lr = (float)(cfg.lr_br / (1.0 + 0.003 * sqrt((double)it)));
  return true;
}

}  // namespace plan
}  // namespace nfsp
