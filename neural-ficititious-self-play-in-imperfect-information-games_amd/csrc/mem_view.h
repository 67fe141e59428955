// An engine's memories at a step boundary, for everything that reads or writes them where they
// lie: the state digest, the checkpoint's writer, loader and parser (state.hip) and the memory
// tables (memtab.hip).  Two layers.  The arithmetic, over integers and with standard headers only
// (tests/test_mem_view.py builds it with a host compiler): how many M_RL records are live, and
// where they lie in the circular log.  The engine's view (hipcc only): per agent those records as
// one or two (RlRec*, n) segments, oldest first, the M_SL rows as one (SlRec*, n) segment, and
// the totals a checkpoint's sizes follow from; engine_view / group_view bring an engine or a
// group to rest and build it.  Outside the kernels (rollout.hip, learner.hip) and the fp32 export
// (engine.hip), mem_view() alone forms M.rl + a * log_cap + row or M.sl + a * sl_cap.
#pragma once
#include <stdint.h>

namespace nfsp {
namespace mem {
// live M_RL records of an agent that has inserted rl_total so far
inline int64_t live_count(int64_t rl_total, int64_t rl_capacity) { return rl_total < rl_capacity ? rl_total : rl_capacity; }

// the last `live` (<= log_cap) of rl_total records, record k at row k % log_cap, as the at most
// two (first row, rows) pieces of the circular log, oldest first; no piece is empty
struct Window {
  int n = 0;
  int64_t row[2], len[2];
};
inline Window log_window(int64_t rl_total, int64_t live, int64_t log_cap) {
  Window w;
  if (live <= 0) return w;
  const int64_t r0 = (rl_total - live) % log_cap;
  const int64_t l0 = live < log_cap - r0 ? live : log_cap - r0;
  w.row[w.n] = r0;
  w.len[w.n++] = l0;
  if (l0 < live) {
    w.row[w.n] = 0;
    w.len[w.n++] = live - l0;
  }
  return w;
}
}  // namespace mem
}  // namespace nfsp

#ifdef __HIP__
#include <string>
#include <vector>

#include "engine_internal.h"

namespace nfsp {
namespace eng {
// an EngineDev that this cfg can have produced at a step boundary (bounds every size derived
// from it: copies, digest segments and tables stay inside the memories)
inline int st_check(const EngineDev& h, const nfsp_engine_cfg& c, const char* what) {
  for (int a = 0; a < 2; ++a) {
    const bool ok = h.rl_total[a] >= 0 && h.sl_total[a] >= 0 && h.sl_count[a] >= 0 &&
                    h.sl_count[a] <= c.sl_capacity && h.sl_count[a] <= h.sl_total[a];
    if (!ok) return nfsp::fail(NFSP_EINVAL, std::string(what) + ": memory counters out of range");
  }
  if (h.rollouts < 0 || h.hands < 0) return nfsp::fail(NFSP_EINVAL, std::string(what) + ": negative hand count");
  return NFSP_OK;
}

// records of both agents: what the RL and SL sections of a checkpoint hold
struct MemTotals {
  int64_t rl, sl;
  uint64_t bytes() const { return (uint64_t)rl * sizeof(RlRec) + (uint64_t)sl * sizeof(SlRec); }
};
inline MemTotals mem_totals(const EngineDev& h, int64_t rl_capacity) {
  return MemTotals{mem::live_count(h.rl_total[0], rl_capacity) + mem::live_count(h.rl_total[1], rl_capacity),
                   h.sl_count[0] + h.sl_count[1]};
}

struct AgentView {
  int n_rl = 0;          // M_RL segments, oldest first
  RlRec* rl[2];
  int64_t rl_n[2];
  SlRec* sl;             // M_SL rows [0, sl_n)
  int64_t sl_n;
};
struct MemView {
  EngineDev st;          // the counters the view lays out
  MemTotals total;
  AgentView agent[2];
};

// h's records (st_check'ed) in e's memories.  h need not be e's own: a load lays the blob's
// counters out in the target's log_cap.
inline MemView mem_view(const nfsp_engine* e, const EngineDev& h) {
  MemView v;
  v.st = h;
  v.total = mem_totals(h, e->cfg.rl_capacity);
  for (int a = 0; a < 2; ++a) {
    AgentView& A = v.agent[a];
    const mem::Window w = mem::log_window(h.rl_total[a], mem::live_count(h.rl_total[a], e->cfg.rl_capacity), e->M.log_cap);
    A.n_rl = w.n;
    for (int k = 0; k < w.n; ++k) {
      A.rl[k] = e->M.rl + a * e->M.log_cap + w.row[k];
      A.rl_n[k] = w.len[k];
    }
    A.sl = e->M.sl + a * e->M.sl_cap;
    A.sl_n = h.sl_count[a];
  }
  return v;
}

// An engine (engine.hip) or a group (group.hip) brought to rest: at a step boundary -- anything
// else is NFSP_EINVAL naming `what` -- and every stream it enqueues on idle.  for_load is the
// weaker precondition of the two load entry points, which replace the state instead of reading
// it: no pending update (an engine: or exchange), while the slices played, the exchange cadence
// and the replicas' agreement are not checked.
int engine_rest(nfsp_engine* e, const char* what, bool for_load = false);
int group_rest(nfsp_group* g, const char* what, bool for_load = false);
// At rest, the EngineDev read back (st_check, and the device's rollout count against the
// host's), and its view.  A group replica's handle is an engine here.
int engine_view(nfsp_engine* e, const char* what, MemView* v);
int group_view(nfsp_group* g, const char* what, GroupState* G, std::vector<MemView>* v);
}  // namespace eng
}  // namespace nfsp
#endif  // __HIP__
