// Stand-alone driver of csrc/learn_plan.h for tests/test_learn_plan.py (built with
// -fsanitize=address,undefined).  Reads one case per line from stdin:
//   rl_total last_rl sl_total last_sl  iteration target_count target_syncs epsilon
//   inserts_per_update batch target_every cfg.epsilon cfg.lr_br eps_const  umax limit
// and prints the plan of each on one line.  Doubles travel as the hex of their 64 bits and the
// float (cfg.lr_br, lr) as that of its 32, so the test compares every value exactly.
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "learn_plan.h"

using namespace nfsp::plan;

static double f64_of(uint64_t b) { double d; memcpy(&d, &b, 8); return d; }
static uint64_t bits_of(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

int main() {
  Inserts n;
  AgentSched s;
  Cadence c;
  uint64_t eps, ceps;
  uint32_t lr;
  int ec;
  int64_t umax, limit;
  while (scanf("%" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNx64
               " %" SCNd64 " %" SCNd32 " %" SCNd32 " %" SCNx64 " %" SCNx32 " %d %" SCNd64 " %" SCNd64,
               &n.rl_total, &n.last_rl, &n.sl_total, &n.last_sl, &s.iteration, &s.target_count, &s.target_syncs, &eps,
               &c.inserts_per_update, &c.batch, &c.target_every, &ceps, &lr, &ec, &umax, &limit) == 16) {
    s.epsilon = f64_of(eps);
    c.epsilon = f64_of(ceps);
    memcpy(&c.lr_br, &lr, 4);
    c.eps_const = ec != 0;
    AgentLearn L;
    if (!plan_agent(n, s, c, umax, limit, L)) {
      printf("err\n");
      continue;
    }
    const AgentPlan& A = L.A;
    uint32_t lr_out;
    memcpy(&lr_out, &L.lr, 4);
    printf("ok P0=%" PRId64 " m_first=%" PRId64 " U=%" PRId64 " m_br0=%" PRId64 " U_br=%" PRId64 " n_sl=%" PRId64
           " sl_total0=%" PRId64 " ar_u1=%" PRId64 " it0=%" PRId64 " it=%" PRId64 " tc=%" PRId64 " syncs=%" PRId64
           " eps=%016" PRIx64 " temp=%016" PRIx64 " lr=%08" PRIx32 " seg=",
           A.P0, A.m_first, A.U, A.m_br0, A.U_br, A.n_sl, A.sl_total0, L.ar_u1, L.it0, L.after.iteration,
           L.after.target_count, L.after.target_syncs, bits_of(L.after.epsilon), bits_of(L.temp), lr_out);
    for (size_t i = 0; i < L.seg.size(); ++i)
      printf("%s%" PRId64 ":%" PRId64 ":%d", i ? "," : "", L.seg[i].u, L.seg[i].v, (int)L.seg[i].sync);
    printf("\n");
  }
  return feof(stdin) ? 0 : 2;    // 2: a malformed line
}
