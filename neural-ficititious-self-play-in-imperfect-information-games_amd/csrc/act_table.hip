// Tables that act (include/nfsp.h nfsp_engine_set_act_table): any of an engine's
// four (agent, role) slots acted by a [ndec][3][3] table over nfsp_tree_export's rows instead of
// its net.  Host code only: the install (the engine's copy, the finiteness check of the seat's
// rows) and the read-back; the lookup itself is the rollout's table variant (rollout.hip
// k_rollout_t, k_rollout_gt).  The group call is group.hip's, which owns nfsp_group.
#include <math.h>

#include <string>
#include <vector>

#include "mem_view.h"
#include "memtab_lookup.h"

using namespace nfsp::eng;

namespace nfsp {
namespace eng {
int act_table_install(nfsp_engine* e, int agent, int role, const float* dev_rows, const char* what) {
  NFSP_REQUIRE((agent == 0 || agent == 1) && (role == 0 || role == 1), "bad agent/role");
  const int slot = agent * 2 + role;
  if (!dev_rows) {                       // the net acts again; the buffer stays for the next install
    e->act_tab[slot] = nullptr;
    return NFSP_OK;
  }
  const MtHost* M = nullptr;
  MtDev D;
  int rc = mt_lookup(e->ctx->game, &M, &D);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(M->nrows[agent] <= ACT_MAX_ROWS, "act table: the seat has more rows than the rollout's LDS holds");
  hipStream_t s = e->ctx->stream;
  const size_t n = (size_t)M->ndec * 9;
  std::vector<float> h(n);
  NFSP_HIP(hipMemcpyAsync(h.data(), dev_rows, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  NFSP_HIP(hipStreamSynchronize(s));
  for (int c = 0; c < M->nrows[agent]; ++c) {
    const int d = M->rows[agent][c];
    for (int k = 0; k < 9; ++k)
      if (!std::isfinite(h[(size_t)d * 9 + k]))
        return nfsp::fail(NFSP_EINVAL, std::string(what) + ": row " + std::to_string(d) + " of the table is not finite");
  }
  if (!e->act_miss) {
    NFSP_HIP(hipMalloc((void**)&e->act_miss, sizeof(unsigned long long) * 4));
    e->allocs.push_back(e->act_miss);
    NFSP_HIP(hipMemsetAsync(e->act_miss, 0, sizeof(unsigned long long) * 4, s));
  }
  if (!e->act_buf[slot]) {
    NFSP_HIP(hipMalloc((void**)&e->act_buf[slot], sizeof(float) * n));
    e->allocs.push_back(e->act_buf[slot]);
  }
  NFSP_HIP(hipMemcpyAsync(e->act_buf[slot], dev_rows, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  NFSP_HIP(hipMemsetAsync(e->act_miss + slot, 0, sizeof(unsigned long long), s));   // a new table counts anew
  NFSP_HIP(hipStreamSynchronize(s));     // the caller may free its own
  e->act_tab[slot] = e->act_buf[slot];
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_engine_set_act_table(nfsp_engine* e, int agent, int role, const float* dev_rows) {
  NFSP_REQUIRE(e, "null argument");
  NFSP_REQUIRE(standalone(e), "nfsp_engine_set_act_table: a replica of an engine group (use the group call, "
                              "nfsp_group_set_act_table)");
  const int rc = engine_rest(e, "nfsp_engine_set_act_table");
  if (rc != NFSP_OK) return rc;
  return act_table_install(e, agent, role, dev_rows, "nfsp_engine_set_act_table");
}

extern "C" int nfsp_engine_get_act_table(nfsp_engine* e, int agent, int role, const float** dev_rows, int64_t* misses) {
  NFSP_REQUIRE(e, "null argument");
  NFSP_REQUIRE((agent == 0 || agent == 1) && (role == 0 || role == 1), "bad agent/role");
  const int slot = agent * 2 + role;
  if (dev_rows) *dev_rows = e->act_tab[slot];
  if (misses) {
    unsigned long long m = 0;
    if (e->act_miss) {
      NFSP_HIP(hipMemcpyAsync(&m, e->act_miss + slot, sizeof(m), hipMemcpyDeviceToHost, e->ctx->stream));
      NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
    }
    *misses = (int64_t)m;
  }
  return NFSP_OK;
}
