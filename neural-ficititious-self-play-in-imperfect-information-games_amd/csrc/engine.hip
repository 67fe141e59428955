// The batched NFSP self-play engine as an object: its lifecycle (allocation from the sizes of
// engine_cfg.h, destruction), nfsp_engine_step, and introspection (stats, the memories in the
// reference's layout, the debug views, the loss log, the timings), and the engine brought to
// rest with the view of its memories (engine_rest, engine_view: mem_view.h).  The rollout path is
// rollout.hip, the learner call engine_update.hip; the data path of a step is described at the
// head of rollout.hip.  Declarations and the semantics contract: include/nfsp.h (nfsp_engine_*).
#include <math.h>

#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "mem_view.h"

namespace nn = nfsp::nn;
using namespace nfsp::eng;

namespace {

// the reference's fp32 tuple layout (utils/replay_buffer.py:53-57) of agent a's memories
__global__ void __launch_bounds__(256) k_export_mem(Memories M, int a) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M.log_cap) {
    const int64_t row = (int64_t)a * M.log_cap + i;
    const RlRec r = M.rl[row];
#pragma unroll
    for (int f = 0; f < nfsp::OBS; ++f) {
      M.ex_rl_s[row * nfsp::OBS + f] = (float)((r.s >> f) & 1u);
      M.ex_rl_s2[row * nfsp::OBS + f] = (float)((r.s2 >> f) & 1u);
    }
    M.ex_rl_a[row * 3 + 0] = r.a0;
    M.ex_rl_a[row * 3 + 1] = r.a1;
    M.ex_rl_a[row * 3 + 2] = r.a2;
    M.ex_rl_r[row] = (float)(int8_t)((r.meta >> 16) & 0xFFu) * 0.5f;
    M.ex_rl_t[row] = (uint8_t)((r.meta >> 8) & 1u);
  }
  if (i < M.sl_cap) {
    const int64_t row = (int64_t)a * M.sl_cap + i;
    const SlRec r = M.sl[row];
#pragma unroll
    for (int f = 0; f < nfsp::OBS; ++f) M.ex_sl_s[row * nfsp::OBS + f] = (float)((r.x >> f) & 1u);
    M.ex_sl_a[row * 3 + 0] = r.a0;
    M.ex_sl_a[row * 3 + 1] = r.a1;
    M.ex_sl_a[row * 3 + 2] = r.a2;
  }
}

}  // namespace

namespace nfsp {
namespace eng {
hipEvent_t take_event(nfsp_engine* e) {
  if (!e->pool.empty()) {
    hipEvent_t ev = e->pool.back();
    e->pool.pop_back();
    return ev;
  }
  hipEvent_t ev = nullptr;
  (void)hipEventCreate(&ev);
  return ev;
}
}  // namespace eng
}  // namespace nfsp

static int eng_alloc(nfsp_engine* e, void** p, size_t bytes) {
  hipError_t r = hipMalloc(p, bytes);
  if (r != hipSuccess) return nfsp::hip_fail(r, "nfsp_engine_create: hipMalloc");
  e->allocs.push_back(*p);
  r = hipMemsetAsync(*p, 0, bytes, e->ctx->stream);
  if (r != hipSuccess) return nfsp::hip_fail(r, "nfsp_engine_create: hipMemset");
  return NFSP_OK;
}

#define EALLOC(ptr, bytes)                                                    \
  do {                                                                        \
    int _rc = eng_alloc(e, (void**)&(ptr), (size_t)(bytes));                  \
    if (_rc != NFSP_OK) { nfsp_engine_destroy(e); return _rc; }               \
  } while (0)

extern "C" int nfsp_engine_default_cfg(nfsp_engine_cfg* c) {
  NFSP_REQUIRE(c, "null argument");
  c->n_lanes = 65536;
  c->hidden = 64;
  c->rl_capacity = 40000;
  c->sl_capacity = 40000;
  c->batch = 128;
  c->inserts_per_update = 128;
  c->target_every = 150;
  c->epochs = 2;
  c->fit_batch = 32;
  c->quirks = NFSP_QUIRKS_REFERENCE;
  c->eta = 0.1f;
  c->lr_br = 0.05f;
  c->lr_ar = 0.1f;
  c->gamma = 0.95;
  c->epsilon = 0.06;
  c->seed = 1234;
  c->slices = 1;
  c->slice_lag = 1;
  const char* ls = getenv("NFSP_LEARNER_SERIAL");
  c->sched = ls && atoi(ls) ? NFSP_SCHED_LEARNER_SERIAL : 0u;
  return NFSP_OK;
}

extern "C" int nfsp_engine_destroy(nfsp_engine* e) {
  if (!e) return NFSP_OK;
  // every stream the engine enqueues on: an update that failed midway may have left a chain
  // running on a side stream without its join into the ctx stream
  if (e->ctx) (void)hipStreamSynchronize(e->ctx->stream);
  for (hipStream_t st : {e->s_br[0], e->s_br[1], e->s_ar})
    if (st) (void)hipStreamSynchronize(st);
  for (void* p : e->allocs) (void)hipFree(p);
  for (auto& pe : e->snap_ev)
    for (hipEvent_t ev : pe)
      if (ev) (void)hipEventDestroy(ev);
  for (auto& m : e->marks) {
    e->pool.push_back(m.second.first);
    e->pool.push_back(m.second.second);
  }
  for (hipEvent_t ev : e->pool) (void)hipEventDestroy(ev);
  for (hipStream_t st : {e->s_br[0], e->s_br[1], e->s_ar})
    if (st) (void)hipStreamDestroy(st);
  delete e;
  return NFSP_OK;
}

namespace nfsp {
namespace eng {
// engine_cfg.h's rules as an error (host only: nfsp_group_cfgs_check runs it without a device)
int engine_cfg_check(const nfsp_engine_cfg* cfg) {
  NFSP_REQUIRE(cfg, "null argument");
  const char* rule = engine_cfg_rule(*cfg);
  NFSP_REQUIRE(!rule, rule);
  return NFSP_OK;
}

// own_streams: the engine's own AR / BR chain streams (nfsp_engine_update); a replica of an
// engine group has none (the group launches its chains)
int engine_create(nfsp_ctx* ctx, const nfsp_engine_cfg* cfg, bool own_streams, nfsp_engine** out) {
  NFSP_REQUIRE(ctx && cfg && out, "null argument");
  const int ck = engine_cfg_check(cfg);
  if (ck != NFSP_OK) return ck;
  *out = nullptr;
  nfsp_engine* e = new nfsp_engine();
  const EngineSizes Z = engine_sizes(*cfg);
  e->ctx = ctx;
  e->cfg = *cfg;
  e->slices = cfg->slices;
  e->N = Z.N;
  e->nblk = Z.nblk;
  const int64_t N = e->N;
  EALLOC(e->w, sizeof(float) * 6 * nn::NP);
  EALLOC(e->st, sizeof(EngineDev));
  EALLOC(e->S.rl_s2, 4 * MAXREC * N);
  EALLOC(e->S.rl_meta, 4 * MAXREC * N);
  EALLOC(e->S.rl_s, 4 * MAXREC * N);
  EALLOC(e->S.rl_a, 4 * 3 * MAXREC * N);
  EALLOC(e->S.sl_x, 4 * MAXREC * N);
  EALLOC(e->S.sl_a, 4 * 3 * MAXREC * N);
  EALLOC(e->S.sl_meta, 4 * MAXREC * N);
  EALLOC(e->S.fin_s, 4 * 2 * N);
  EALLOC(e->S.fin_a, 4 * 6 * N);
  EALLOC(e->S.counts, 4 * N);
  EALLOC(e->S.local, 8 * N);
  EALLOC(e->S.block_sum, sizeof(uint4) * e->nblk);
  EALLOC(e->S.block_base, sizeof(uint4) * e->nblk);
  e->M.log_cap = Z.log_cap;
  e->M.sl_cap = cfg->sl_capacity;
  e->M.pend_cap = Z.pend_cap;
  const int64_t lc = 2 * e->M.log_cap, sc = 2 * e->M.sl_cap, pc = 2 * e->M.pend_cap;
  EALLOC(e->M.rl, sizeof(RlRec) * lc);
  EALLOC(e->M.sl, sizeof(SlRec) * sc);
  EALLOC(e->M.pend_x, 4 * pc);
  EALLOC(e->M.pend_a, 4 * 3 * pc);
  EALLOC(e->M.pend_pos, 8 * pc);
  EALLOC(e->M.dbg_rows, 8 * 4 * cfg->batch);
  EALLOC(e->M.dbg_perms, 4 * 4 * 4 * cfg->batch);
  // the learner's buffers, for umax update triggers per agent (cfg.slice_lag 2: two sets, slice
  // parity; the reservoir lists are shared -- only the ctx stream's prep kernels use them, in
  // slice order)
  e->slice_lag = cfg->slice_lag;
  for (int k = 0; k < (e->slice_lag == 2 ? 2 : 1); ++k) {   // (group replicas too: pipelined groups)
    LearnBufs& L = e->LBs[k];
    L.umax = Z.umax;
    const int64_t ub = 2 * L.umax * cfg->batch, ueb = ub * cfg->epochs;
    EALLOC(L.br_rows, sizeof(BrRow) * ub);
    EALLOC(L.br_perm, ueb);
    EALLOC(L.br_expl, sizeof(double) * 2 * L.umax);
    EALLOC(L.br_rec, 2 * Z.rec_bytes);
    EALLOC(L.ar_rec, 2 * Z.rec_bytes);
    EALLOC(L.ar_active, 2 * L.umax);
    EALLOC(L.br_loss, 4 * 2 * L.umax * cfg->epochs);
    EALLOC(L.ar_loss, 4 * 2 * L.umax * cfg->epochs);
    if (k == 0) {
      EALLOC(L.res_head, sizeof(unsigned long long) * sc);
      EALLOC(L.res_next, 4 * pc);
      EALLOC(L.res_slot, 4 * pc);
    } else {
      L.res_head = e->LBs[0].res_head;
      L.res_next = e->LBs[0].res_next;
      L.res_slot = e->LBs[0].res_slot;
    }
  }
  if (e->slice_lag == 2) {
    EALLOC(e->snap, sizeof(float) * 2 * 6 * nn::NP);
    if (!own_streams) EALLOC(e->snap_eps_dev, sizeof(double) * 4);   // a group replica
    for (auto& pe : e->snap_ev)
      for (hipEvent_t& ev : pe) {
        const hipError_t er = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (er != hipSuccess) {
          nfsp_engine_destroy(e);
          return nfsp::hip_fail(er, "nfsp_engine_create: hipEventCreate");
        }
      }
  }
  for (hipStream_t* st : {&e->s_br[0], &e->s_br[1], &e->s_ar}) {
    if (!own_streams) break;
    hipError_t sr = hipStreamCreateWithFlags(st, hipStreamNonBlocking);
    if (sr != hipSuccess) {
      nfsp_engine_destroy(e);
      return nfsp::hip_fail(sr, "nfsp_engine_create: hipStreamCreate");
    }
  }
  EngineDev h{};
  for (int a = 0; a < 2; ++a) {
    h.epsilon[a] = cfg->epsilon;
    h.temp[a] = 1.0;
    h.lr_br[a] = cfg->lr_br;
    e->hs.epsilon[a] = cfg->epsilon;
  }
  hipError_t r = hipMemcpyAsync(e->st, &h, sizeof(h), hipMemcpyHostToDevice, ctx->stream);
  if (r == hipSuccess) r = hipStreamSynchronize(ctx->stream);
  if (r != hipSuccess) {
    nfsp_engine_destroy(e);
    return nfsp::hip_fail(r, "nfsp_engine_create: init state");
  }
  *out = e;
  return NFSP_OK;
}

// mem_view.h: the engine at a step boundary, its streams idle
int engine_rest(nfsp_engine* e, const char* what, bool for_load) {
  const char* why = nullptr;
  if (e->pending_update || e->xchg_pending)
    why = for_load ? "a rollout or an exchange is pending" : "a rollout awaits nfsp_engine_update, or an exchange is pending";
  else if (!for_load && e->xchg_every > 0 && e->xchg_calls % e->xchg_every != 0)
    why = "the exchange is due only after further learner calls";
  else if (!for_load && e->rollouts % (uint64_t)e->slices != 0) why = "the step's slices are not all played";
  if (why) return nfsp::fail(NFSP_EINVAL, std::string(what) + ": not at a step boundary (" + why + ")");
  NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
  for (hipStream_t st : {e->s_ar, e->s_br[0], e->s_br[1]})
    if (st) NFSP_HIP(hipStreamSynchronize(st));
  return NFSP_OK;
}

int engine_view(nfsp_engine* e, const char* what, MemView* v) {
  int rc = engine_rest(e, what);
  if (rc != NFSP_OK) return rc;
  EngineDev h;
  NFSP_HIP(hipMemcpyAsync(&h, e->st, sizeof(h), hipMemcpyDeviceToHost, e->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
  if ((rc = st_check(h, e->cfg, "engine state")) != NFSP_OK) return rc;
  if ((uint64_t)h.rollouts != e->rollouts) return nfsp::fail(NFSP_EINVAL, "engine state: the device's rollout count differs from the host's");
  *v = mem_view(e, h);
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_engine_create(nfsp_ctx* ctx, const nfsp_engine_cfg* cfg, nfsp_engine** out) {
  return nfsp::eng::engine_create(ctx, cfg, true, out);
}

extern "C" int nfsp_engine_weights(nfsp_engine* e, int agent, int net, float** dev_w) {
  NFSP_REQUIRE(e && dev_w, "null argument");
  NFSP_REQUIRE((agent == 0 || agent == 1) && net >= 0 && net <= 2, "bad agent/net");
  *dev_w = e->w + (agent * 3 + net) * nn::NP;
  return NFSP_OK;
}

// one hand on every lane: each slice's rollout, then the learner on its inserts
extern "C" int nfsp_engine_step(nfsp_engine* e) {
  NFSP_REQUIRE(e, "null argument");
  if (e->slice_lag == 2 && e->slices > 1 && standalone(e)) return nfsp::eng::step_pipelined(e);
  for (int k = 0; k < e->slices; ++k) {
    int rc = nfsp_rollout(e);
    if (rc != NFSP_OK) return rc;
    if ((rc = nfsp_engine_update(e)) != NFSP_OK) return rc;
  }
  return NFSP_OK;
}

extern "C" int nfsp_engine_get_stats(nfsp_engine* e, nfsp_engine_stats* out) {
  NFSP_REQUIRE(e && out, "null argument");
  EngineDev h;
  NFSP_HIP(hipMemcpyAsync(&h, e->st, sizeof(h), hipMemcpyDeviceToHost, e->ctx->stream));
  NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
  *out = nfsp_engine_stats{};
  out->hands = h.hands;
  out->rollouts = h.rollouts;
  for (int a = 0; a < 2; ++a) {
    // before nfsp_engine_update has consumed a rollout its inserts are already made: the
    // RL ones are in M_RL, the SL ones wait in the pending list
    const int64_t rl_total = h.rl_total[a] + (e->pending_update ? h.last_rl[a] : 0);
    out->rl_total[a] = rl_total;
    out->sl_total[a] = h.sl_total[a] + (e->pending_update ? h.last_sl[a] : 0);
    out->rl_size[a] = rl_total < e->cfg.rl_capacity ? rl_total : e->cfg.rl_capacity;
    out->sl_size[a] = h.sl_count[a];
    out->last_rl[a] = h.last_rl[a];
    out->last_sl[a] = h.last_sl[a];
    out->br_updates[a] = h.br_updates[a];
    out->ar_updates[a] = h.ar_updates[a];
    out->iteration[a] = h.iteration[a];
    out->target_syncs[a] = h.target_syncs[a];
    for (int k = 0; k < 3; ++k) out->actions[a][k] = (int64_t)h.actions[a][k];
    out->reward[a] = 0.5 * (double)h.reward_half[a];
    out->epsilon[a] = h.epsilon[a];
    out->temp[a] = h.temp[a];
    out->lr_br[a] = h.lr_br[a];
    out->exploitability[a] = h.expl[a];
  }
  return NFSP_OK;
}

extern "C" int nfsp_engine_memories(nfsp_engine* e, int agent, nfsp_records* rl, int64_t* log_cap,
                                    nfsp_records* sl, uint32_t** px, float** pa, int64_t** ppos) {
  NFSP_REQUIRE(e && (agent == 0 || agent == 1), "bad argument");
  Memories& M = e->M;
  if ((rl || sl) && !M.ex_sl_a) {      // the fp32 reference-layout views, on first use
    // (resumable: a failed allocation leaves the export unusable until a later call
    // completes the set -- ex_sl_a, the last one, is the "all allocated" mark)
    const int64_t lc = 2 * M.log_cap, sc = 2 * M.sl_cap;
    for (auto pr : {std::make_pair((void**)&M.ex_rl_s, 4 * nfsp::OBS * lc), std::make_pair((void**)&M.ex_rl_s2, 4 * nfsp::OBS * lc),
                    std::make_pair((void**)&M.ex_rl_a, 4 * 3 * lc), std::make_pair((void**)&M.ex_rl_r, 4 * lc),
                    std::make_pair((void**)&M.ex_rl_t, lc), std::make_pair((void**)&M.ex_sl_s, 4 * nfsp::OBS * sc),
                    std::make_pair((void**)&M.ex_sl_a, 4 * 3 * sc)}) {
      if (*pr.first) continue;
      NFSP_HIP(hipMalloc(pr.first, (size_t)pr.second));
      e->allocs.push_back(*pr.first);
    }
  }
  const int64_t lo = (int64_t)agent * M.log_cap;
  const int64_t so = (int64_t)agent * M.sl_cap;
  if (rl || sl) {
    const int64_t n = M.log_cap > M.sl_cap ? M.log_cap : M.sl_cap;
    k_export_mem<<<(unsigned)nfsp_blocks(n, 256), 256, 0, e->ctx->stream>>>(M, agent);
    NFSP_LAUNCHED("k_export_mem");
  }
  if (rl) {
    rl->s = M.ex_rl_s + lo * nfsp::OBS;
    rl->a = M.ex_rl_a + lo * 3;
    rl->r = M.ex_rl_r + lo;
    rl->s2 = M.ex_rl_s2 + lo * nfsp::OBS;
    rl->t = M.ex_rl_t + lo;
    rl->cap = M.log_cap;
  }
  if (log_cap) *log_cap = M.log_cap;
  if (sl) {
    sl->s = M.ex_sl_s + so * nfsp::OBS;
    sl->a = M.ex_sl_a + so * 3;
    sl->r = nullptr;
    sl->s2 = nullptr;
    sl->t = nullptr;
    sl->cap = e->M.sl_cap;
  }
  const int64_t po = (int64_t)agent * e->M.pend_cap;
  if (px) *px = e->M.pend_x + po;
  if (pa) *pa = e->M.pend_a + po * 3;
  if (ppos) *ppos = e->M.pend_pos + po;
  return NFSP_OK;
}

extern "C" int nfsp_engine_last_update(nfsp_engine* e, int agent, int role, int64_t** rows,
                                       int32_t** perms) {
  NFSP_REQUIRE(e && (agent == 0 || agent == 1) && (role == 0 || role == 1), "bad argument");
  const int d = agent * 2 + role;
  if (rows) *rows = e->M.dbg_rows + d * e->cfg.batch;
  if (perms) *perms = e->M.dbg_perms + d * e->cfg.epochs * e->cfg.batch;
  return NFSP_OK;
}

extern "C" int nfsp_engine_lane_counts(nfsp_engine* e, uint32_t** counts) {
  NFSP_REQUIRE(e && counts, "null argument");
  *counts = e->S.counts;
  return NFSP_OK;
}

extern "C" int nfsp_engine_set_timing(nfsp_engine* e, int on) {
  NFSP_REQUIRE(e, "null argument");
  e->timing = on != 0;
  return NFSP_OK;
}

extern "C" int nfsp_engine_set_loss_log(nfsp_engine* e, int on) {
  NFSP_REQUIRE(e, "null argument");
  e->log_loss = on != 0;
  return NFSP_OK;
}

extern "C" int nfsp_engine_losses(nfsp_engine* e, double* out) {
  NFSP_REQUIRE(e && out, "null argument");
  NFSP_REQUIRE(e->log_loss, "the loss log is off (nfsp_engine_set_loss_log)");
  NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
  const int E = e->cfg.epochs;
  const LearnBufs& LB = e->LBs[e->last_par];      // the last learner call's set
  for (int a = 0; a < 2; ++a)
    for (int n = 0; n < 2; ++n) {                 // n: 0 = AR (avg_strategy_model), 1 = BR
      const int64_t U = n ? e->last_Ubr[a] : e->last_U[a];
      const float* src = (n ? LB.br_loss : LB.ar_loss) + (int64_t)a * LB.umax * E;
      std::vector<float> h((size_t)(U * E));
      if (U > 0) NFSP_HIP(hipMemcpy(h.data(), src, sizeof(float) * U * E, hipMemcpyDeviceToHost));
      double sum = 0.0, last = NAN;
      int64_t cnt = 0;
      for (int64_t q = 0; q < U * E; ++q)
        if (!std::isnan(h[q])) { sum += h[q]; cnt++; last = h[q]; }
      out[(a * 2 + n) * 2 + 0] = cnt ? sum / (double)cnt : NAN;
      out[(a * 2 + n) * 2 + 1] = last;
    }
  return NFSP_OK;
}

extern "C" int nfsp_engine_get_timings(nfsp_engine* e, double* ms, int64_t* launches) {
  NFSP_REQUIRE(e && ms && launches, "null argument");
  NFSP_HIP(hipStreamSynchronize(e->ctx->stream));
  for (int k = 0; k < KT_N; ++k) { ms[k] = 0.0; launches[k] = 0; }
  for (auto& m : e->marks) {
    float t = 0.f;
    NFSP_HIP(hipEventElapsedTime(&t, m.second.first, m.second.second));
    ms[m.first] += t;
    launches[m.first] += 1;
    e->pool.push_back(m.second.first);
    e->pool.push_back(m.second.second);
  }
  e->marks.clear();
  return NFSP_OK;
}
