// The engine's learner (nfsp_engine_update): update_strategy at the reference cadence
// for the RL/SL inserts of the last rollout.  Reference: agent/agent.py:192-273.
// This file: the learner's kernels (the BR instantiation of k_chain3 among them: this is the
// BR chain's translation unit, built with the chain flags) and their host launchers
// (learner_internal.h).  The host code of a learner call, which launches the kernels through
// the launchers, is engine_update.hip (one engine) and group.hip (an engine group).  The device
// code of the targets that another translation unit shares is br_targets.h (br_persist.hip).
//
// An update's inputs (sampled rows, fit permutations, reservoir contents at that moment,
// DQN targets) do not depend on the weights being trained, except the targets on the
// target net, which only changes every TargetModelUpdateRate BR updates.  So all of it
// is produced by wide parallel kernels, and the only sequential work -- the SGD steps
// themselves -- runs in one workgroup per (agent, net) with the whole net resident:
//
//   k_br_prep       [all BR updates]  sample 128 M_RL rows in the window the reference
//                                     would see, gather (s, s2, argmax a, r, t), perms
//   k_ar_slots      [all SL inserts]  reservoir slot of every insert (Philox), per-slot
//                                     insert lists (so any past moment can be read back)
//   k_ar_prep       [all AR updates]  M_SL size at the trigger, sample 128 slots, read the
//                                     slot contents AS OF the trigger, perms -> fit rows
//   k_res_apply     [all SL inserts]  final reservoir contents (last writer per slot)
//   k_br_targets    [a segment]       Q_target forwards, TD values, proxy, row-0 quirk
//   k_chain3<BR/AR> [1 WG per agent]  epochs x minibatch SGD, whole net in registers
// BR chains are cut into segments at target-sync points; the two agents' BR chains and
// the AR chains run on separate streams.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "br_targets.h"

using nfsp::u32x4;
namespace nn = nfsp::nn;
using namespace nfsp::eng;
using namespace nfsp::chain;

namespace {

// ---------------------------------------------------------------------------
// BR prep: rows of update u of agent a (agent/agent.py:217 sample_batch)
// ---------------------------------------------------------------------------
template <int TABLE>   // TABLE: engine groups, blockIdx.z = replica of `tab`
__global__ void __launch_bounds__(128) k_br_prep(PrepArgs P0, const PrepArgs* __restrict__ tab) {
  const PrepArgs& P = TABLE ? tab[blockIdx.z] : P0;
  __shared__ int64_t cand[MAX_BATCH];
  __shared__ uint32_t key[MAX_BATCH];
  const int a = blockIdx.y;
  const int64_t u = blockIdx.x;
  const AgentPlan& pl = P.A[a];
  if (u >= pl.U_br) return;
  const int b = threadIdx.x;
  const int dbg = a * 2 + 1;
  const int64_t m = pl.m_br0 + u;
  const int64_t pm = m * P.c;
  const int64_t win = pm < P.rl_cap ? pm : P.rl_cap;
  sample_distinct(cand, P.B, pm - win, win, TAG_SAMPLE | (uint32_t)dbg, m, P.k0, P.k1);
  const int64_t slot = (int64_t)a * P.LB.umax + u;
  if (b < P.B) {
    const int64_t row = (int64_t)a * P.M.log_cap + cand[b] % P.M.log_cap;
    const uint4 q = *reinterpret_cast<const uint4*>(&P.M.rl[row]);   // s, s2, meta, a0
    BrRow rr;
    rr.s = q.x;
    rr.s2 = q.y;
    rr.meta = q.z;
    P.LB.br_rows[slot * P.B + b] = rr;
  }
  const bool last = u == pl.U_br - 1;
  for (int e = 0; e < P.E; ++e) {
    int rank;
    draw_perm(key, P.B, e, TAG_PERM | (uint32_t)dbg, m, P.k0, P.k1, rank);
    if (b < P.B) {
      P.LB.br_perm[(slot * P.E + e) * P.B + rank] = (uint8_t)b;
      if (last) P.M.dbg_perms[(dbg * P.E + e) * P.B + rank] = b;
    }
  }
  if (last && b < P.B) P.M.dbg_rows[dbg * P.B + b] = cand[b];
}

// ---------------------------------------------------------------------------
// reservoir slots + per-slot insert lists (utils/ReservoirBuffer.py:18-28)
// ---------------------------------------------------------------------------
template <int TABLE>   // TABLE: engine groups, blockIdx.z = replica of `tab`
__global__ void __launch_bounds__(256) k_ar_slots(PrepArgs P0, const PrepArgs* __restrict__ tab) {
  const PrepArgs& P = TABLE ? tab[blockIdx.z] : P0;
  const int a = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const AgentPlan& pl = P.A[a];
  if (q >= pl.n_sl) return;
  const int64_t cap = P.M.sl_cap;
  const int64_t tot = pl.sl_total0 + q;          // adds before this one
  int64_t slot;
  if (tot < cap) {
    slot = tot;                                  // append while count < buffer_size
  } else {
    const u32x4 r = nfsp::philox4x32({TAG_RES | (uint32_t)a, (uint32_t)tot, (uint32_t)(tot >> 32), 0u},
                                     P.k0, P.k1);
    const uint64_t r64 = ((uint64_t)r.x << 32) | r.y;
    const int64_t j = (P.quirks & NFSP_EXT_RESERVOIR)
                          ? (int64_t)(r64 % (uint64_t)(tot + 1))  // Algorithm R: U{0..tot}
                          : 1 + (int64_t)(r64 % (uint64_t)cap);   // randrange(1, N + 1)
    slot = j < cap ? j : -1;                                     // replace iff j < N
  }
  const int64_t qi = (int64_t)a * P.M.pend_cap + q;
  P.LB.res_slot[qi] = (int32_t)slot;
  if (slot >= 0) {
    const unsigned long long mine = ((unsigned long long)P.tag << 32) | (unsigned long long)q;
    const unsigned long long old = atomicExch(&P.LB.res_head[(int64_t)a * cap + slot], mine);
    P.LB.res_next[qi] = (uint32_t)(old >> 32) == P.tag ? (int32_t)(old & 0xFFFFFFFFull) : -1;
  }
}

// latest insert of this rollout into `slot` with index < limit (-1: none)
__device__ inline int64_t latest_insert(const LearnBufs& LB, const Memories& M, int a, int64_t slot,
                                        int64_t limit, uint32_t tag) {
  const unsigned long long h = LB.res_head[(int64_t)a * M.sl_cap + slot];
  if ((uint32_t)(h >> 32) != tag) return -1;
  int64_t best = -1;
  int32_t q = (int32_t)(h & 0xFFFFFFFFull);
  while (q >= 0) {
    if (q < limit && q > best) best = q;
    q = LB.res_next[(int64_t)a * M.pend_cap + q];
  }
  return best;
}

// ---------------------------------------------------------------------------
// AR prep (agent/agent.py:259-261): M_SL as it was at the trigger
// ---------------------------------------------------------------------------
template <int TABLE>   // TABLE: engine groups, blockIdx.z = replica of `tab`
__global__ void __launch_bounds__(128) k_ar_prep(PrepArgs P0, const PrepArgs* __restrict__ tab) {
  const PrepArgs& P = TABLE ? tab[blockIdx.z] : P0;
  __shared__ int64_t cand[MAX_BATCH];
  __shared__ uint32_t key[MAX_BATCH];
  __shared__ uint32_t rx[MAX_BATCH];
  __shared__ float ra[MAX_BATCH][3];
  __shared__ uint32_t px[MAX_BATCH];
  __shared__ float pt[MAX_BATCH][3];
  const int a = blockIdx.y;
  const int64_t u = blockIdx.x;
  const AgentPlan& pl = P.A[a];
  if (u >= pl.U) return;
  const int b = threadIdx.x;
  const int dbg = a * 2 + 0;
  const int64_t m = pl.m_first + u;
  const int64_t pm = m * P.c;
  const int64_t slot_u = (int64_t)a * P.LB.umax + u;
  // SL inserts made before the trigger (pend_pos is nondecreasing): a 128-ary search, a few
  // rounds of one probe per thread instead of one thread's ~20 dependent loads.  lo / hi
  // are block-uniform: every thread takes the same rounds.
  const int64_t* pos = P.M.pend_pos + (int64_t)a * P.M.pend_cap;
  const int nt = blockDim.x;
  int64_t lo = 0, hi = pl.n_sl;
  while (hi - lo > nt) {
    const int64_t span = hi - lo;       // probe t at lo + span (t + 1) / (nt + 1): increasing
    const int k = __syncthreads_count(pos[lo + span * (b + 1) / (nt + 1)] <= pm);
    const int64_t below = lo + span * k / (nt + 1);          // probe k - 1 (k >= 1)
    const int64_t above = lo + span * (k + 1) / (nt + 1);    // probe k (k < nt)
    lo = k > 0 ? below + 1 : lo;
    hi = k < nt ? above : hi;
  }
  const int64_t nb = lo + __syncthreads_count(lo + b < hi && pos[lo + b] <= pm);
  const int64_t tot = pl.sl_total0 + nb;
  const int64_t count = tot < P.M.sl_cap ? tot : P.M.sl_cap;
  if (count <= P.B) {                         // size() > minibatch_size fails
    if (b == 0) P.LB.ar_active[slot_u] = 0;
    return;
  }
  if (b == 0) {
    P.LB.ar_active[slot_u] = 1;
    atomicAdd((unsigned long long*)&P.st->ar_updates[a], 1ull);
  }
  sample_distinct(cand, P.B, 0, count, TAG_SAMPLE | (uint32_t)dbg, m, P.k0, P.k1);
  if (b < P.B) {
    const int64_t j = cand[b];
    const int64_t q = latest_insert(P.LB, P.M, a, j, nb, P.tag);
    if (q >= 0) {
      const int64_t qi = (int64_t)a * P.M.pend_cap + q;
      rx[b] = P.M.pend_x[qi];
      ra[b][0] = P.M.pend_a[qi * 3 + 0];
      ra[b][1] = P.M.pend_a[qi * 3 + 1];
      ra[b][2] = P.M.pend_a[qi * 3 + 2];
    } else {
      const SlRec r = P.M.sl[(int64_t)a * P.M.sl_cap + j];
      rx[b] = r.x;
      ra[b][0] = r.a0;
      ra[b][1] = r.a1;
      ra[b][2] = r.a2;
    }
  }
  const bool last = u == pl.U - 1;
  for (int e = 0; e < P.E; ++e) {
    int rank;
    draw_perm(key, P.B, e, TAG_PERM | (uint32_t)dbg, m, P.k0, P.k1, rank);
    if (b < P.B) {        // fit position rank <- sampled row b
      px[rank] = rx[b];
      pt[rank][0] = ra[b][0]; pt[rank][1] = ra[b][1]; pt[rank][2] = ra[b][2];
      if (last) P.M.dbg_perms[(dbg * P.E + e) * P.B + rank] = b;
    }
    __syncthreads();
    const bool in = b < P.B;
    // targets / batch: the AR chain's cross-entropy gradient takes them pre-scaled (exact)
    const float sc = 1.0f / (float)CHAIN_MB;
    emit_recs(P.LB.ar_rec + (slot_u * P.E + e) * (P.B / CHAIN_MB), in ? px[b] : 0u, in ? pt[b][0] * sc : 0.f,
              in ? pt[b][1] * sc : 0.f, in ? pt[b][2] * sc : 0.f, P.lr_ar, P.B, b);
    __syncthreads();
  }
  if (last && b < P.B) P.M.dbg_rows[dbg * P.B + b] = cand[b];
}

template <int TABLE>   // TABLE: engine groups, blockIdx.z = replica of `tab`
__global__ void __launch_bounds__(256) k_res_apply(PrepArgs P0, const PrepArgs* __restrict__ tab) {
  const PrepArgs& P = TABLE ? tab[blockIdx.z] : P0;
  const int a = blockIdx.y;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= P.A[a].n_sl) return;
  const int64_t qi = (int64_t)a * P.M.pend_cap + q;
  const int64_t slot = P.LB.res_slot[qi];
  if (slot < 0) return;
  if (latest_insert(P.LB, P.M, a, slot, P.A[a].n_sl, P.tag) != q) return;   // a later add wins
  SlRec r;
  r.x = P.M.pend_x[qi];
  r.a0 = P.M.pend_a[qi * 3 + 0];
  r.a1 = P.M.pend_a[qi * 3 + 1];
  r.a2 = P.M.pend_a[qi * 3 + 2];
  P.M.sl[(int64_t)a * P.M.sl_cap + slot] = r;
}

// ---------------------------------------------------------------------------
// DQN targets of one BR segment (agent/agent.py:219-241), one update per workgroup
// ---------------------------------------------------------------------------
// blockIdx.x = update within the segment; blockIdx.y = job (of `jobs`, else `one`).  gamma, lr0
// and quirks are the job's own (one engine: its cfg's; a group: each replica's).
__global__ void __launch_bounds__(256) k_br_targets(const TargetJob* __restrict__ jobs, TargetJob one,
                                                    int B, int E) {
  const TargetJob J = jobs ? jobs[blockIdx.y] : one;
  const int64_t bx = blockIdx.x;
  // The compiler folds the two sources of J into one selected address and loads the job through
  // it with vector loads, the by-value `one` (kernel-argument memory) included.  The three values
  // that were launch-wide arguments steer branches and selects of the whole workgroup (br_act,
  // the ROW0 / TERMINAL quirks) and the f64 TD and lr arithmetic: made scalar again.
  const double gamma = uniform_f64(J.gamma), lr0 = uniform_f64(J.lr0);
  const unsigned quirks = uniform32(J.quirks);
#include "br_targets_body.inc"
}

// mode bits: 1 = the insert counters (both agents; they must be current before the next
// rollout's commit), 2 << a = agent a's learner results and schedules (after its BR chain)
template <int TABLE>   // TABLE: engine groups, block = replica of `tab`
__global__ void k_finalize(FinalArgs F0, const FinalArgs* __restrict__ tab, int mode) {
  const FinalArgs& F = TABLE ? tab[blockIdx.x] : F0;
  if (threadIdx.x != 0) return;
  for (int a = 0; a < 2; ++a) {
    EngineDev* st = F.st;
    if (mode & 1) {
      st->rl_total[a] += F.n_rl[a];
      st->sl_total[a] += F.n_sl[a];
      st->sl_count[a] = st->sl_total[a] < F.sl_cap ? st->sl_total[a] : F.sl_cap;
    }
    if ((mode & (2 << a)) && F.U_br[a] > 0) {
      st->expl[a] = F.br_expl[(int64_t)a * F.umax + F.U_br[a] - 1];
      st->br_updates[a] += F.U_br[a];
      st->iteration[a] = F.iteration[a];
      st->target_count[a] = F.tcount[a];
      st->target_syncs[a] = F.syncs[a];
      st->epsilon[a] = F.eps[a];
      st->temp[a] = F.temp[a];
      st->lr_br[a] = F.lr[a];
    }
  }
}

// engine groups: the exchanged nets of all replicas <- W0 + (sum_r (W_r - W0)) * scale, and W0 <-
// that (nfsp_engine_set_exchange's arithmetic over shards, on device, in replica order).
// wtab [3 nets: AR, BR, target][R][2 agents]; nets / bcast: masks over the 3 (bcast: the first
// exchange of a net copies replica 0's everywhere)
__global__ void __launch_bounds__(256) k_group_xchg(float* const* __restrict__ wtab, float* __restrict__ w0 /*[3][2][NP]*/,
                                                    int R, unsigned nets, unsigned bcast, float scale) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * 2 * nn::NP) return;
  const int n = i / (2 * nn::NP), k = i - n * 2 * nn::NP;
  const int a = k / nn::NP, q = k - a * nn::NP;
  const bool b = (bcast >> n) & 1u;
  if (!b && !((nets >> n) & 1u)) return;
  float* const* war = wtab + (size_t)n * R * 2;
  float nw;
  if (b) {
    nw = war[a][q];
  } else {
    const float base = w0[i];
    float s = 0.f;
    // the sum stays in replica order; the unroll lets 16 replicas' loads go out together
    // (one at a time, R = 256 took 0.2 ms of latency per step)
#pragma unroll 16
    for (int r = 0; r < R; ++r) s = s + (war[2 * r + a][q] - base);
    nw = base + s * scale;
  }
  w0[i] = nw;
  for (int r = 0; r < R; ++r) war[2 * r + a][q] = nw;
}

// engine groups: the replicas' EngineDev, gathered for one readback
__global__ void k_gather_st(EngineDev* const* __restrict__ src, EngineDev* __restrict__ dst, int R) {
  constexpr int W = (int)(sizeof(EngineDev) / 8);
  static_assert(sizeof(EngineDev) % 8 == 0, "EngineDev words");
  for (int i = threadIdx.x; i < R * W; i += blockDim.x) {
    const int r = i / W, k = i - r * W;
    reinterpret_cast<uint64_t*>(dst + r)[k] = reinterpret_cast<const uint64_t*>(src[r])[k];
  }
}

}  // namespace

#ifdef NFSP_CHAIN_STAMPS
// diagnostic build only: the accumulated chain phase cycles ([8][4][10] u64), then reset
extern "C" int nfsp_debug_chain_stamps(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_chain_stamps), sizeof(g_chain_stamps)) != hipSuccess) return -1;
  static const unsigned long long zero[8][4][10] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_chain_stamps), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif

// ---------------------------------------------------------------------------
// host side: the launchers (learner_internal.h).  The device code object lists the template
// kernels in the order of their first use below -- the <0> prep kernels, the BR chain,
// k_finalize<0>, then the <1> forms -- so the definitions keep that order.
// ---------------------------------------------------------------------------
namespace nfsp {
namespace eng {

// the first n0 / n1 updates' epoch losses of the two agents in a log of the plan's buffer set
// <- NaN (no fit recorded)
static int clear_loss_log(const PrepArgs& P, float* loss, int64_t n0, int64_t n1, hipStream_t s) {
  const int64_t n[2] = {n0, n1};
  for (int a = 0; a < 2; ++a)
    NFSP_HIP(hipMemsetAsync(loss + a * P.LB.umax * P.E, 0xFF, sizeof(float) * n[a] * P.E, s));
  return NFSP_OK;
}

// launch_prep / launch_prep_table.  TABLE 0: one engine (R 1), its PrepArgs by value; 1: the
// same prep kernels, every replica in one launch (blockIdx.z = its entry of `tab`)
template <int TABLE>
static int launch_prep_t(nfsp_engine* const* eng, const LearnPlan* L, int R, const PrepArgs* tab, hipEvent_t fork_br,
                         hipEvent_t fork, hipStream_t s) {
  const PrepArgs one = TABLE ? PrepArgs{} : L[0].P;
  int64_t maxU = 0, maxUbr = 0, maxSL = 0;
  for (int r = 0; r < R; ++r) {
    maxU = L[r].maxU > maxU ? L[r].maxU : maxU;
    maxUbr = L[r].maxUbr > maxUbr ? L[r].maxUbr : maxUbr;
    maxSL = L[r].maxSL > maxSL ? L[r].maxSL : maxSL;
  }
  const bool loss_log = eng[0]->log_loss;   // a group: on in all replicas or none
  int rc;
  if (maxUbr > 0) {
    k_br_prep<TABLE><<<dim3((unsigned)maxUbr, 2, R), 128, 0, s>>>(one, tab);
    NFSP_LAUNCHED("k_br_prep");
  }
  if (loss_log)
    for (int r = 0; r < R; ++r)
      if ((rc = clear_loss_log(L[r].P, L[r].P.LB.br_loss, L[r].P.A[0].U_br, L[r].P.A[1].U_br, s)) != NFSP_OK) return rc;
  NFSP_HIP(hipEventRecord(fork_br, s));
  if (maxSL > 0) {
    k_ar_slots<TABLE><<<dim3(nfsp_blocks(maxSL, 256), 2, R), 256, 0, s>>>(one, tab);
    NFSP_LAUNCHED("k_ar_slots");
  }
  if (maxU > 0) {
    k_ar_prep<TABLE><<<dim3((unsigned)maxU, 2, R), 128, 0, s>>>(one, tab);
    NFSP_LAUNCHED("k_ar_prep");
  }
  if (loss_log)                          // (an inactive AR update records no fit either)
    for (int r = 0; r < R; ++r)
      if ((rc = clear_loss_log(L[r].P, L[r].P.LB.ar_loss, L[r].P.A[0].U, L[r].P.A[1].U, s)) != NFSP_OK) return rc;
  NFSP_HIP(hipEventRecord(fork, s));
  if (maxSL > 0) {
    k_res_apply<TABLE><<<dim3(nfsp_blocks(maxSL, 256), 2, R), 256, 0, s>>>(one, tab);
    NFSP_LAUNCHED("k_res_apply");
  }
  return NFSP_OK;
}

int launch_prep(nfsp_engine* e, const LearnPlan& L, hipEvent_t fork_br, hipEvent_t fork, hipStream_t s) {
  return launch_prep_t<0>(&e, &L, 1, nullptr, fork_br, fork, s);
}

int launch_br_targets(const TargetJob* jobs, const TargetJob& one, int64_t n, int njobs, int B, int E, hipStream_t s) {
  k_br_targets<<<dim3((unsigned)n, (unsigned)njobs), 256, 0, s>>>(jobs, one, B, E);
  NFSP_LAUNCHED("k_br_targets");
  return NFSP_OK;
}

int launch_br_chain(const ChainArgs& C, int blocks, unsigned quirks, bool loss_log, hipStream_t s) {
  if (quirks & NFSP_EXT_LINEAR_Q)
    return launch_chain_br_linear(C, blocks, loss_log, (quirks & NFSP_EXT_MSE_Q) != 0, s);
  static std::atomic<uint64_t> attr{0};
  return launch_chain<1>(C, blocks, loss_log, s, attr);
}

template <int TABLE>
static int launch_finalize_t(const FinalArgs& F, const FinalArgs* tab, int n, int mode, hipStream_t s) {
  k_finalize<TABLE><<<n, 64, 0, s>>>(F, tab, mode);
  NFSP_LAUNCHED("k_finalize");
  return NFSP_OK;
}

int launch_finalize(const FinalArgs& F, int mode, hipStream_t s) { return launch_finalize_t<0>(F, nullptr, 1, mode, s); }

int launch_prep_table(nfsp_engine* const* eng, const LearnPlan* L, int R, const PrepArgs* tab, hipEvent_t fork_br,
                      hipEvent_t fork, hipStream_t s) {
  return launch_prep_t<1>(eng, L, R, tab, fork_br, fork, s);
}

int launch_finalize_table(const FinalArgs* tab, int n, int mode, hipStream_t s) {
  return launch_finalize_t<1>(FinalArgs{}, tab, n, mode, s);
}

int launch_gather_st(EngineDev* const* src, EngineDev* dst, int R, hipStream_t s) {
  k_gather_st<<<1, 256, 0, s>>>(src, dst, R);
  NFSP_LAUNCHED("k_gather_st");
  return NFSP_OK;
}

int launch_group_xchg(float* const* wtab, float* w0, int R, unsigned nets, unsigned bcast, float scale, hipStream_t s) {
  k_group_xchg<<<nfsp_blocks(3 * 2 * nn::NP, 256), 256, 0, s>>>(wtab, w0, R, nets, bcast, scale);
  NFSP_LAUNCHED("k_group_xchg");
  return NFSP_OK;
}

}  // namespace eng
}  // namespace nfsp
