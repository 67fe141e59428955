// The engine's learner (nfsp_engine_update): update_strategy at the reference cadence
// for the RL/SL inserts of the last rollout.  Reference: agent/agent.py:192-273.
// This file: the learner's kernels (the BR instantiation of k_chain3 among them: this is the
// BR chain's translation unit, built with the chain flags), their host launchers
// (learner_internal.h), and the one-engine learner call.  The engine group's host code, which
// launches the same kernels through the launchers, is group.hip.
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

#include "learner_internal.h"

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

// 8 bf16 0/1 values of the layer-1 K slots 8g..8g+7 (bits 4g..4g+3, 16+4g..16+4g+3 of x)
__device__ inline uint4 bits8u(uint32_t x, int g) {
  const uint32_t n0 = (x >> (4 * g)) & 0xFu, n1 = (x >> (16 + 4 * g)) & 0xFu;
  return make_uint4((n0 & 1u) * 0x3F80u + ((n0 >> 1) & 1u) * 0x3F800000u,
                    ((n0 >> 2) & 1u) * 0x3F80u + ((n0 >> 3) & 1u) * 0x3F800000u,
                    (n1 & 1u) * 0x3F80u + ((n1 >> 1) & 1u) * 0x3F800000u,
                    ((n1 >> 2) & 1u) * 0x3F80u + ((n1 >> 3) & 1u) * 0x3F800000u);
}

// The chain records of one (update, epoch): the thread of fit position b < B holds its
// observation mask x, targets and the lr; minibatch b >> 5 gets the swizzled fa chunks and
// tg of its sample b & 31 (the chain reads the transposed operand from fa itself).  Every
// valid sample also carries the bias input (CHAIN_BIAS_BIT).
__device__ inline void emit_recs(StepRec* __restrict__ recs, uint32_t x, float t0, float t1, float t2,
                                 float lr, int B, int b) {
  if (b < B) {
    x |= CHAIN_BIAS_BIT;
    StepRec& R = recs[b >> 5];
    const int k = b & 31;
#pragma unroll
    for (int g = 0; g < 4; ++g) R.fa[g][fa_slot(g, k)] = bits8u(x, g);
    R.tg[k] = make_float4(t0, t1, t2, lr);
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
// a workgroup-uniform field of a job that arrived in VGPRs, in SGPRs (as brp_uniform's below)
__device__ __forceinline__ unsigned tj_uniform(unsigned x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ double tj_uniform(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

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
  const double gamma = tj_uniform(J.gamma), lr0 = tj_uniform(J.lr0);
  const unsigned quirks = tj_uniform(J.quirks);
#include "br_targets_body.inc"
}

// one update's targets by the calling workgroup (k_br_persist's helpers): the same body
__device__ __forceinline__ void br_targets_item(const TargetJob J, int64_t bx, int B, int E, double gamma,
                                                unsigned quirks, double lr0) {
#include "br_targets_body.inc"
}

// ---------------------------------------------------------------------------
// k_br_persist: an engine group's whole BR learner call in one launch (nfsp_group_sched.br_persist;
// round 5, re-landed in round 6 -- DESIGN.md Appendix A.1b).  Workgroups 0 .. njobs - 1 are
// chains, one per (replica, agent) with BR work: each runs its target-sync segments in order,
// in pieces of `chunk` updates, each piece as soon as its targets are written.  The others are
// helpers: they take work items -- (segment, update) -- in queue order and write that update's
// targets and step records (k_br_targets' body).  The host queues the first segments' items; a
// chain queues its next segment's items once the segment's last piece has synced the target
// net they read.  No round waits for another job's segment and no targets launch sits between
// chains.  The same SGD steps as the rounds, bit for bit (a piece resumes from the weights in
// memory).
// Hand-offs, agent scope (per-XCD L2s): the writer's stores, __threadfence in every writing
// thread, the workgroup barrier, then one release atomic; the reader polls relaxed in one
// thread, then one acquire fence and the workgroup barrier.  Every wait is bounded (spin x
// s_sleep 8): on expiry *err is set and the workgroup leaves, so a lost hand-off ends the
// kernel; the host reports it (group_check_err).
// Loop shape: each loop has ONE thread-0 region per iteration, at its top, and the iteration
// ends on a barrier.  The round-5 form also had a thread-0 region at the bottom (the helper's
// "item done" atomic); the compiler merged the two across the back edge into a loop of their
// own, which left the barrier-bearing body as an inner loop that lanes 1-63 of wave 0 and waves
// 1-3 iterated on the stale work word while lane 0 waited for them to leave it: the hang of
// profiles/r05_group_br_persist (found in round 6 in the ISA, profiles/r06/persist_rootcause).
// The words that end the loops (a bail, the next item) are read through readfirstlane, so the
// loops' exits are scalar branches, and a job's fields are made scalar (brp_uniform).
// ---------------------------------------------------------------------------
constexpr uint32_t BRP_EMPTY = 0xFFFFFFFFu, BRP_DONE = 0xFFFFFFFEu;
static_assert(BRP_EMPTY == nfsp::plan::SLOT_EMPTY, "the host fills the queue (group_plan.h)");
constexpr int BRP_STATIC_LDS = 16 * 1024;   // bound on the kernel's static LDS (the targets buffers)

#ifdef NFSP_BRP_STAMPS
// diagnostic build only (tools/build_lib_variant.py brpst -DNFSP_BRP_STAMPS=1, tools/brp_stamps.py):
// per chain [wait cycles, chain cycles, SGD steps, pieces], per helper [wait, work, items, 0]
__device__ unsigned long long g_brp_stamps[2][64][4];
#define BRP_T() __builtin_amdgcn_s_memtime()
#endif

// A job read from the tables arrives in VGPRs (vector loads: the kernel writes global memory,
// so no scalar loads); readfirstlane makes its fields scalar again, as k_chain3's kernel-argument
// jobs are -- otherwise every record load's buffer descriptor becomes a readfirstlane loop
__device__ __forceinline__ int64_t brp_u64(int64_t x) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)x);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)x >> 32));
  return (int64_t)(((uint64_t)hi << 32) | lo);
}
template <class T>
__device__ __forceinline__ T* brp_ptr(T* p) { return reinterpret_cast<T*>(brp_u64(reinterpret_cast<int64_t>(p))); }
__device__ __forceinline__ ChainJob brp_uniform(ChainJob J) {
  J.w = brp_ptr(J.w);
  J.sync_to = brp_ptr(J.sync_to);
  J.snap_to = brp_ptr(J.snap_to);
  J.rec = brp_ptr(J.rec);
  J.active = brp_ptr(J.active);
  J.loss_out = brp_ptr(J.loss_out);
  J.u0 = brp_u64(J.u0);
  J.u1 = brp_u64(J.u1);
  return J;
}

__device__ __forceinline__ void brp_bail(int32_t* err, int k) {
  __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_fetch_add(err + k, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void __launch_bounds__(256) k_br_persist(BrPersistArgs P) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ uint32_t s_word;
#ifdef NFSP_BRP_STAMPS
  unsigned long long st_wait = 0, st_chain = 0, st_steps = 0, st_pieces = 0, st_t1 = 0;
#endif
  if ((int)blockIdx.x < P.njobs) {                         // ---- a chain
    const int j = blockIdx.x;
    for (int s = P.job_seg0[j]; s < P.job_seg0[j + 1]; ++s) {
      const ChainJob JS = brp_uniform(P.seg_job[s]);
      for (int64_t a = JS.u0, c = 0; a < JS.u1; a += P.chunk, ++c) {
        const int64_t b = a + P.chunk < JS.u1 ? a + P.chunk : JS.u1;
        if (threadIdx.x == 0) {                            // the iteration's one thread-0 region
#ifdef NFSP_BRP_STAMPS
          const unsigned long long t0 = BRP_T();
          if (st_t1) st_chain += t0 - st_t1;
#endif
          const uint32_t* done = &P.chunk_done[P.seg_chunk0[s] + c];
          int it = 0;
          while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (uint32_t)(b - a) &&
                 ++it < P.spin)
            __builtin_amdgcn_s_sleep(8);
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
          s_word = it >= P.spin;
          if (s_word) brp_bail(P.err, 1);
#ifdef NFSP_BRP_STAMPS
          st_t1 = BRP_T();
          st_wait += st_t1 - t0;
          st_steps += (b - a) * P.C.E * (P.C.B / CHAIN_MB);
          ++st_pieces;
#endif
        }
        __syncthreads();
        // readfirstlane: the compiler then knows the value is uniform -- a scalar branch, a loop
        // with uniform exits (with a vector value the loop's exits are divergent, values carried
        // in it are taken as divergent and every record load's buffer descriptor became a
        // readfirstlane loop: 1,280 instructions per 4 steps against k_chain3's 1,217)
        if (__builtin_amdgcn_readfirstlane(s_word)) return; // workgroup-uniform
        ChainJob JP = JS;
        JP.u0 = a;
        JP.u1 = b;
        if (b < JS.u1) JP.sync_to = nullptr;               // the segment's last piece syncs
        chain3_run<1, 0, 1>(P.C, JP, smem_raw);
        __threadfence();        // the piece's weights (and synced target net) out, for the next
        __syncthreads();        // piece's loads by other waves and for the helpers
      }
      if (s + 1 < P.job_seg0[j + 1]) {                     // queue the next segment's items
        const uint32_t m = (uint32_t)P.seg_tgt[s + 1].n;
        if (threadIdx.x == 0) s_word = __hip_atomic_fetch_add(&P.ctr[1], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const uint32_t base = __builtin_amdgcn_readfirstlane(s_word);
        for (uint32_t i = threadIdx.x; i < m; i += blockDim.x)
          __hip_atomic_store(&P.slots[base + i], ((uint32_t)(s + 1) << 16) | i, __ATOMIC_RELEASE,
                             __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();        // s_word is rewritten by the next wait
      }
    }
#ifdef NFSP_BRP_STAMPS
    if (threadIdx.x == 0) {
      if (st_t1) st_chain += BRP_T() - st_t1;
      unsigned long long* d = g_brp_stamps[0][j & 63];
      atomicAdd(d + 0, st_wait); atomicAdd(d + 1, st_chain); atomicAdd(d + 2, st_steps); atomicAdd(d + 3, st_pieces);
    }
#endif
    return;
  }
  uint32_t* prev_done = nullptr;                           // thread 0: the last item's chunk counter
  for (;;) {                                                // ---- a helper
    if (threadIdx.x == 0) {                                // the iteration's one thread-0 region:
#ifdef NFSP_BRP_STAMPS
      const unsigned long long t0 = BRP_T();
      if (st_t1) st_chain += t0 - st_t1;                   // (helpers: work cycles)
#endif
      if (prev_done)                                       // publish the last item, take the next
        __hip_atomic_fetch_add(prev_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t p = __hip_atomic_fetch_add(&P.ctr[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      uint32_t v = BRP_DONE;
      if (p < (uint32_t)P.nitems) {
        int it = 0;
        while ((v = __hip_atomic_load(&P.slots[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == BRP_EMPTY &&
               ++it < P.spin)
          __builtin_amdgcn_s_sleep(8);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        if (v == BRP_EMPTY) {
          brp_bail(P.err, 2);
          v = BRP_DONE;
        }
      }
      s_word = v;
#ifdef NFSP_BRP_STAMPS
      st_t1 = BRP_T();
      st_wait += st_t1 - t0;
      if (v != BRP_DONE) ++st_steps;
      if (v == BRP_DONE) {
        unsigned long long* d = g_brp_stamps[1][(blockIdx.x - P.njobs) & 63];
        atomicAdd(d + 0, st_wait); atomicAdd(d + 1, st_chain); atomicAdd(d + 2, st_steps);
      }
#endif
    }
    __syncthreads();
    const uint32_t v = __builtin_amdgcn_readfirstlane(s_word);
    __syncthreads();
    if (v == BRP_DONE) return;                             // workgroup-uniform (scalar)
    const int s = (int)(v >> 16);
    const int64_t i = (int64_t)(v & 0xFFFFu);
    br_targets_item(P.seg_tgt[s], i, P.C.B, P.C.E, P.gamma, P.quirks, P.lr0);
    __threadfence();
    __syncthreads();
    prev_done = &P.chunk_done[P.seg_chunk0[s] + i / P.chunk];
  }
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
// host side (learner_internal.h): the plan of one engine's learner call, its jobs, the launchers
// ---------------------------------------------------------------------------
namespace nfsp {
namespace eng {

int plan_update(const nfsp_engine* e, const EngineDev& h, LearnPlan& L) {
  const nfsp_engine_cfg& cfg = e->cfg;
  PrepArgs& P = L.P;
  P = PrepArgs{};
  P.M = e->M;
  P.LB = e->LB;
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
  L.maxU = L.maxUbr = L.maxSL = 0;
  for (int a = 0; a < 2; ++a) {
    AgentPlan& pl = P.A[a];
    pl.P0 = h.rl_total[a];
    const int64_t n = h.last_rl[a];
    pl.m_first = pl.P0 / P.c + 1;
    const int64_t m_last = (pl.P0 + n) / P.c;
    pl.U = m_last >= pl.m_first ? m_last - pl.m_first + 1 : 0;
    // BR update iff min(p_m, cap) > batch  <=>  m * c > batch
    pl.m_br0 = pl.m_first > cfg.batch / P.c + 1 ? pl.m_first : cfg.batch / P.c + 1;
    pl.U_br = m_last >= pl.m_br0 ? m_last - pl.m_br0 + 1 : 0;
    pl.n_sl = h.last_sl[a];
    pl.sl_total0 = h.sl_total[a];
    NFSP_REQUIRE(pl.U <= e->LB.umax, "update plan exceeds the learner buffers");
    L.maxU = pl.U > L.maxU ? pl.U : L.maxU;
    L.maxUbr = pl.U_br > L.maxUbr ? pl.U_br : L.maxUbr;
    L.maxSL = pl.n_sl > L.maxSL ? pl.n_sl : L.maxSL;
  }
  FinalArgs& F = L.F;
  F = FinalArgs{};
  F.st = e->st;
  F.br_expl = e->LB.br_expl;
  F.umax = e->LB.umax;
  F.sl_cap = cfg.sl_capacity;
  for (int a = 0; a < 2; ++a) {
    const AgentPlan& pl = P.A[a];
    F.n_rl[a] = h.last_rl[a];
    F.n_sl[a] = pl.n_sl;
    F.U_br[a] = pl.U_br;
    // the schedules from the host's mirror (the device copy in EngineDev, written by
    // k_finalize, may still be in flight with cfg.slice_lag 2)
    int64_t it = e->hs.iteration[a], tc = e->hs.target_count[a], syncs = e->hs.target_syncs[a];
    double eps = e->hs.epsilon[a];
    L.it0[a] = it;
    // BR segments between target syncs: [u, v) ends after the first update whose
    // target_count % every == 0 (agent/agent.py:266-273)
    L.seg[a].clear();
    for (int64_t u = 0; u < pl.U_br;) {
      int64_t v = u;
      bool sync = false;
      while (v < pl.U_br) {
        const bool s_here = (tc + v) % cfg.target_every == 0;
        ++v;
        if (s_here) { sync = true; break; }
      }
      L.seg[a].push_back({u, v, sync});
      u = v;
    }
    // schedules (agent/agent.py:245-253, 266-273) in the reference's double arithmetic
    for (int64_t k = 0; k < pl.U_br; ++k) {
      if (tc % cfg.target_every == 0) syncs++;
      tc++;
      it += 2;
      eps = (cfg.quirks & NFSP_EXT_EPS_CONST) ? cfg.epsilon : eps / (double)it;
    }
    if (e->update_limit > 0) {         // test hook: only a prefix of the updates runs
      std::vector<Segment> kept;
      for (const Segment& sg : L.seg[a]) {
        if (sg.u >= e->update_limit) break;
        kept.push_back(sg.v <= e->update_limit ? sg : Segment{sg.u, e->update_limit, false});
      }
      L.seg[a] = kept;
    }
    F.iteration[a] = it;
    F.tcount[a] = tc;
    F.syncs[a] = syncs;
    F.eps[a] = eps;
    L.hs.iteration[a] = it;
    L.hs.target_count[a] = tc;
    L.hs.target_syncs[a] = syncs;
    L.hs.epsilon[a] = eps;
    F.temp[a] = 1.0 / (1.0 + 0.02 * sqrt((double)it));
    F.lr[a] = (float)(cfg.lr_br / (1.0 + 0.003 * sqrt((double)it)));
  }
  return NFSP_OK;
}

void commit_plan(nfsp_engine* e, const LearnPlan& L) {
  e->learn_tag = L.P.tag;
  e->hs = L.hs;
  for (int a = 0; a < 2; ++a) {
    e->last_U[a] = L.P.A[a].U;
    e->last_Ubr[a] = L.P.A[a].U_br;
  }
  e->pending_update = false;
}

static int64_t recs_per_update(const nfsp_engine* e) { return (int64_t)e->cfg.epochs * (e->cfg.batch / CHAIN_MB); }

ChainJob ar_job(const nfsp_engine* e, const LearnPlan& L, int a) {
  const int64_t um = e->LB.umax;
  ChainJob j{};
  j.w = e->w + (a * 3 + 0) * nn::NP;
  j.sync_to = nullptr;
  j.snap_to = nullptr;
  j.rec = e->LB.ar_rec + a * um * recs_per_update(e);
  j.active = e->LB.ar_active + a * um;
  j.loss_out = e->log_loss ? e->LB.ar_loss + a * um * e->cfg.epochs : nullptr;
  j.u0 = 0;
  j.u1 = L.P.A[a].U;
  if (e->update_limit > 0 && j.u1 > e->update_limit) j.u1 = e->update_limit;   // test hook
  return j;
}

TargetJob br_target_job(const nfsp_engine* e, const LearnPlan& L, int a, const Segment& sg) {
  const int64_t um = e->LB.umax, B = e->cfg.batch, E = e->cfg.epochs;
  TargetJob t{};
  t.rows = e->LB.br_rows + a * um * B;
  t.perm = e->LB.br_perm + a * um * E * B;
  t.expl = e->LB.br_expl + a * um;
  t.rec = e->LB.br_rec + a * um * recs_per_update(e);
  t.tw = e->w + (a * 3 + 2) * nn::NP;
  t.u0 = sg.u;
  t.n = sg.v - sg.u;
  t.it0 = L.it0[a];
  t.gamma = e->cfg.gamma;
  t.lr0 = e->cfg.lr_br;
  t.quirks = e->cfg.quirks;
  return t;
}

ChainJob br_chain_job(const nfsp_engine* e, int a, const Segment& sg) {
  const int64_t um = e->LB.umax;
  ChainJob j{};
  j.w = e->w + (a * 3 + 1) * nn::NP;
  j.sync_to = sg.sync ? e->w + (a * 3 + 2) * nn::NP : nullptr;
  j.snap_to = nullptr;
  j.rec = e->LB.br_rec + a * um * recs_per_update(e);
  j.active = nullptr;
  j.loss_out = e->log_loss ? e->LB.br_loss + a * um * e->cfg.epochs : nullptr;
  j.u0 = sg.u;
  j.u1 = sg.v;
  return j;
}

// ---- launchers.  The device code object lists the template kernels in the order of their first
// use below -- the <0> prep kernels, the BR chain, k_finalize<0>, then the <1> forms -- so the
// definitions keep that order.

// the first n0 / n1 updates' epoch losses of the two agents <- NaN (no fit recorded)
static int clear_loss_log(const nfsp_engine* e, float* loss, int64_t n0, int64_t n1, hipStream_t s) {
  const int64_t n[2] = {n0, n1};
  for (int a = 0; a < 2; ++a)
    NFSP_HIP(hipMemsetAsync(loss + a * e->LB.umax * e->cfg.epochs, 0xFF, sizeof(float) * n[a] * e->cfg.epochs, s));
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
      if ((rc = clear_loss_log(eng[r], eng[r]->LB.br_loss, L[r].P.A[0].U_br, L[r].P.A[1].U_br, s)) != NFSP_OK) return rc;
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
      if ((rc = clear_loss_log(eng[r], eng[r]->LB.ar_loss, L[r].P.A[0].U, L[r].P.A[1].U, s)) != NFSP_OK) return rc;
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

int launch_br_persist(const BrPersistArgs& P, int helpers, hipStream_t s) {
  static std::atomic<uint64_t> mask{0};
  static std::atomic<int> dyn{0};
  int dev = 0;
  NFSP_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (!(mask.load(std::memory_order_acquire) & bit)) {
    hipFuncAttributes fa{};
    NFSP_HIP(hipFuncGetAttributes(&fa, (const void*)k_br_persist));
    if ((int)fa.sharedSizeBytes > BRP_STATIC_LDS) return nfsp::fail(NFSP_EINVAL, "k_br_persist: static LDS");
    const int d = CHAIN_LDS - BRP_STATIC_LDS;
    if (d < (int)sizeof(Chain3Smem)) return nfsp::fail(NFSP_EINVAL, "k_br_persist: LDS");
    NFSP_HIP(hipFuncSetAttribute((const void*)k_br_persist, hipFuncAttributeMaxDynamicSharedMemorySize, d));
    dyn.store(d, std::memory_order_release);
    mask.fetch_or(bit, std::memory_order_acq_rel);
  }
  k_br_persist<<<P.njobs + helpers, 256, dyn.load(std::memory_order_acquire), s>>>(P);
  NFSP_LAUNCHED("k_br_persist");
  return NFSP_OK;
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
    float* snap = e->snap + (size_t)e->xchg_pend_par * 6 * nn::NP;
    for (int a = 0; a < 2; ++a)
      NFSP_HIP(hipMemcpyAsync(snap + (a * 3 + 0) * nn::NP, e->w + (a * 3 + 0) * nn::NP,
                              sizeof(float) * nn::NP, hipMemcpyDeviceToDevice, e->s_ar));
    NFSP_HIP(hipEventRecord(e->snap_ev[e->xchg_pend_par][0], e->s_ar));
  }
  return NFSP_OK;
}

// One learner call for the pending rollout.  par: the learner-buffer set (slice parity; 0
// unless cfg.slice_lag 2).  pipelined: leave the chains running (no join into the ctx
// stream; each BR stream publishes its agent's results itself), and when snap_after, copy
// the nets into snapshot `par` after the chains and record snap_ev[par] for the rollout two
// slices on (step_pipelined).
static int update_impl(nfsp_engine* e, bool pipelined, int par, bool snap_after) {
  if (!e->pending_update) return NFSP_OK;
  hipStream_t s = e->ctx->stream;
  const nfsp_engine_cfg& cfg = e->cfg;
  // the trigger plan needs the rollout's insert counts: one small readback
  EngineDev h;
  NFSP_HIP(hipMemcpyAsync(&h, e->st, sizeof(h), hipMemcpyDeviceToHost, s));
  NFSP_HIP(hipStreamSynchronize(s));
  KTimer kt(e, KT_LEARNER);
  e->LB = e->LBs[par];
  LearnPlan L;
  int rc = plan_update(e, h, L);
  if (rc != NFSP_OK) return rc;
  commit_plan(e, L);
  // the cross-shard exchange after this call's AR chain (nfsp_engine_set_exchange)
  const bool xchg = e->xchg_every > 0 && (++e->xchg_calls) % e->xchg_every == 0;
  if (pipelined && snap_after)         // the rollout two slices on acts with this epsilon
    for (int a = 0; a < 2; ++a) e->snap_eps[par][a] = e->hs.epsilon[a];
  // ---- parallel prep on the ctx stream (launch_prep): the BR streams fork behind the BR rows
  // (agent 0's BR segments are the learner's critical path), the AR stream behind the AR records
  hipEvent_t fork_br = take_event(e), fork = take_event(e);
  {
    KTimer kprep(e, KT_PREP);
    if ((rc = launch_prep(e, L, fork_br, fork, s)) != NFSP_OK) return rc;
  }
  // the counters, before the next rollout's commit
  if (pipelined && (rc = launch_finalize(L.F, 1, s)) != NFSP_OK) return rc;
  float* snap = e->snap + (size_t)par * 6 * nn::NP;
  // diagnostic (cfg.sched NFSP_SCHED_LEARNER_SERIAL): BR work waits for the AR chains, to time
  // them alone
  const bool serial_ar = (e->cfg.sched & NFSP_SCHED_LEARNER_SERIAL) != 0;
  hipEvent_t ar_done = fork;
  // ---- AR chains (both agents, one launch) on their own stream.  With the exchange on and
  // the slices pipelined, this call's exchange (and the AR snapshot it feeds) is enqueued by
  // the NEXT call, after its prep and BR chains and right before its AR chain (or at the
  // step's end): an exchange may hold the host until the AR stream reaches it (RCCL's world-1
  // path synchronises the stream), and this way the host has enqueued everything the other
  // streams need before it can wait -- the AR stream's next chain needs the exchange anyway.
  auto ar_part = [&]() -> int {
    int r;
    if (pipelined && (r = flush_exchange(e)) != NFSP_OK) return r;
    NFSP_HIP(hipStreamWaitEvent(e->s_ar, fork, 0));
    if (L.maxU > 0) {
      ChainArgs C = chain_args(cfg);
      for (int a = 0; a < 2; ++a) {
        C.job[a] = ar_job(e, L, a);
        if (snap_after && !xchg) C.job[a].snap_to = snap + (a * 3 + 0) * nn::NP;   // written by the chain
      }
      KTimer kc(e, KT_CHAIN_AR, e->s_ar);
      if ((r = launch_chain_ar(C, 2, e->log_loss, e->s_ar)) != NFSP_OK) return r;
    }
    if (xchg) {
      e->xchg_pending = true;
      e->xchg_pend_par = par;
      e->xchg_pend_snap = snap_after;
      if (!pipelined && (r = flush_exchange(e)) != NFSP_OK) return r;
    } else if (snap_after) {
      if (L.maxU == 0)                 // no AR chain this call: copy the nets as they are
        for (int a = 0; a < 2; ++a)
          NFSP_HIP(hipMemcpyAsync(snap + (a * 3 + 0) * nn::NP, e->w + (a * 3 + 0) * nn::NP,
                                  sizeof(float) * nn::NP, hipMemcpyDeviceToDevice, e->s_ar));
      NFSP_HIP(hipEventRecord(e->snap_ev[par][0], e->s_ar));
    }
    if (serial_ar) {
      ar_done = take_event(e);
      NFSP_HIP(hipEventRecord(ar_done, e->s_ar));
    }
    return NFSP_OK;
  };
  // ---- BR: per agent on its own stream, segments between target syncs = targets + chain
  auto br_part = [&]() -> int {
    int r;
    for (int a = 0; a < 2; ++a) {
      hipStream_t sa = e->s_br[a];
      NFSP_HIP(hipStreamWaitEvent(sa, serial_ar ? ar_done : fork_br, 0));
      KTimer kspan(e, KT_BR_STREAM0 + a, sa);     // this agent's BR stream, end to end
      for (size_t gi = 0; gi < L.seg[a].size(); ++gi) {
        const Segment& sg = L.seg[a][gi];
        {
          KTimer kt2(e, KT_TARGETS, sa);
          r = launch_br_targets(nullptr, br_target_job(e, L, a, sg), sg.v - sg.u, 1, cfg.batch, cfg.epochs, sa);
        }
        if (r != NFSP_OK) return r;
        ChainArgs C = chain_args(cfg);
        C.job[0] = br_chain_job(e, a, sg);
        if (snap_after && gi + 1 == L.seg[a].size())            // the last segment writes the snapshot
          C.job[0].snap_to = snap + (a * 3 + 1) * nn::NP;
        KTimer kc(e, KT_CHAIN_BR, sa);
        if ((r = launch_br_chain(C, 1, cfg.quirks, e->log_loss, sa)) != NFSP_OK) return r;
      }
      // this agent's learner results, after its chain
      if (pipelined && (r = launch_finalize(L.F, 2 << a, sa)) != NFSP_OK) return r;
      if (snap_after) {
        if (L.seg[a].empty())             // no BR chain this call: copy the net as it is
          NFSP_HIP(hipMemcpyAsync(snap + (a * 3 + 1) * nn::NP, e->w + (a * 3 + 1) * nn::NP,
                                  sizeof(float) * nn::NP, hipMemcpyDeviceToDevice, sa));
        NFSP_HIP(hipEventRecord(e->snap_ev[par][1 + a], sa));
      }
    }
    return NFSP_OK;
  };
  // with the exchange on, the BR chains first (they never wait for an exchange), then the AR
  // chain and the exchange (pipelined: the previous call's exchange, then this call's AR chain;
  // else this call's, whose host transport synchronises the AR stream -- the BR streams are
  // busy by then instead of waiting for the host)
  const bool br_first = e->xchg_every > 0 && !serial_ar;
  if (br_first) {
    if ((rc = br_part()) != NFSP_OK) return rc;
    if ((rc = ar_part()) != NFSP_OK) return rc;
  } else {
    if ((rc = ar_part()) != NFSP_OK) return rc;
    if ((rc = br_part()) != NFSP_OK) return rc;
  }
  e->pool.push_back(fork);
  e->pool.push_back(fork_br);
  if (ar_done != fork) e->pool.push_back(ar_done);
  if (pipelined) return NFSP_OK;
  // ---- join and publish the schedules
  if ((rc = join_into(e, s, {e->s_ar, e->s_br[0], e->s_br[1]})) != NFSP_OK) return rc;
  return launch_finalize(L.F, 7, s);
}

extern "C" int nfsp_engine_update(nfsp_engine* e) {
  NFSP_REQUIRE(e, "null argument");
  NFSP_REQUIRE(e->s_ar, "a replica of an engine group is stepped by nfsp_group_step");
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
  for (int p = 0; p < 2; ++p) {
    NFSP_HIP(hipMemcpyAsync(e->snap + (size_t)p * 6 * nn::NP, e->w, sizeof(float) * 6 * nn::NP,
                            hipMemcpyDeviceToDevice, s));
    for (int a = 0; a < 2; ++a) e->snap_eps[p][a] = e->hs.epsilon[a];
  }
  int rc;
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

#ifdef NFSP_BRP_STAMPS
extern "C" int nfsp_debug_brp_stamps(unsigned long long* out, int reset) {
  NFSP_HIP(hipDeviceSynchronize());
  NFSP_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_brp_stamps), sizeof(g_brp_stamps)));
  if (reset) {
    static unsigned long long zero[2][64][4] = {};
    NFSP_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_brp_stamps), zero, sizeof(zero)));
  }
  return NFSP_OK;
}
#endif
