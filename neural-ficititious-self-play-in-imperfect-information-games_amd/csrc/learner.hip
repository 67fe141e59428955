// The engine's learner (nfsp_engine_update): update_strategy at the reference cadence
// for the RL/SL inserts of the last rollout.  Reference: agent/agent.py:192-273.
// This file: the learner's kernels (the BR instantiation of k_chain3 among them: this is the
// BR chain's translation unit, built with the chain flags) and their host launchers
// (learner_internal.h).  The host code of a learner call, which launches the kernels through
// the launchers, is engine_update.hip (one engine) and group.hip (an engine group).
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

}  // namespace eng
}  // namespace nfsp

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
