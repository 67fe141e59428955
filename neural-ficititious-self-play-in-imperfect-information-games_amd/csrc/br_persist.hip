// The persistent group BR kernel (nfsp_group_sched.br_persist, opt-in): an engine group's whole
// BR learner call in one launch, instead of group.hip's rounds.  Everything that exists only for
// it: the kernel and its queue protocol, its launcher and the host side of its tables and bail
// flags (br_persist.h, called from group.hip).  Built with the chain flags: the kernel inlines
// the BR chain's body (chain3.h chain3_run) and the targets' (br_targets.h).
#include <string.h>

#include <string>

#include "br_persist.h"
#include "br_targets.h"

using namespace nfsp::eng;
using namespace nfsp::chain;

namespace nfsp {
namespace eng {
// k_br_persist's arguments
struct BrPersistArgs {
  chain::ChainArgs C;           // B, E (the chains' jobs come from seg_job)
  const chain::ChainJob* seg_job;   // [nseg] chain job of each segment (u0, u1: the segment; sync_to)
  const TargetJob* seg_tgt;     // [nseg] its targets job
  const int32_t* seg_chunk0;    // [nseg] its first chunk counter
  const int32_t* job_seg0;      // [njobs + 1] chain workgroup j's segments: [job_seg0[j], job_seg0[j + 1])
  uint32_t* slots;              // [nitems] work items (segment << 16 | update in it); BRP_EMPTY until queued
  uint32_t* ctr;                // [0] helpers' claims, [1] queue reservations
  uint32_t* chunk_done;         // finished items per chunk
  int32_t* err;                 // pinned host: [0] a wait expired, [1] chain bails, [2] helper bails
  int njobs, nitems, chunk;
  int spin;                     // bound of every wait (s_sleep 8 rounds)
  double gamma, lr0;
  unsigned quirks;
};
}  // namespace eng
}  // namespace nfsp

namespace {

constexpr int BRP_SPIN = 1 << 18;           // x s_sleep 8 (~56 ms): far past any legitimate wait
constexpr int BRP_HELPERS = 48;             // helper workgroups (c4_emul_r8, timeline tool, with
                                            // the scalar jobs: 96 / 144 / 192 helpers 193.1 /
                                            // 189.5 / 188.1 ms, the AR chains slowing 155 -> 166;
                                            // the rounds 179.6)

// ---------------------------------------------------------------------------
// k_br_persist: an engine group's whole BR learner call in one launch (nfsp_group_sched.br_persist;
// round 5, re-landed in round 6 -- DESIGN.md Appendix A.1b).  Workgroups 0 .. njobs - 1 are
// chains, one per (replica, agent) with BR work: each runs its target-sync segments in order,
// in pieces of `chunk` updates, each piece as soon as its targets are written.  The others are
// helpers: they take work items -- (segment, update) -- in queue order and write that update's
// targets and step records (br_targets.h, k_br_targets' body).  The host queues the first
// segments' items; a chain queues its next segment's items once the segment's last piece has
// synced the target net they read.  No round waits for another job's segment and no targets
// launch sits between chains.  The same SGD steps as the rounds, bit for bit (a piece resumes
// from the weights in memory).
// Hand-offs, agent scope (per-XCD L2s): the writer's stores, __threadfence in every writing
// thread, the workgroup barrier, then one release atomic; the reader polls relaxed in one
// thread, then one acquire fence and the workgroup barrier.  Every wait is bounded (spin x
// s_sleep 8): on expiry *err is set and the workgroup leaves, so a lost hand-off ends the
// kernel; the host reports it (brp_flags_take below).
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
// so no scalar loads); its fields are made scalar again (br_targets.h), as k_chain3's
// kernel-argument jobs are -- otherwise every record load's buffer descriptor becomes a
// readfirstlane loop
__device__ __forceinline__ ChainJob brp_uniform(ChainJob J) {
  J.w = uniform_ptr(J.w);
  J.sync_to = uniform_ptr(J.sync_to);
  J.snap_to = uniform_ptr(J.snap_to);
  J.rec = uniform_ptr(J.rec);
  J.active = uniform_ptr(J.active);
  J.loss_out = uniform_ptr(J.loss_out);
  J.u0 = (int64_t)uniform64((uint64_t)J.u0);
  J.u1 = (int64_t)uniform64((uint64_t)J.u1);
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

// launch with a CU per workgroup: dynamic LDS up to what the CU has left beside the kernel's
// static LDS (the helpers' targets buffers), as the one-engine chains reserve theirs
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

}  // namespace

// ---------------------------------------------------------------------------
// host side (br_persist.h)
// ---------------------------------------------------------------------------
namespace nfsp {
namespace eng {

hipError_t brp_flags_alloc(int32_t** flags) {
  const hipError_t r = hipHostMalloc((void**)flags, sizeof(int32_t) * 4, hipHostMallocMapped | hipHostMallocCoherent);
  if (r == hipSuccess) memset(*flags, 0, sizeof(int32_t) * 4);
  return r;
}

void brp_flags_free(int32_t* flags) {
  if (flags) (void)hipHostFree(flags);
}

int brp_flags_take(int32_t* flags) {
  volatile int32_t* h = flags;
  if (!h || !h[0]) return NFSP_OK;
  const int cb = h[1], hb = h[2];
  h[0] = h[1] = h[2] = 0;
  return nfsp::fail(NFSP_EHIP, "k_br_persist: a bounded wait expired (work-queue hand-off): chain bails " +
                                   std::to_string(cb) + ", helper bails " + std::to_string(hb));
}

BrpTabs brp_tabs_take(TabCursor& cur, const plan::PersistPlan& q) {
  BrpTabs o;
  o.seg_job = cur.take<ChainJob>(q.segs.size());
  o.seg_tgt = cur.take<TargetJob>(q.segs.size());
  o.seg_chunk0 = cur.take<int32_t>(q.chunk0.size());
  o.job_seg0 = cur.take<int32_t>(q.jseg0.size());
  o.slots = cur.take<uint32_t>(q.slots.size());
  o.ctr = cur.take<uint32_t>(2);
  o.chunk_done = cur.take<uint32_t>((size_t)q.nchunks);
  return o;
}

void brp_tabs_fill(char* h_tab, const BrpTabs& o, const plan::PersistPlan& q, nfsp_engine* const* eng,
                   const LearnPlan* L) {
  for (size_t i = 0; i < q.segs.size(); ++i) {
    const plan::SegRef& t = q.segs[i];
    const Segment& sg = L[t.r].seg[t.a][t.seg];
    tab_at<ChainJob>(h_tab, o.seg_job)[i] = br_chain_job(eng[t.r], L[t.r], t.a, sg);
    tab_at<TargetJob>(h_tab, o.seg_tgt)[i] = br_target_job(eng[t.r], L[t.r], t.a, sg);
  }
  memcpy(h_tab + o.seg_chunk0, q.chunk0.data(), sizeof(int32_t) * q.chunk0.size());
  memcpy(h_tab + o.job_seg0, q.jseg0.data(), sizeof(int32_t) * q.jseg0.size());
  if (!q.slots.empty()) memcpy(h_tab + o.slots, q.slots.data(), sizeof(uint32_t) * q.slots.size());
  tab_at<uint32_t>(h_tab, o.ctr)[0] = 0u;          // helpers' claims
  tab_at<uint32_t>(h_tab, o.ctr)[1] = q.npre;      // queue reservations
  memset(h_tab + o.chunk_done, 0, sizeof(uint32_t) * (size_t)q.nchunks);
}

int brp_launch(char* d_tab, const BrpTabs& o, const plan::PersistPlan& q, const nfsp_engine_cfg& cfg, int spin,
               int32_t* flags, hipStream_t s) {
  if (q.jseg0.size() <= 1) return NFSP_OK;   // no BR work
  BrPersistArgs P{};
  P.C = chain_args(cfg);
  P.seg_job = tab_at<const ChainJob>(d_tab, o.seg_job);
  P.seg_tgt = tab_at<const TargetJob>(d_tab, o.seg_tgt);
  P.seg_chunk0 = tab_at<const int32_t>(d_tab, o.seg_chunk0);
  P.job_seg0 = tab_at<const int32_t>(d_tab, o.job_seg0);
  P.slots = tab_at<uint32_t>(d_tab, o.slots);
  P.ctr = tab_at<uint32_t>(d_tab, o.ctr);
  P.chunk_done = tab_at<uint32_t>(d_tab, o.chunk_done);
  NFSP_HIP(hipHostGetDevicePointer((void**)&P.err, flags, 0));
  P.njobs = (int)q.jseg0.size() - 1;
  P.nitems = (int)q.slots.size();
  P.chunk = BRP_CHUNK;
  P.spin = spin > 1 ? spin : BRP_SPIN;
  P.gamma = cfg.gamma;
  P.lr0 = cfg.lr_br;
  P.quirks = cfg.quirks;
  return launch_br_persist(P, BRP_HELPERS, s);
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
