// The rollout path of the batched NFSP self-play engine: the fused rollout kernel and the
// deterministic commit of its records into the agents' memories, for one engine (nfsp_rollout)
// and for the replicas of an engine group in shared launches (the _g kernels).
// Declarations and the semantics contract: include/nfsp.h (nfsp_engine_*).
//
// Data path of one nfsp_engine_step, per lane slice.  This file, on the ctx stream:
//   k_rollout   one lane = one env: deal, eta draws, main.train's D/L/D scheduler, every
//               Agent.play (observe -> RL record, act with the AR net or eps-greedy BR
//               net -> env.step -> SL record).  Networks of both agents in LDS.  Records
//               go to lane-major staging ([slot][lane], so a wave's stores coalesce).
//   k_scan1/2   exclusive prefix over lanes of the 4 per-lane record counts -> canonical
//               insert order (lane, then play order) independent of scheduling.
//   k_commit    RL records -> each agent's circular M_RL log (bit-packed RlRec);
//               SL records -> the agent's pending list with their RL stream position.
// Then the learner call (engine_update.hip; kernels in learner.hip): one readback of the insert
// counts for the host's plan of update_strategy's triggers (learn_plan.h), then
//   prep kernels  on the ctx stream, all updates at once: k_br_prep (sampled M_RL rows, fit
//               permutations), k_ar_slots / k_ar_prep (reservoir slots; the AR step records
//               from M_SL as of each trigger), k_res_apply (the reservoir after the inserts)
//   k_br_targets  per agent on its BR stream, per segment between target syncs: the DQN
//               targets and the BR step records
//   k_chain3    the SGD steps, one workgroup per (agent, net) with the net in registers: the
//               BR chain after each segment's targets, both AR chains on the AR stream
//   k_finalize  the insert counters and the reference schedules into EngineDev.
#include <vector>

#include "engine_internal.h"
#include "memtab_lookup.h"

using nfsp::Hand;
using nfsp::u32x4;
namespace nn = nfsp::nn;
using namespace nfsp::eng;

namespace {

// ---------------------------------------------------------------------------
// k_rollout
// ---------------------------------------------------------------------------
struct RolloutArgs {
  int N;                    // lanes of this rollout (one slice)
  uint32_t lane0;           // global id of the slice's first lane (cfg.slices)
  uint32_t k0, k1;
  uint32_t g_lo, g_hi;      // hand index of this rollout (per lane)
  float eta;
  unsigned quirks;
  int game;                 // nfsp::GAME_LEDUC | GAME_KUHN
  int eps_by_value;         // 1: eps_v (the host's schedule mirror); 0: st->epsilon (groups)
  double eps_v[2];
  const float* w;           // [2][3][NP]: the acting nets (the engine's, or a snapshot)
  EngineDev* st;
  Staging S;
};

// Tables that act (nfsp_engine_set_act_table): slot = seat * 2 + role (0 = AR, 1 = BR).  A slot
// with rows set acts with that [ndec][3][3] table through memtab_lookup.h's lookup instead of
// its net; the TAB variant of the rollout alone reads this.
struct ActTabs {
  const float* rows[4];     // the engine's copy per slot, null: the net acts
  const uint32_t* keys;     // [2][MT_H]  the game's lookup on this device
  const uint16_t* vals;     // [2][MT_H]
  const int32_t* rowmap;    // [2][MT_MAX_ROWS] the seat's compact row -> decision row
  unsigned long long* miss; // [4] lookups that found no information set
  int32_t nrows[2];
};

// One replica's rollout / commit arguments in an engine group's device table.
struct GroupRollout {
  RolloutArgs A;
  Memories M;
  int nblk;
  float* snap;          // slice_lag 2: the replica's snapshots [2][2][3][NP] (else null)
  double* snap_eps;     //   and their epsilons [2][2], on device
  ActTabs T;            // the replica's tables that act (k_rollout_gt)
};

// The TAB variant's LDS beside the four nets: both seats' keys (4 KB each) and values (2 KB each),
// the seat's rows of each slot's table (ACT_MAX_ROWS x 9 f32) and the slots' miss counters:
// 21,664 B on top of the 37.9 KB.  Reached from the TAB variant only, so k_rollout and
// k_rollout_g hold none of it.
constexpr int ACT_SLOT_F32 = ACT_MAX_ROWS * 9;
constexpr int ACT_LDS_WORDS = 2 * MT_H + MT_H + 4 * ACT_SLOT_F32 + 4;
__device__ __forceinline__ uint32_t* act_lds() {
  __shared__ __attribute__((aligned(16))) uint32_t s_tab[ACT_LDS_WORDS];
  return s_tab;
}

template <bool TAB>
__device__ __forceinline__ void rollout_body(const RolloutArgs& A, const ActTabs* T, int bx) {
  __shared__ __attribute__((aligned(16))) float sw[4 * NET_LDS];
  __shared__ unsigned s_act[2][3];
  __shared__ int s_rew[2];
  const int tid = threadIdx.x;
  // stage AR0, BR0, AR1, BR1 (fwd_lds layout: padded W1 rows, {b1, W2} per hidden unit)
  for (int e = tid; e < 4 * nn::NP; e += blockDim.x) {
    const int net = e / nn::NP, q = e - net * nn::NP;
    const int agent = net >> 1, kind = net & 1;
    sw[net * NET_LDS + net_lds_index(q)] = A.w[(agent * 3 + kind) * nn::NP + q];
  }
  for (int e = tid; e < 4 * nn::H; e += blockDim.x) sw[(e / nn::H) * NET_LDS + ZROW + e % nn::H] = 0.f;
  if (tid < 6) s_act[tid / 3][tid % 3] = 0;
  if (tid < 2) s_rew[tid] = 0;
  // TAB: the lookup of both seats and the installed slots' rows (the seat's, compact)
  const uint32_t* tkeys = nullptr;
  const uint16_t* tvals = nullptr;
  const float* trows = nullptr;
  unsigned* tmiss = nullptr;
  unsigned thas = 0;                       // bit slot: the slot acts with a table
  if constexpr (TAB) {
    uint32_t* const lds = act_lds();
    uint16_t* const lv = reinterpret_cast<uint16_t*>(lds + 2 * MT_H);
    float* const lr = reinterpret_cast<float*>(lds + 3 * MT_H);
    unsigned* const lm = lds + 3 * MT_H + 4 * ACT_SLOT_F32;
    // a group replica without a table (k_rollout_gt) has no lookup either: nothing of T is read
    if (T->rows[0] || T->rows[1] || T->rows[2] || T->rows[3])
      for (int e = tid; e < 2 * MT_H; e += blockDim.x) {
        lds[e] = T->keys[e];
        lv[e] = T->vals[e];
      }
#pragma unroll
    for (int slot = 0; slot < 4; ++slot) {
      const float* src = T->rows[slot];
      if (!src) continue;                  // uniform over the workgroup
      thas |= 1u << slot;
      const int seat = slot >> 1;
      int nr = T->nrows[seat];
      nr = nr < ACT_MAX_ROWS ? nr : ACT_MAX_ROWS;
      for (int e = tid; e < nr * 9; e += blockDim.x)
        lr[slot * ACT_SLOT_F32 + e] = src[(size_t)T->rowmap[seat * MT_MAX_ROWS + e / 9] * 9 + e % 9];
    }
    if (tid < 4) lm[tid] = 0;
    tkeys = lds; tvals = lv; trows = lr; tmiss = lm;
  }
  __syncthreads();

  const int L = bx * blockDim.x + tid;     // staging index (lane within the slice)
  if (L < A.N) {
    const int N = A.N;
    const uint32_t LG = A.lane0 + (uint32_t)L;   // global lane id: Philox counters, dealer
    const double eps0 = A.eps_by_value ? A.eps_v[0] : A.st->epsilon[0];
    const double eps1 = A.eps_by_value ? A.eps_v[1] : A.st->epsilon[1];
    const int dealer = (int)((LG + A.g_lo) & 1u);
    const int lhand = 1 - dealer;
    uint8_t r0, r1, rp = 0;
    {
      const u32x4 u = nfsp::philox4x32({LG, A.g_lo, A.g_hi, 0u}, A.k0, A.k1);
      if (A.game == nfsp::GAME_KUHN)
        nfsp::deal_kuhn(nfsp::below(u.x, 3), nfsp::below(u.y, 2), r0, r1);
      else
        nfsp::deal_from_draws(nfsp::below(u.x, 6), nfsp::below(u.y, 5), nfsp::below(u.z, 4), r0, r1, rp);
    }
    // eta draws, dealer first (main.py:36-45): 'a' (AR) iff random() > eta
    int polBR[2];
    {
      const u32x4 u = nfsp::philox4x32({LG, A.g_lo, A.g_hi, 1u}, A.k0, A.k1);
      polBR[dealer] = !(nfsp::u01(u.x) > A.eta);
      polBR[lhand] = !(nfsp::u01(u.y) > A.eta);
    }
    Hand h;
    nfsp::hand_reset(h, dealer, r0, r1, rp, A.game);
    const bool alias = (A.quirks & NFSP_QUIRK_ALIAS_RL) != 0;
    int nrl = 0, nsl = 0, nrlp[2] = {0, 0}, nslp[2] = {0, 0};
    int dec = 0, dec_ar = 0;
    uint64_t act_pack = 0;       // 6 x 8-bit action counters (agent*3 + action)
    int rew_half[2] = {0, 0};
    // main.train scheduler (main.py:55-67) as phases of one while-iteration
    int phase = 0, rnd0 = 0;
    bool dT = false, lT = false, first = true;
    for (;;) {
      int who = -1;
      bool initial = false;
      while (!(dT && lT)) {
        if (phase == 0) {
          phase = 1;
          rnd0 = h.rnd;
          if (!dT) { who = dealer; initial = first; first = false; break; }
        } else if (phase == 1) {
          phase = 2;
          if (!lT) { who = lhand; break; }
        } else {
          phase = 0;
          if (rnd0 == h.rnd && !dT) { who = dealer; break; }
        }
      }
      if (who < 0) break;
      const int p = who;
      bool t = false;
      // ---- Agent.play (agent/agent.py:130-156) ----
      if (!initial) {
        t = h.term != 0;
        const float r = t ? h.rew[p] : 0.f;
        const double asum = ((double)h.la[p][0] + (double)h.la[p][1]) + (double)h.la[p][2];
        if (asum != 0.0) {        // np.average(a) != 0 -> remember_for_rl
          const int k = nrl++;
          nrlp[p]++;
          const int rh = (int)(r * 2.0f);
          A.S.rl_s2[k * N + L] = nfsp::hand_obs(h, p);
          A.S.rl_meta[k * N + L] = ((uint32_t)rh & 0xFFu) | ((t ? 1u : 0u) << 8) | ((uint32_t)p << 9);
          if (!alias) {
            A.S.rl_s[k * N + L] = h.s[p];
            A.S.rl_a[(k * 3 + 0) * N + L] = h.la[p][0];
            A.S.rl_a[(k * 3 + 1) * N + L] = h.la[p][1];
            A.S.rl_a[(k * 3 + 2) * N + L] = h.la[p][2];
          }
        }
        if (t) rew_half[p] += (int)(r * 2.0f);
      }
      if (!t) {
        const uint32_t x = nfsp::hand_obs(h, p);
        float y[3];
        // one forward for the whole wave: the net (AR or BR of seat p) is a per-lane LDS
        // base, so lanes acting with different nets share the instructions instead of the
        // wave running an AR and a BR forward one after the other
        const bool br = polBR[p] != 0;
        bool fwd = true;
        u32x4 ub{};
        if (br) {                  // act_best_response's eps draw (agent/agent.py:124-128)
          ub = nfsp::philox4x32({LG, A.g_lo, A.g_hi, 2u + (uint32_t)dec}, A.k0, A.k1);
          dec++;
          fwd = (double)nfsp::u01(ub.x) > (p ? eps1 : eps0);
        }
        bool net = fwd;
        if constexpr (TAB) {
          // the net replaced by a lookup: the slot's row at (p, x), bit for bit.  Every decision
          // of a hand is a row of the tree; an observation that is none acts with y = 0 (the
          // all-zero rule: a fold) and is counted
          const int slot = p * 2 + (br ? 1 : 0);
          if (fwd && ((thas >> slot) & 1u)) {
            net = false;
            const int sid = mt_find(tkeys + p * MT_H, tvals + p * MT_H, x);
            if (sid >= 0 && sid < ACT_SLOT_F32 / 3) {
              const float* row = trows + slot * ACT_SLOT_F32 + sid * 3;
              y[0] = row[0]; y[1] = row[1]; y[2] = row[2];
            } else {
              y[0] = y[1] = y[2] = 0.f;
              atomicAdd(&tmiss[slot], 1u);
            }
          }
        }
        if (net) {
          fwd_lds(sw + (p * 2 + (br ? 1 : 0)) * NET_LDS, x, br ? br_act(A.quirks) : NFSP_ACT_SOFTMAX, y);
        } else if (!fwd) {                   // np.random.rand(1, 1, 3)
          y[0] = nfsp::u01(ub.y); y[1] = nfsp::u01(ub.z); y[2] = nfsp::u01(ub.w);
        }
        if (!br && (A.quirks & NFSP_EXT_SAMPLE_AR)) {   // sample the average policy (textbook NFSP)
          const u32x4 u = nfsp::philox4x32({LG, A.g_lo, A.g_hi, 0x80000000u + (uint32_t)dec_ar},
                                           A.k0, A.k1);
          dec_ar++;
          const float r = nfsp::u01(u.x);
          const int v = r < y[0] ? 0 : (r < y[0] + y[1] ? 1 : 2);
          y[0] = v == 0 ? 1.f : 0.f; y[1] = v == 1 ? 1.f : 0.f; y[2] = v == 2 ? 1.f : 0.f;
        }
        nfsp::hand_step(h, p, y[0], y[1], y[2]);
        if (polBR[p]) {           // remember_best_response(s2, a_t)
          const int k = nsl++;
          nslp[p]++;
          A.S.sl_x[k * N + L] = x;
          if (A.quirks & NFSP_EXT_SL_ONEHOT) {   // the action taken (textbook NFSP)
            const int v = nfsp::argmax3(y[0], y[1], y[2]);
            A.S.sl_a[(k * 3 + 0) * N + L] = v == 0 ? 1.f : 0.f;
            A.S.sl_a[(k * 3 + 1) * N + L] = v == 1 ? 1.f : 0.f;
            A.S.sl_a[(k * 3 + 2) * N + L] = v == 2 ? 1.f : 0.f;
          } else {
            A.S.sl_a[(k * 3 + 0) * N + L] = y[0];
            A.S.sl_a[(k * 3 + 1) * N + L] = y[1];
            A.S.sl_a[(k * 3 + 2) * N + L] = y[2];
          }
          A.S.sl_meta[k * N + L] = (uint32_t)p | ((uint32_t)nrlp[p] << 8);
        }
        act_pack += 1ull << (8 * (p * 3 + nfsp::argmax3(y[0], y[1], y[2])));
      }
      if (p == dealer) dT = t; else lT = t;
    }
    A.S.fin_s[0 * N + L] = h.s[0];
    A.S.fin_s[1 * N + L] = h.s[1];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) A.S.fin_a[(q * 3 + c) * N + L] = h.la[q][c];
    A.S.counts[L] = (uint32_t)nrlp[0] | ((uint32_t)nrlp[1] << 4) | ((uint32_t)nslp[0] << 8) |
                    ((uint32_t)nslp[1] << 12);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const unsigned v = (unsigned)((act_pack >> (8 * q)) & 0xFFu);
      if (v) atomicAdd(&s_act[q / 3][q % 3], v);
    }
    if (rew_half[0]) atomicAdd(&s_rew[0], rew_half[0]);
    if (rew_half[1]) atomicAdd(&s_rew[1], rew_half[1]);
  }
  __syncthreads();
  if (tid < 6 && s_act[tid / 3][tid % 3])
    atomicAdd(&A.st->actions[tid / 3][tid % 3], (unsigned long long)s_act[tid / 3][tid % 3]);
  if (tid < 2 && s_rew[tid]) atomicAdd((unsigned long long*)&A.st->reward_half[tid],
                                       (unsigned long long)(long long)s_rew[tid]);
  if constexpr (TAB) {
    if (tid < 4 && tmiss[tid]) atomicAdd(&T->miss[tid], (unsigned long long)tmiss[tid]);
  }
}

// One engine's rollout runs 512-lane workgroups (8 waves): a 65,536-lane slice then takes
// 128 CUs instead of all 256.  Each rollout workgroup holds 38 KB of LDS (the four nets), so a
// CU running one cannot take a chain workgroup (150 KB, chain3.h CHAIN_LDS); with every CU
// holding one, a BR chain launched during the rollout waited for it to drain (~86 us, once
// per slice on agent 0's BR stream: 1.3 ms per C3 step).  The table variant (k_rollout_t, launched
// only while a slot of the engine has a table) holds 21.2 KB more, 59 KB: it cannot share a CU with
// a chain workgroup either, so the same holds for it.
constexpr int ROLLOUT_WG = 512;
__global__ void __launch_bounds__(ROLLOUT_WG) k_rollout(RolloutArgs A) { rollout_body<false>(A, nullptr, blockIdx.x); }
__global__ void __launch_bounds__(ROLLOUT_WG) k_rollout_t(RolloutArgs A, ActTabs T) {
  rollout_body<true>(A, &T, blockIdx.x);
}

// engine groups: blockIdx.y = replica (the rollout index is the same for every replica)
// par >= 0 (slice_lag 2): the replica acts with its snapshot `par` and that snapshot's epsilon
__global__ void __launch_bounds__(256) k_rollout_g(const GroupRollout* __restrict__ tab, uint32_t g_lo,
                                                   uint32_t g_hi, uint32_t lane0, int par) {
  const GroupRollout& T = tab[blockIdx.y];
  RolloutArgs A = T.A;
  A.g_lo = g_lo;
  A.g_hi = g_hi;
  A.lane0 = lane0;
  if (par >= 0) {
    A.w = T.snap + (size_t)par * 6 * nn::NP;
    A.eps_by_value = 1;
    A.eps_v[0] = T.snap_eps[2 * par + 0];
    A.eps_v[1] = T.snap_eps[2 * par + 1];
  }
  rollout_body<false>(A, nullptr, blockIdx.x);
}

// the same with the replicas' tables that act, launched while any replica has one; a replica
// with none acts with its nets or its snapshot as in k_rollout_g.  A table is not snapshotted:
// the one installed at the step boundary acts in every slice.
__global__ void __launch_bounds__(256) k_rollout_gt(const GroupRollout* __restrict__ tab, uint32_t g_lo,
                                                    uint32_t g_hi, uint32_t lane0, int par) {
  const GroupRollout& T = tab[blockIdx.y];
  RolloutArgs A = T.A;
  A.g_lo = g_lo;
  A.g_hi = g_hi;
  A.lane0 = lane0;
  if (par >= 0) {
    A.w = T.snap + (size_t)par * 6 * nn::NP;
    A.eps_by_value = 1;
    A.eps_v[0] = T.snap_eps[2 * par + 0];
    A.eps_v[1] = T.snap_eps[2 * par + 1];
  }
  rollout_body<true>(A, &T.T, blockIdx.x);
}

// slice_lag 2 in a group: replica blockIdx.y's nets and epsilon -> its snapshot `par` (-1: both
// parities, a step's start), after the slice's learner (and exchange) on the same stream
__global__ void __launch_bounds__(256) k_group_snap(const GroupRollout* __restrict__ tab, int par) {
  const GroupRollout& T = tab[blockIdx.y];
  const int p0 = par < 0 ? 0 : par, p1 = par < 0 ? 1 : par;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 6 * nn::NP; i += gridDim.x * blockDim.x) {
    const float v = T.A.w[i];
    for (int p = p0; p <= p1; ++p) T.snap[(size_t)p * 6 * nn::NP + i] = v;
  }
  if (blockIdx.x == 0 && threadIdx.x < 2)
    for (int p = p0; p <= p1; ++p) T.snap_eps[2 * p + threadIdx.x] = T.A.st->epsilon[threadIdx.x];
}

// The same for a pipelined group step (nfsp_group_step, slice_lag 2): the nets of one learner
// stream only, on that stream right after its chains -- part 0: both agents' AR nets (after
// the AR chains and the exchange); part 1: the BR and target nets and the epsilons (after the
// BR chains and their k_finalize).  Together the two write what k_group_snap writes.
__global__ void __launch_bounds__(256) k_group_snap_part(const GroupRollout* __restrict__ tab, int par, int part) {
  const GroupRollout& T = tab[blockIdx.y];
  float* const dst = T.snap + (size_t)par * 6 * nn::NP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 6 * nn::NP; i += gridDim.x * blockDim.x) {
    const int net = (i / nn::NP) % 3;            // [agent][AR, BR, target][NP]
    if ((net == 0) == (part == 0)) dst[i] = T.A.w[i];
  }
  if (part == 1 && blockIdx.x == 0 && threadIdx.x < 2) T.snap_eps[2 * par + threadIdx.x] = T.A.st->epsilon[threadIdx.x];
}

// ---------------------------------------------------------------------------
// scan of the 4 per-lane counts (canonical insert order)
// ---------------------------------------------------------------------------
__device__ inline unsigned long long unpack_counts(uint32_t c) {
  return (unsigned long long)(c & 15u) | ((unsigned long long)((c >> 4) & 15u) << 16) |
         ((unsigned long long)((c >> 8) & 15u) << 32) | ((unsigned long long)((c >> 12) & 15u) << 48);
}

__device__ __forceinline__ void scan1_body(const uint32_t* __restrict__ counts, int N,
                                           unsigned long long* __restrict__ local,
                                           uint4* __restrict__ block_sum, int bx) {
  __shared__ unsigned long long wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int L = bx * 256 + tid;
  const unsigned long long v = L < N ? unpack_counts(counts[L]) : 0ull;
  // inclusive wave scan (fields never carry: block totals <= 256 * 4)
  unsigned long long x = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  unsigned long long pre = 0;
  for (int k = 0; k < wv; ++k) pre += wsum[k];
  if (L < N) local[L] = pre + x - v;
  if (tid == 255) {
    const unsigned long long tot = pre + x;
    block_sum[bx] = make_uint4((uint32_t)(tot & 0xFFFF), (uint32_t)((tot >> 16) & 0xFFFF),
                               (uint32_t)((tot >> 32) & 0xFFFF), (uint32_t)(tot >> 48));
  }
}

__global__ void __launch_bounds__(256) k_scan1(const uint32_t* __restrict__ counts, int N,
                                               unsigned long long* __restrict__ local,
                                               uint4* __restrict__ block_sum) {
  scan1_body(counts, N, local, block_sum, blockIdx.x);
}

__global__ void __launch_bounds__(256) k_scan1_g(const GroupRollout* __restrict__ tab) {
  const RolloutArgs& A = tab[blockIdx.y].A;
  scan1_body(A.S.counts, A.N, A.S.local, A.S.block_sum, blockIdx.x);
}

__device__ __forceinline__ void scan2_body(const uint4* __restrict__ block_sum, int nblk,
                                           uint4* __restrict__ block_base, EngineDev* st) {
  __shared__ uint4 part[1024];
  __shared__ uint4 carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = make_uint4(0, 0, 0, 0);
  __syncthreads();
  for (int c0 = 0; c0 < nblk; c0 += 1024) {
    const int i = c0 + tid;
    const uint4 v = i < nblk ? block_sum[i] : make_uint4(0, 0, 0, 0);
    part[tid] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      uint4 y = make_uint4(0, 0, 0, 0);
      if (tid >= d) y = part[tid - d];
      __syncthreads();
      if (tid >= d) {
        uint4 p = part[tid];
        p.x += y.x; p.y += y.y; p.z += y.z; p.w += y.w;
        part[tid] = p;
      }
      __syncthreads();
    }
    const uint4 inc = part[tid];
    const uint4 cb = carry;
    if (i < nblk)
      block_base[i] = make_uint4(cb.x + inc.x - v.x, cb.y + inc.y - v.y, cb.z + inc.z - v.z,
                                 cb.w + inc.w - v.w);
    __syncthreads();
    if (tid == 1023) carry = make_uint4(cb.x + inc.x, cb.y + inc.y, cb.z + inc.z, cb.w + inc.w);
    __syncthreads();
  }
  if (tid == 0) {
    st->last_rl[0] = carry.x;
    st->last_rl[1] = carry.y;
    st->last_sl[0] = carry.z;
    st->last_sl[1] = carry.w;
  }
}

__global__ void __launch_bounds__(1024) k_scan2(const uint4* __restrict__ block_sum, int nblk,
                                                uint4* __restrict__ block_base, EngineDev* st) {
  scan2_body(block_sum, nblk, block_base, st);
}

__global__ void __launch_bounds__(1024) k_scan2_g(const GroupRollout* __restrict__ tab) {   // block = replica
  const GroupRollout& T = tab[blockIdx.x];
  scan2_body(T.A.S.block_sum, T.nblk, T.A.S.block_base, T.A.st);
}

// ---------------------------------------------------------------------------
// k_commit: staging -> M_RL logs (fp32 rows) and the pending SL lists
// ---------------------------------------------------------------------------
__device__ __forceinline__ void commit_body(int N, unsigned quirks, const Staging& S, const Memories& M,
                                            const EngineDev* __restrict__ st, int bx) {
  const int L = bx * blockDim.x + threadIdx.x;
  if (L >= N) return;
  const uint32_t cnt = S.counts[L];
  const unsigned long long loc = S.local[L];
  const uint4 bb = S.block_base[L >> 8];
  const int64_t off_rl[2] = {(int64_t)bb.x + (int64_t)(loc & 0xFFFF),
                             (int64_t)bb.y + (int64_t)((loc >> 16) & 0xFFFF)};
  const int64_t off_sl[2] = {(int64_t)bb.z + (int64_t)((loc >> 32) & 0xFFFF),
                             (int64_t)bb.w + (int64_t)(loc >> 48)};
  const int nrl = (int)(cnt & 15u) + (int)((cnt >> 4) & 15u);
  const int nsl = (int)((cnt >> 8) & 15u) + (int)((cnt >> 12) & 15u);
  const bool alias = (quirks & NFSP_QUIRK_ALIAS_RL) != 0;
  int seen[2] = {0, 0};
  for (int k = 0; k < nrl; ++k) {
    const uint32_t meta = S.rl_meta[k * N + L];
    const int p = (meta >> 9) & 1;
    const int64_t pos = st->rl_total[p] + off_rl[p] + seen[p]++;
    const int64_t row = (int64_t)p * M.log_cap + pos % M.log_cap;
    float a[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = alias ? S.fin_a[(p * 3 + c) * N + L] : S.rl_a[(k * 3 + c) * N + L];
    RlRec rec;
    rec.s = alias ? S.fin_s[p * N + L] : S.rl_s[k * N + L];
    rec.s2 = S.rl_s2[k * N + L];
    rec.meta = (uint32_t)nfsp::argmax3(a[0], a[1], a[2]) | (meta & 0x100u) | ((meta & 0xFFu) << 16);
    rec.a0 = a[0]; rec.a1 = a[1]; rec.a2 = a[2];
    rec.pad[0] = rec.pad[1] = 0;
    M.rl[row] = rec;
  }
  int sseen[2] = {0, 0};
  for (int k = 0; k < nsl; ++k) {
    const uint32_t meta = S.sl_meta[k * N + L];
    const int p = meta & 1;
    const int64_t li = (int64_t)p * M.pend_cap + off_sl[p] + sseen[p]++;
    M.pend_x[li] = S.sl_x[k * N + L];
#pragma unroll
    for (int c = 0; c < 3; ++c) M.pend_a[li * 3 + c] = S.sl_a[(k * 3 + c) * N + L];
    M.pend_pos[li] = st->rl_total[p] + off_rl[p] + (int64_t)(meta >> 8);
  }
}

__global__ void __launch_bounds__(256) k_commit(int N, unsigned quirks, Staging S, Memories M,
                                                const EngineDev* __restrict__ st) {
  commit_body(N, quirks, S, M, st, blockIdx.x);
}

__global__ void __launch_bounds__(256) k_commit_g(const GroupRollout* __restrict__ tab) {
  const GroupRollout& T = tab[blockIdx.y];
  commit_body(T.A.N, T.A.quirks, T.A.S, T.M, T.A.st, blockIdx.x);
}

__global__ void k_finish_rollout(EngineDev* st, int64_t N) {
  if (threadIdx.x == 0) {
    st->hands += N;
    st->rollouts += 1;
  }
}

__global__ void k_finish_rollout_g(const GroupRollout* __restrict__ tab, int R) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {   // R may exceed the block
    EngineDev* st = tab[r].A.st;
    st->hands += tab[r].A.N;
    st->rollouts += 1;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
namespace nfsp {
namespace eng {
static RolloutArgs rollout_args(const nfsp_engine* e) {
  RolloutArgs A;
  A.N = e->N;
  A.eps_by_value = 0;               // groups: each replica's st->epsilon (static table)
  A.eps_v[0] = A.eps_v[1] = 0.0;
  // the next rollout plays slice rollouts % slices; a lane's hand index is its hand count
  const uint64_t hand = e->rollouts / (uint64_t)e->slices;
  A.lane0 = (uint32_t)((e->rollouts % (uint64_t)e->slices) * (uint64_t)e->N);
  A.k0 = (uint32_t)e->cfg.seed;
  A.k1 = (uint32_t)(e->cfg.seed >> 32);
  A.g_lo = (uint32_t)hand;
  A.g_hi = (uint32_t)(hand >> 32);
  A.eta = e->cfg.eta;
  A.quirks = e->cfg.quirks;
  A.game = e->ctx->game;
  A.w = e->w;
  A.st = e->st;
  A.S = e->S;
  return A;
}

static bool act_any(const nfsp_engine* e) {
  return e->act_tab[0] || e->act_tab[1] || e->act_tab[2] || e->act_tab[3];
}

// the engine's tables that act, with the game's lookup on this device (none set: all null)
static int act_tabs(const nfsp_engine* e, ActTabs* T) {
  *T = ActTabs{};
  if (!act_any(e)) return NFSP_OK;
  const MtHost* M = nullptr;
  MtDev D;
  const int rc = mt_lookup(e->ctx->game, &M, &D);
  if (rc != NFSP_OK) return rc;
  for (int k = 0; k < 4; ++k) T->rows[k] = e->act_tab[k];
  T->keys = D.keys;
  T->vals = D.vals;
  T->rowmap = D.rows;
  T->miss = e->act_miss;
  T->nrows[0] = M->nrows[0];
  T->nrows[1] = M->nrows[1];
  return NFSP_OK;
}

int rollout_launch(nfsp_engine* e) { return rollout_launch_with(e, e->w, e->hs.epsilon); }

int rollout_launch_with(nfsp_engine* e, const float* w, const double eps[2]) {
  NFSP_REQUIRE(!e->pending_update, "nfsp_engine_update must consume the previous rollout first");
  hipStream_t s = e->ctx->stream;
  RolloutArgs A = rollout_args(e);
  A.w = w;
  A.eps_by_value = 1;               // the schedule as the host computed it (= st->epsilon)
  A.eps_v[0] = eps[0];
  A.eps_v[1] = eps[1];
  ActTabs T;
  const int trc = act_tabs(e, &T);
  if (trc != NFSP_OK) return trc;
  {
    KTimer kt(e, KT_ROLLOUT);
    if (act_any(e)) k_rollout_t<<<(e->N + ROLLOUT_WG - 1) / ROLLOUT_WG, ROLLOUT_WG, 0, s>>>(A, T);
    else k_rollout<<<(e->N + ROLLOUT_WG - 1) / ROLLOUT_WG, ROLLOUT_WG, 0, s>>>(A);
  }
  NFSP_LAUNCHED("k_rollout");
  {
    KTimer kt(e, KT_SCAN);
    k_scan1<<<e->nblk, 256, 0, s>>>(e->S.counts, e->N, e->S.local, e->S.block_sum);
    k_scan2<<<1, 1024, 0, s>>>(e->S.block_sum, e->nblk, e->S.block_base, e->st);
  }
  NFSP_LAUNCHED("k_scan");
  {
    KTimer kt(e, KT_COMMIT);
    k_commit<<<e->nblk, 256, 0, s>>>(e->N, e->cfg.quirks, e->S, e->M, e->st);
  }
  NFSP_LAUNCHED("k_commit");
  k_finish_rollout<<<1, 64, 0, s>>>(e->st, e->N);
  NFSP_LAUNCHED("k_finish_rollout");
  e->rollouts++;
  e->pending_update = true;
  return NFSP_OK;
}

int group_rollout_table(nfsp_engine* const* eng, int R, void** d_tab) {
  std::vector<GroupRollout> h(R);
  for (int r = 0; r < R; ++r) {
    NFSP_REQUIRE(eng[r]->N == eng[0]->N && eng[r]->slices == eng[0]->slices,
                 "group replicas differ in n_lanes or slices");
    h[r].A = rollout_args(eng[r]);
    h[r].M = eng[r]->M;
    h[r].nblk = eng[r]->nblk;
    h[r].snap = eng[r]->snap;
    h[r].snap_eps = eng[r]->snap_eps_dev;
    const int rc = act_tabs(eng[r], &h[r].T);
    if (rc != NFSP_OK) return rc;
  }
  if (!*d_tab) NFSP_HIP(hipMalloc(d_tab, sizeof(GroupRollout) * R));
  NFSP_HIP(hipMemcpy(*d_tab, h.data(), sizeof(GroupRollout) * R, hipMemcpyHostToDevice));
  return NFSP_OK;
}

// every replica's rollout in one launch per kernel (blockIdx.y = replica); the marks are
// kept on replica 0
int group_rollout_launch(nfsp_engine* const* eng, int R, const void* d_tab, int par) {
  nfsp_engine* e0 = eng[0];
  for (int r = 0; r < R; ++r)
    NFSP_REQUIRE(!eng[r]->pending_update && eng[r]->rollouts == e0->rollouts,
                 "group replicas out of step");
  hipStream_t s = e0->ctx->stream;
  const GroupRollout* tab = static_cast<const GroupRollout*>(d_tab);
  {
    KTimer kt(e0, KT_ROLLOUT);
    const RolloutArgs A0 = rollout_args(e0);   // slice and hand index, the same for every replica
    bool any = false;
    for (int r = 0; r < R; ++r) any = any || act_any(eng[r]);
    if (any) k_rollout_gt<<<dim3(e0->nblk, R), 256, 0, s>>>(tab, A0.g_lo, A0.g_hi, A0.lane0, par);
    else k_rollout_g<<<dim3(e0->nblk, R), 256, 0, s>>>(tab, A0.g_lo, A0.g_hi, A0.lane0, par);
  }
  NFSP_LAUNCHED("k_rollout_g");
  {
    KTimer kt(e0, KT_SCAN);
    k_scan1_g<<<dim3(e0->nblk, R), 256, 0, s>>>(tab);
    k_scan2_g<<<R, 1024, 0, s>>>(tab);
  }
  NFSP_LAUNCHED("k_scan_g");
  {
    KTimer kt(e0, KT_COMMIT);
    k_commit_g<<<dim3(e0->nblk, R), 256, 0, s>>>(tab);
  }
  NFSP_LAUNCHED("k_commit_g");
  k_finish_rollout_g<<<1, 256, 0, s>>>(tab, R);
  NFSP_LAUNCHED("k_finish_rollout_g");
  for (int r = 0; r < R; ++r) {
    eng[r]->rollouts++;
    eng[r]->pending_update = true;
  }
  return NFSP_OK;
}

int group_snap_part_launch(nfsp_engine* const* eng, int R, const void* d_tab, int par, int part, hipStream_t s,
                           int r0) {
  k_group_snap_part<<<dim3(nfsp_blocks(6 * nn::NP, 256), R), 256, 0, s>>>(
      static_cast<const GroupRollout*>(d_tab) + r0, par, part);
  NFSP_LAUNCHED("k_group_snap_part");
  return NFSP_OK;
}

int group_snap_launch(nfsp_engine* const* eng, int R, const void* d_tab, int par) {
  for (int r = 0; r < R; ++r)
    NFSP_REQUIRE(eng[r]->snap && eng[r]->snap_eps_dev, "group replica without snapshots (slice_lag 1)");
  k_group_snap<<<dim3(nfsp_blocks(6 * nn::NP, 256), R), 256, 0, eng[0]->ctx->stream>>>(
      static_cast<const GroupRollout*>(d_tab), par);
  NFSP_LAUNCHED("k_group_snap");
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_rollout_with(nfsp_engine* e, const float* dev_w, const double* eps) {
  NFSP_REQUIRE(e && dev_w && eps, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is stepped by nfsp_group_step");
  const double ev[2] = {eps[0], eps[1]};
  return nfsp::eng::rollout_launch_with(e, dev_w, ev);
}

extern "C" int nfsp_rollout(nfsp_engine* e) {
  NFSP_REQUIRE(e, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is stepped by nfsp_group_step");
  return nfsp::eng::rollout_launch(e);
}
