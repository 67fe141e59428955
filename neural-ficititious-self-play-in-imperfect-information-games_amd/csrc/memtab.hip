// M_SL / M_RL tabulated per information set on the device (include/nfsp.h nfsp_memory_table,
// nfsp_engine_memory_table, nfsp_group_memory_tables).
//
// A record belongs to (seat, observation) = one (row, rank) of the evaluator's tree
// (exploit_tree.h).  Per game and seat the host builds an open-addressing table observation ->
// sid = 3 x (the seat's compact row) + rank from HostTables; k_memtab stages the seat's table to
// LDS, reads every record once (one 16-byte load: an M_RL record's key, argmax, t and r all sit
// in its first half) and adds into LDS bins [sid][action][field], int64, one copy per workgroup,
// with plain LDS adds (ds_add_u64): neither a copy per wave nor folding the lanes of a wave that
// share a key paid (DESIGN.md §9 has the measurement).  A workgroup writes its bins with plain
// stores and k_memtab_sum adds the workgroups' partials: integers only and no global atomics,
// so every order of accumulation gives the same bits.
//
// One launch serves any number of tables (a seat of an engine or of a group's replica each)
// through a device job table, as the chains' ChainJob does.  The engine and group forms open with
// engine_view / group_view (mem_view.h) and take an agent's segments from that view, as the
// state digest does.
//
// The third kind, NFSP_MEM_TD (nfsp_td_table), counts what the BR net is fitted to: per M_RL
// record k_br_targets' value r + gamma max Q_target(s2), by the stored s and argmax.  The target
// net lies in LDS beside the hash and the bins (fwd_lds' layout) and every lane forwards its
// record's s2 -- lanes without a record or an information set forward x = 0, fwd_lds ballots --
// and adds fix(v) and fix(max Q).  gamma, quirks and the net ride in the table's job, so the
// replicas of a heterogeneous group go through one launch.
//
// The fourth kind, NFSP_MEM_TDQ (nfsp_tdq_table), is the third with a table in the target net's
// place: the seat's Q rows lie in LDS in front of the bins, compact by sid as the bins are, and a
// record's bootstrap is the largest of the three entries at lookup(seat, s2), 0 where s2 is no
// information set.  There is no forward, so it keeps MT_U records per lane in flight as the
// counting kinds do.  nfsp_engine_tabular_q / nfsp_group_tabular_q run K fitted-Q sweeps with it:
// per sweep k_memtab<TDQ>, k_memtab_sum and k_table_rows (tabq.hip) on the stream, the Q tables
// alternating between two buffers of the workspace, and one synchronisation at the end.
#include <math.h>

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "exploit_tree.h"
#include "mem_view.h"
#include "memtab_lookup.h"

using namespace nfsp::eng;

namespace {

constexpr int MT_MAX_SEG = 8;
constexpr int MT_WG = 1024;             // 16 waves
constexpr int MT_U = 4;                 // records per lane in flight
constexpr int TD_U = 1;                 // NFSP_MEM_TD: one, so that fwd_lds_n<9>'s gathers stay in registers
                                        //   (124 VGPRs at 1,024 lanes, no scratch: DESIGN.md §9)
constexpr int MT_BLOCKS = 512;          // 2 workgroups per CU of an MI355X
constexpr int MT_LDS_MAX = 64 * 1024;
constexpr int64_t MT_SAT = 4294967295ll;   // 2^32 - 1

static_assert(sizeof(SlRec) == 16 && sizeof(RlRec) == 32, "record layout");

// fix(x) = rint(x * 2^24), ties to even; |x| >= 256 or not finite saturates (NaN: 0) and counts
__host__ __device__ inline int64_t mt_fix(float x, int& clamped) {
  if (!(fabsf(x) < 256.f)) {
    ++clamped;
    return x != x ? 0 : x > 0.f ? MT_SAT : -MT_SAT;
  }
  return (int64_t)rint((double)x * (double)(1 << NFSP_MEMTAB_FIX_SHIFT));
}

// ---------------------------------------------------------------------------
// host: the lookup of a game (memtab_lookup.h)
// ---------------------------------------------------------------------------
}  // namespace

namespace nfsp {
namespace eng {
int mt_host(int game, const MtHost** out) {
  static std::mutex mu;
  static std::map<int, MtHost> cache;
  const nfsp::ex::HostTables* H = nullptr;
  int rc = nfsp::ex::host_tables(game, &H);
  if (rc != NFSP_OK) return rc;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(game);
  if (it == cache.end()) {
    MtHost M;
    M.ndec = (int)H->legal.size();
    for (int s = 0; s < 2; ++s)
      for (int h = 0; h < MT_H; ++h) {
        M.keys[s][h] = MT_EMPTY;
        M.vals[s][h] = 0;
      }
    for (int d = 0; d < M.ndec; ++d) {
      const int s = H->legal[d] >> 1;
      NFSP_REQUIRE((s == 0 || s == 1) && M.nrows[s] < MT_MAX_ROWS && 6 * (M.nrows[s] + 1) <= MT_H,
                   "memory table: the tree has more rows per seat than the lookup holds");
      const int c = M.nrows[s]++;
      M.rows[s][c] = d;
      for (int r = 0; r < 3; ++r) {
        const uint32_t x = H->obs[(size_t)d * 3 + r];
        uint32_t h = mt_hash(x);
        while (M.keys[s][h] != MT_EMPTY) {
          NFSP_REQUIRE(M.keys[s][h] != x, "memory table: two information sets of a seat share an observation");
          h = (h + 1) & (MT_H - 1);
        }
        M.keys[s][h] = x;
        M.vals[s][h] = (uint16_t)(c * 3 + r);
      }
    }
    it = cache.emplace(game, M).first;
  }
  *out = &it->second;
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

namespace {

// ---------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------
struct MtTab {                            // one table: a seat's records in up to MT_MAX_SEG pieces
  const uint4* p[MT_MAX_SEG];             // 16-byte aligned
  int64_t n[MT_MAX_SEG];                  // records
  int64_t* out;                           // the joint table [ndec][3][3][3] the seat's rows go to
  int32_t nseg, seat;
  const float* tw;                        // NFSP_MEM_TD: the target net (packed), gamma and the quirks;
                                          //   NFSP_MEM_TDQ: the joint Q table [ndec][3][3] in its place
  double gamma;
  uint32_t quirks, pad;
};
struct MtArgs {
  const uint32_t* keys;                   // [2][MT_H]
  const uint16_t* vals;                   // [2][MT_H]
  const int32_t* rows;                    // [2][MT_MAX_ROWS]
  const MtTab* tabs;
  int64_t* partial;                       // [tables][nb][nvp]: bins, then matched, unmatched, clamped
  int64_t* info;                          // [tables][4]
  int32_t nb, nvp;
  int32_t nrows[2];
};

__device__ inline int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline void lds_add(int64_t* p, int64_t v) {
  if (v) atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// One record (sid >= 0) into the bins.  SL: val = fix(a), the count goes to action k.  RL:
// val[0] = r in half units, val[1] = t, both to k.  TD: val[0] = fix(v), val[1] = fix(max Q) of a
// record that bootstraps, both to k; TDQ as TD.
template <int KIND>
__device__ inline void mt_accum(int64_t* bins, int sid, int k, const int64_t val[3]) {
  constexpr int NF = KIND == NFSP_MEM_SL ? 2 : 3;
  int64_t* b = bins + sid * 3 * NF;
  lds_add(b + k * NF + 0, 1);
  if (KIND == NFSP_MEM_SL) {
#pragma unroll
    for (int j = 0; j < 3; ++j) lds_add(b + j * NF + 1, val[j]);
  } else {
    lds_add(b + k * NF + 1, val[0]);
    lds_add(b + k * NF + 2, val[1]);
  }
}

// k_br_targets' TD value (br_targets_body.inc): the product and the sum each rounded, as the
// restatement of tests/tdtab_ref.py rounds them
__device__ inline float td_value(float r, float qmax, double gamma, bool terminal) {
#pragma clang fp contract(off)
  return (float)(terminal ? (double)r : (double)r + gamma * (double)qmax);
}

template <int KIND, int U>
__global__ void __launch_bounds__(MT_WG) k_memtab(MtArgs A) {
  extern __shared__ __attribute__((aligned(16))) int64_t mt_lds[];
  constexpr int NF = KIND == NFSP_MEM_SL ? 2 : 3;
  constexpr int RQ = KIND == NFSP_MEM_SL ? 1 : 2;      // 16-byte words per record
  const MtTab& T = A.tabs[blockIdx.y];
  const int seat = T.seat;
  const int nv = A.nrows[seat] * 9 * NF;
  // TD: the target net comes first; TDQ: the seat's Q rows [sid][3], an even number of floats
  const int NETQ = KIND == NFSP_MEM_TD ? NET_LDS / 2 : KIND == NFSP_MEM_TDQ ? (A.nrows[seat] * 9 + 1) / 2 : 0;
  float* sw = reinterpret_cast<float*>(mt_lds);        // TD: [NET_LDS], fwd_lds' layout and bank map
  int64_t* bins = mt_lds + NETQ;                       // [nv]
  int64_t* ctr = bins + nv;                            // matched, unmatched, clamped
  uint32_t* hk = reinterpret_cast<uint32_t*>(ctr + 4);
  uint16_t* hv = reinterpret_cast<uint16_t*>(hk + MT_H);
  for (int v = threadIdx.x; v < nv + 4; v += MT_WG) bins[v] = 0;
  for (int h = threadIdx.x; h < MT_H; h += MT_WG) {
    hk[h] = A.keys[seat * MT_H + h];
    hv[h] = A.vals[seat * MT_H + h];
  }
  if (KIND == NFSP_MEM_TD) stage_net_lds(sw, T.tw, threadIdx.x, MT_WG);
  if (KIND == NFSP_MEM_TDQ)                            // compact row c of the seat is row A.rows[c] of the joint table
    for (int v = threadIdx.x; v < A.nrows[seat] * 9; v += MT_WG) sw[v] = T.tw[A.rows[seat * MT_MAX_ROWS + v / 9] * 9 + v % 9];
  const double gamma = T.gamma;                        // TD; uniform over the workgroup, as act
  const unsigned quirks = T.quirks;
  const int act = br_act(quirks);
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = (int64_t)blockIdx.x * (MT_WG / 64) + wave, nw = (int64_t)gridDim.x * (MT_WG / 64);
  int matched = 0, unmatched = 0, clamped = 0;
  for (int s = 0; s < T.nseg; ++s) {
    const uint4* __restrict__ p = T.p[s];
    const int64_t n = T.n[s];
    // a wave takes 64 * U consecutive records per turn: the bound is the wave's, not the lane's
    for (int64_t base = gw * (64 * U); base < n; base += nw * (64 * U)) {
      uint4 rec[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t k = base + u * 64 + lane;
        rec[u] = k < n ? p[k * RQ] : make_uint4(MT_EMPTY, 0, 3, 0);    // neither a key nor an action
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool valid = base + u * 64 + lane < n;
        int sid = valid ? mt_find(hk, hv, rec[u].x) : -1;
        int k = 0;
        int64_t val[3] = {0, 0, 0};
        if (KIND == NFSP_MEM_SL) {
          if (sid >= 0) {
            const float a0 = __uint_as_float(rec[u].y), a1 = __uint_as_float(rec[u].z), a2 = __uint_as_float(rec[u].w);
            k = nfsp::argmax3(a0, a1, a2);
            val[0] = mt_fix(a0, clamped);
            val[1] = mt_fix(a1, clamped);
            val[2] = mt_fix(a2, clamped);
          }
        } else {
          k = (int)(rec[u].z & 0xFFu);
          if (k > 2) sid = -1;                          // not a stored argmax: no bin
          if (KIND == NFSP_MEM_RL) {
            val[0] = (int8_t)(rec[u].z >> 16);
            val[1] = (rec[u].z >> 8) & 1u;
          } else if (KIND == NFSP_MEM_TDQ) {
            if (sid >= 0) {
              const int sid2 = mt_find(hk, hv, rec[u].y);          // s2 is any word: a terminal one is no set
              const float qmax = sid2 < 0 ? 0.f : fmaxf(fmaxf(sw[sid2 * 3], sw[sid2 * 3 + 1]), sw[sid2 * 3 + 2]);
              const float r = (float)(int8_t)((rec[u].z >> 16) & 0xFFu) * 0.5f;
              const bool terminal = !(quirks & NFSP_QUIRK_TERMINAL_BOOTSTRAP) && ((rec[u].z >> 8) & 1u);
              val[0] = mt_fix(td_value(r, qmax, gamma, terminal), clamped);
              val[1] = terminal ? 0 : mt_fix(qmax, clamped);
            }
          } else {
            // every lane of the wave forwards (fwd_lds ballots): one without a record or a bin
            // forwards x = 0 and drops the result.  s2 is any 30-bit word, fwd_lds exact for it
            float y[3];
            fwd_lds(sw, sid >= 0 ? rec[u].y : 0u, act, y);
            if (sid >= 0) {
              const float qmax = fmaxf(fmaxf(y[0], y[1]), y[2]);
              const float r = (float)(int8_t)((rec[u].z >> 16) & 0xFFu) * 0.5f;
              const bool terminal = !(quirks & NFSP_QUIRK_TERMINAL_BOOTSTRAP) && ((rec[u].z >> 8) & 1u);
              val[0] = mt_fix(td_value(r, qmax, gamma, terminal), clamped);
              val[1] = terminal ? 0 : mt_fix(qmax, clamped);
            }
          }
        }
        matched += sid >= 0;
        unmatched += valid && sid < 0;
        if (sid >= 0) mt_accum<KIND>(bins, sid, k, val);
      }
    }
  }
  matched = wave_sum(matched);
  unmatched = wave_sum(unmatched);
  clamped = wave_sum(clamped);
  if (lane == 0) {
    lds_add(ctr + 0, matched);
    lds_add(ctr + 1, unmatched);
    lds_add(ctr + 2, clamped);
  }
  __syncthreads();
  int64_t* out = A.partial + ((int64_t)blockIdx.y * A.nb + blockIdx.x) * A.nvp;
  for (int v = threadIdx.x; v < nv; v += MT_WG) out[v] = bins[v];
  if (threadIdx.x < 3) out[A.nvp - 3 + threadIdx.x] = ctr[threadIdx.x];
}

// The partials of table blockIdx.y -> the seat's rows of the joint table (every value of every
// such row is written; field 2 of an M_SL table is 0) and its info.  A workgroup owns 64
// consecutive values; its 16 waves each add every 16th block's partial (512-byte rows, so the
// loads coalesce) and wave 0 adds the 16 sums.  One workgroup per table looping over all of its
// partials measured 0.4 ms at C3 size: 20 times the read of the records.
__global__ void __launch_bounds__(MT_WG) k_memtab_sum(MtArgs A, int kind) {
  __shared__ int64_t red[MT_WG / 64][64];
  const MtTab& T = A.tabs[blockIdx.y];
  const int seat = T.seat, NF = kind == NFSP_MEM_SL ? 2 : 3;
  const int nv = A.nrows[seat] * 9 * NF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;                    // [0, nv): a bin; [nv, nv + 3): the info
  const bool valid = j < nv + 3;
  const int64_t* part = A.partial + (int64_t)blockIdx.y * A.nb * A.nvp + (j < nv ? j : valid ? A.nvp - 3 + (j - nv) : 0);
  int64_t s = 0;
  if (valid)
    for (int b = wave; b < A.nb; b += MT_WG / 64) s += part[(int64_t)b * A.nvp];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && valid) {
    for (int w = 1; w < MT_WG / 64; ++w) s += red[w][lane];
    if (j < nv) {
      const int sid = j / (3 * NF), k = (j / NF) % 3, f = j % NF;
      int64_t* o = T.out + ((int64_t)A.rows[seat * MT_MAX_ROWS + sid / 3] * 3 + sid % 3) * 9 + k * 3;
      o[f] = s;
      if (NF == 2 && f == 1) o[2] = 0;
    } else {
      A.info[blockIdx.y * 4 + 1 + (j - nv)] = s;
    }
  }
}

// ---------------------------------------------------------------------------
// host: per-device tables and workspace, the launch
// ---------------------------------------------------------------------------
struct MtWork {
  char* buf = nullptr;
  size_t cap = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};
};
std::mutex g_mu;                          // a call holds it from its first launch to its last copy
std::map<std::pair<int, int>, MtDev> g_dev;
std::map<int, MtWork> g_work;
thread_local double g_last_ms = 0.0;

int mt_device(int dev, int game, const MtHost& M, MtDev* out) {
  auto it = g_dev.find({dev, game});
  if (it == g_dev.end()) {
    MtDev D;
    NFSP_HIP(hipMalloc((void**)&D.keys, sizeof(M.keys)));
    NFSP_HIP(hipMalloc((void**)&D.vals, sizeof(M.vals)));
    NFSP_HIP(hipMalloc((void**)&D.rows, sizeof(M.rows)));
    NFSP_HIP(hipMemcpy(D.keys, M.keys, sizeof(M.keys), hipMemcpyHostToDevice));
    NFSP_HIP(hipMemcpy(D.vals, M.vals, sizeof(M.vals), hipMemcpyHostToDevice));
    NFSP_HIP(hipMemcpy(D.rows, M.rows, sizeof(M.rows), hipMemcpyHostToDevice));
    it = g_dev.emplace(std::make_pair(dev, game), D).first;
  }
  *out = it->second;
  return NFSP_OK;
}

}  // namespace

namespace nfsp {
namespace eng {
int mt_lookup(int game, const MtHost** host, MtDev* dev) {
  int rc = mt_host(game, host);
  if (rc != NFSP_OK) return rc;
  int d = 0;
  NFSP_HIP(hipGetDevice(&d));
  std::lock_guard<std::mutex> lk(g_mu);
  return mt_device(d, game, **host, dev);
}
}  // namespace eng
}  // namespace nfsp

namespace {

// A call in three parts, all under g_mu: mt_plan sizes the launch for `nt` tables and lays the
// workspace out -- `sets` job tables (a sweep alternates between two), the info, the partials
// and `extra` bytes of the caller's behind them; mt_enqueue uploads nothing and synchronises
// nothing, it launches k_memtab and k_memtab_sum for one job table; mt_finish copies the last
// launch's info and synchronises.  K sweeps are K enqueues between one plan and one finish.
struct MtPlan {
  MtArgs A{};                             // A.tabs: job table 0
  int nt = 0, kind = 0, sets = 1;
  size_t lds = 0, b_set = 0;
  std::vector<int64_t> total;             // records per table
  char* extra = nullptr;                  // 16-byte aligned
  MtWork* W = nullptr;
};

int mt_plan(int game, int kind, const std::vector<MtTab>& tabs, int sets, size_t extra, MtPlan* P) {
  const int nt = (int)tabs.size();
  const MtHost* M = nullptr;
  int rc = mt_host(game, &M);
  if (rc != NFSP_OK) return rc;
  int64_t maxn = 0;
  P->total.assign(nt, 0);
  for (int t = 0; t < nt; ++t) {
    for (int s = 0; s < tabs[t].nseg; ++s) P->total[t] += tabs[t].n[s];
    NFSP_REQUIRE(P->total[t] < (1ll << 31), "memory table: 2^31 records or more in one table");
    maxn = P->total[t] > maxn ? P->total[t] : maxn;
  }
  const int NF = kind == NFSP_MEM_SL ? 2 : 3;
  const int nrmax = M->nrows[0] > M->nrows[1] ? M->nrows[0] : M->nrows[1];
  const int nvp = nrmax * 9 * NF + 3;
  const bool td = kind == NFSP_MEM_TD;
  const size_t front = td ? sizeof(float) * NET_LDS : kind == NFSP_MEM_TDQ ? sizeof(int64_t) * (size_t)((nrmax * 9 + 1) / 2) : 0;
  P->lds = sizeof(int64_t) * ((size_t)(nvp - 3) + 4) + MT_H * (sizeof(uint32_t) + sizeof(uint16_t)) + front;
  NFSP_REQUIRE(P->lds <= (size_t)MT_LDS_MAX, "memory table: the bins do not fit the workgroup's LDS");
  const int64_t turn = (int64_t)MT_WG * (td ? TD_U : MT_U);      // two turns of a workgroup per block
  int64_t nb = (maxn + turn * 2 - 1) / (turn * 2);
  const int64_t cap = MT_BLOCKS / nt > 1 ? MT_BLOCKS / nt : 1;
  nb = nb < 1 ? 1 : nb > cap ? cap : nb;

  int dev = 0;
  NFSP_HIP(hipGetDevice(&dev));
  MtDev D;
  if ((rc = mt_device(dev, game, *M, &D)) != NFSP_OK) return rc;
  MtWork& W = g_work[dev];
  P->b_set = (sizeof(MtTab) * nt + 15) & ~(size_t)15;
  const size_t b_info = sizeof(int64_t) * 4 * nt;
  const size_t b_part = (sizeof(int64_t) * (size_t)nt * nb * nvp + 15) & ~(size_t)15;
  const size_t need = P->b_set * sets + b_info + b_part + extra;
  if (W.cap < need) {
    if (W.buf) NFSP_HIP(hipFree(W.buf));
    W.buf = nullptr;
    W.cap = 0;
    NFSP_HIP(hipMalloc((void**)&W.buf, need));
    W.cap = need;
  }
  for (hipEvent_t& ev : W.ev)
    if (!ev) NFSP_HIP(hipEventCreate(&ev));
  MtArgs& A = P->A;
  A.keys = D.keys;
  A.vals = D.vals;
  A.rows = D.rows;
  A.tabs = reinterpret_cast<const MtTab*>(W.buf);
  A.info = reinterpret_cast<int64_t*>(W.buf + P->b_set * sets);
  A.partial = reinterpret_cast<int64_t*>(W.buf + P->b_set * sets + b_info);
  A.nb = (int32_t)nb;
  A.nvp = nvp;
  A.nrows[0] = M->nrows[0];
  A.nrows[1] = M->nrows[1];
  P->nt = nt;
  P->kind = kind;
  P->sets = sets;
  P->extra = W.buf + P->b_set * sets + b_info + b_part;
  P->W = &W;
  return NFSP_OK;
}

// job table `set` <- tabs (pageable host memory: the copy has left it when the call returns)
int mt_upload(hipStream_t st, const MtPlan& P, int set, const std::vector<MtTab>& tabs) {
  NFSP_HIP(hipMemcpyAsync(P.W->buf + P.b_set * set, tabs.data(), sizeof(MtTab) * P.nt, hipMemcpyHostToDevice, st));
  return NFSP_OK;
}

int mt_enqueue(hipStream_t st, const MtPlan& P, int set) {
  MtArgs A = P.A;
  A.tabs = reinterpret_cast<const MtTab*>(P.W->buf + P.b_set * set);
  const dim3 grid((unsigned)A.nb, (unsigned)P.nt);
  if (P.kind == NFSP_MEM_SL) k_memtab<NFSP_MEM_SL, MT_U><<<grid, MT_WG, P.lds, st>>>(A);
  else if (P.kind == NFSP_MEM_RL) k_memtab<NFSP_MEM_RL, MT_U><<<grid, MT_WG, P.lds, st>>>(A);
  else if (P.kind == NFSP_MEM_TD) k_memtab<NFSP_MEM_TD, TD_U><<<grid, MT_WG, P.lds, st>>>(A);
  else k_memtab<NFSP_MEM_TDQ, MT_U><<<grid, MT_WG, P.lds, st>>>(A);
  NFSP_LAUNCHED("k_memtab");
  k_memtab_sum<<<dim3((unsigned)((A.nvp + 63) / 64), (unsigned)P.nt), MT_WG, 0, st>>>(A, P.kind);
  NFSP_LAUNCHED("k_memtab_sum");
  return NFSP_OK;
}

// after the last enqueue (W.ev[0] recorded before the first): the one info copy, the one wait
int mt_finish(hipStream_t st, const MtPlan& P, nfsp_memtab_info* info) {
  NFSP_HIP(hipEventRecord(P.W->ev[1], st));
  std::vector<int64_t> h((size_t)4 * P.nt);
  NFSP_HIP(hipMemcpyAsync(h.data(), P.A.info, sizeof(int64_t) * 4 * P.nt, hipMemcpyDeviceToHost, st));
  NFSP_HIP(hipStreamSynchronize(st));
  float ms = 0.f;
  NFSP_HIP(hipEventElapsedTime(&ms, P.W->ev[0], P.W->ev[1]));
  g_last_ms = ms;
  for (int t = 0; t < P.nt; ++t)
    if (info) info[t] = nfsp_memtab_info{P.total[t], h[4 * t + 1], h[4 * t + 2], h[4 * t + 3]};
  return NFSP_OK;
}

// The tables of `tabs` (their `out` set) on `st`; info[t] filled; synchronises st.
int mt_run(hipStream_t st, int game, int kind, std::vector<MtTab>& tabs, nfsp_memtab_info* info) {
  if (tabs.empty()) return NFSP_OK;
  std::lock_guard<std::mutex> lk(g_mu);
  MtPlan P;
  int rc = mt_plan(game, kind, tabs, 1, 0, &P);
  if (rc != NFSP_OK || (rc = mt_upload(st, P, 0, tabs)) != NFSP_OK) return rc;
  NFSP_HIP(hipEventRecord(P.W->ev[0], st));
  if ((rc = mt_enqueue(st, P, 0)) != NFSP_OK) return rc;
  return mt_finish(st, P, info);
}

// K fitted-Q sweeps (include/nfsp.h nfsp_engine_tabular_q) over R joint tables: tabs[2r + a] is
// agent a of engine r with its segments, gamma and quirks set; its Q pointer and `out` are set
// here.  Q_0 = fill (0 where NULL); sweep j reads Q buffer j & 1 and writes the other, through the
// int64 table (dev_tab, or a scratch one of the workspace).  3K launches, one synchronisation.
int mt_sweeps(hipStream_t st, int game, std::vector<MtTab>& tabs, int sweeps, const float* dev_fill, float* dev_q,
              int64_t* dev_tab, nfsp_memtab_info* info, int32_t* changed) {
  const int nt = (int)tabs.size(), R = nt / 2;
  if (R == 0) return NFSP_OK;
  const MtHost* M = nullptr;
  int rc = mt_host(game, &M);
  if (rc != NFSP_OK) return rc;
  const size_t nq = (size_t)R * M->ndec * 9;
  const size_t b_q = (sizeof(float) * nq + 15) & ~(size_t)15, b_tab = dev_tab ? 0 : sizeof(int64_t) * nq * 3;
  const size_t b_chg = (sizeof(int32_t) * R + 15) & ~(size_t)15;
  std::lock_guard<std::mutex> lk(g_mu);
  MtPlan P;
  if ((rc = mt_plan(game, NFSP_MEM_TDQ, tabs, 2, 2 * b_q + b_chg + b_tab, &P)) != NFSP_OK) return rc;
  float* q[2] = {reinterpret_cast<float*>(P.extra), reinterpret_cast<float*>(P.extra + b_q)};
  int32_t* chg = reinterpret_cast<int32_t*>(P.extra + 2 * b_q);
  int64_t* tab = dev_tab ? dev_tab : reinterpret_cast<int64_t*>(P.extra + 2 * b_q + b_chg);
  for (int set = 0; set < 2; ++set) {
    for (int t = 0; t < nt; ++t) {
      tabs[t].tw = q[set] + (size_t)(t / 2) * M->ndec * 9;
      tabs[t].out = tab + (size_t)(t / 2) * M->ndec * 27;
    }
    if ((rc = mt_upload(st, P, set, tabs)) != NFSP_OK) return rc;
  }
  if (dev_fill) NFSP_HIP(hipMemcpyAsync(q[0], dev_fill, sizeof(float) * nq, hipMemcpyDeviceToDevice, st));
  else NFSP_HIP(hipMemsetAsync(q[0], 0, sizeof(float) * nq, st));
  NFSP_HIP(hipEventRecord(P.W->ev[0], st));
  for (int j = 0; j < sweeps; ++j) {
    if ((rc = mt_enqueue(st, P, j & 1)) != NFSP_OK) return rc;
    if ((rc = table_rows_enqueue(st, M->ndec, NFSP_ROWS_TD_MEAN, tab, dev_fill, q[j & 1], R, q[(j + 1) & 1], chg)) != NFSP_OK)
      return rc;
  }
  NFSP_HIP(hipMemcpyAsync(dev_q, q[sweeps & 1], sizeof(float) * nq, hipMemcpyDeviceToDevice, st));
  std::vector<int32_t> hc(R);
  NFSP_HIP(hipMemcpyAsync(hc.data(), chg, sizeof(int32_t) * R, hipMemcpyDeviceToHost, st));
  if ((rc = mt_finish(st, P, info)) != NFSP_OK) return rc;
  for (int r = 0; r < R; ++r)
    if (changed) changed[r] = hc[r];
  return NFSP_OK;
}

int mt_seg(MtTab& T, const void* p, int64_t n) {
  if (n <= 0) return NFSP_OK;
  NFSP_REQUIRE(T.nseg < MT_MAX_SEG, "memory table: too many segments");
  T.p[T.nseg] = static_cast<const uint4*>(p);
  T.n[T.nseg++] = n;
  return NFSP_OK;
}

// agent a's table of an engine at a step boundary (A: the agent's view, mem_view.h); TD: with the
// agent's own target net, gamma and quirks; TDQ: with these two, the Q rows being mt_sweeps'
int mt_engine_tab(nfsp_engine* e, const AgentView& A, int kind, int a, int64_t* out, MtTab* T) {
  *T = MtTab{};
  T->seat = a;
  T->out = out;
  if (kind == NFSP_MEM_TD) {
    T->tw = e->w + (a * 3 + 2) * nfsp::nn::NP;       // NET_TARGET
  }
  if (kind == NFSP_MEM_TD || kind == NFSP_MEM_TDQ) {
    T->gamma = e->cfg.gamma;
    T->quirks = e->cfg.quirks;
  }
  if (kind == NFSP_MEM_SL) return mt_seg(*T, A.sl, A.sl_n);
  for (int k = 0; k < A.n_rl; ++k) {
    int rc = mt_seg(*T, A.rl[k], A.rl_n[k]);
    if (rc != NFSP_OK) return rc;
  }
  return NFSP_OK;
}

bool kind_ok(int kind) { return kind == NFSP_MEM_SL || kind == NFSP_MEM_RL; }

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfsp_memtab_lookup(int game, int seat, uint32_t obs) {
  const MtHost* M = nullptr;
  if (mt_host(game, &M) != NFSP_OK || (seat != 0 && seat != 1)) return -1;
  const int sid = mt_find(M->keys[seat], M->vals[seat], obs);
  return sid < 0 ? -1 : M->rows[seat][sid / 3] * 3 + sid % 3;
}

extern "C" int64_t nfsp_memtab_fix(float x) {
  int clamped = 0;
  return mt_fix(x, clamped);
}

extern "C" int nfsp_memtab_last_ms(double* ms) {
  NFSP_REQUIRE(ms, "null argument");
  *ms = g_last_ms;
  return NFSP_OK;
}

namespace {

// the raw forms: one seat's table of the caller's segments (td: NFSP_MEM_TD's arguments, or
// NFSP_MEM_TDQ's with the Q table as dev_target_w)
int mt_raw(nfsp_ctx* ctx, int game, int kind, int seat, const nfsp_mem_segment* segs, int nsegs, const nfsp_td_args* td,
           int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(ctx && dev_out && (segs || nsegs == 0), "null argument");
  NFSP_REQUIRE(seat == 0 || seat == 1, "memory table: bad kind or seat");
  NFSP_REQUIRE(nsegs >= 0 && nsegs <= NFSP_MEMTAB_MAX_SEGMENTS, "memory table: too many segments");
  std::vector<MtTab> tabs(1);
  tabs[0].seat = seat;
  tabs[0].out = dev_out;
  if (td) {
    tabs[0].tw = td->dev_target_w;
    tabs[0].gamma = td->gamma;
    tabs[0].quirks = td->quirks;
  }
  int64_t total = 0;
  for (int s = 0; s < nsegs; ++s) {
    NFSP_REQUIRE(segs[s].n >= 0 && (segs[s].dev_recs || segs[s].n == 0), "memory table: bad segment");
    NFSP_REQUIRE(((uintptr_t)segs[s].dev_recs & 15u) == 0, "memory table: records must be 16-byte aligned");
    NFSP_REQUIRE(segs[s].n < (1ll << 31) && (total += segs[s].n) < (1ll << 31),
                 "memory table: 2^31 records or more in one table");
    int rc = mt_seg(tabs[0], segs[s].dev_recs, segs[s].n);
    if (rc != NFSP_OK) return rc;
  }
  return mt_run(ctx->stream, game, kind, tabs, info);
}

int mt_engine(nfsp_engine* e, const char* what, int kind, int64_t* dev_out, nfsp_memtab_info info[2]) {
  MemView v;
  int rc = engine_view(e, what, &v);
  if (rc != NFSP_OK) return rc;
  std::vector<MtTab> tabs(2);
  for (int a = 0; a < 2; ++a)
    if ((rc = mt_engine_tab(e, v.agent[a], kind, a, dev_out, &tabs[a])) != NFSP_OK) return rc;
  return mt_run(e->ctx->stream, e->ctx->game, kind, tabs, info);
}

int mt_group(nfsp_group* g, const char* what, int kind, int64_t* dev_out, nfsp_memtab_info* info) {
  GroupState G;
  std::vector<MemView> v;
  int rc = group_view(g, what, &G, &v);
  if (rc != NFSP_OK) return rc;
  const MtHost* M = nullptr;
  if ((rc = mt_host(G.ctx->game, &M)) != NFSP_OK) return rc;
  std::vector<MtTab> tabs((size_t)2 * G.R);
  for (int r = 0; r < G.R; ++r)
    for (int a = 0; a < 2; ++a)
      if ((rc = mt_engine_tab(G.eng[r], v[r].agent[a], kind, a, dev_out + (int64_t)r * M->ndec * 27, &tabs[2 * r + a])) != NFSP_OK)
        return rc;
  return mt_run(G.ctx->stream, G.ctx->game, kind, tabs, info);
}

}  // namespace

extern "C" int nfsp_memory_table(nfsp_ctx* ctx, int game, int kind, int seat, const nfsp_mem_segment* segs, int nsegs,
                                 int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(kind_ok(kind), "memory table: bad kind or seat");
  return mt_raw(ctx, game, kind, seat, segs, nsegs, nullptr, dev_out, info);
}

extern "C" int nfsp_engine_memory_table(nfsp_engine* e, int kind, int64_t* dev_out, nfsp_memtab_info info[2]) {
  NFSP_REQUIRE(e && dev_out, "null argument");
  NFSP_REQUIRE(kind_ok(kind), "memory table: bad kind");
  return mt_engine(e, "nfsp_engine_memory_table", kind, dev_out, info);
}

extern "C" int nfsp_group_memory_tables(nfsp_group* g, int kind, int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(g && dev_out, "null argument");
  NFSP_REQUIRE(kind_ok(kind), "memory table: bad kind");
  return mt_group(g, "nfsp_group_memory_tables", kind, dev_out, info);
}

extern "C" int nfsp_td_table(nfsp_ctx* ctx, int game, int seat, const nfsp_mem_segment* segs, int nsegs,
                             const nfsp_td_args* td, int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(td && td->dev_target_w, "null argument");
  NFSP_REQUIRE(td->reserved == 0, "nfsp_td_args.reserved must be 0");
  NFSP_REQUIRE(((uintptr_t)td->dev_target_w & 3u) == 0, "TD table: the target net must be 4-byte aligned");
  return mt_raw(ctx, game, NFSP_MEM_TD, seat, segs, nsegs, td, dev_out, info);
}

extern "C" int nfsp_engine_td_table(nfsp_engine* e, int64_t* dev_out, nfsp_memtab_info info[2]) {
  NFSP_REQUIRE(e && dev_out, "null argument");
  return mt_engine(e, "nfsp_engine_td_table", NFSP_MEM_TD, dev_out, info);
}

extern "C" int nfsp_group_td_tables(nfsp_group* g, int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(g && dev_out, "null argument");
  return mt_group(g, "nfsp_group_td_tables", NFSP_MEM_TD, dev_out, info);
}

extern "C" int nfsp_tdq_table(nfsp_ctx* ctx, int game, int seat, const nfsp_mem_segment* segs, int nsegs, const float* dev_q,
                              double gamma, uint32_t quirks, int64_t* dev_out, nfsp_memtab_info* info) {
  NFSP_REQUIRE(dev_q, "null argument");
  NFSP_REQUIRE(((uintptr_t)dev_q & 3u) == 0, "TDQ table: the Q table must be 4-byte aligned");
  const nfsp_td_args td{dev_q, gamma, quirks, 0};
  return mt_raw(ctx, game, NFSP_MEM_TDQ, seat, segs, nsegs, &td, dev_out, info);
}

namespace {
int tq_args(int sweeps, const float* dev_fill, float* dev_q, int64_t* dev_tab) {
  NFSP_REQUIRE(dev_q, "null argument");
  NFSP_REQUIRE(sweeps >= 1 && sweeps <= NFSP_TABQ_MAX_SWEEPS, "tabular Q: sweeps must be in [1, 64]");
  NFSP_REQUIRE((((uintptr_t)dev_fill | (uintptr_t)dev_q) & 3u) == 0 && ((uintptr_t)dev_tab & 7u) == 0,
               "tabular Q: misaligned table");
  return NFSP_OK;
}
}  // namespace

extern "C" int nfsp_engine_tabular_q(nfsp_engine* e, int sweeps, const float* dev_fill, float* dev_q, int64_t* dev_tab,
                                     nfsp_memtab_info info[2], int32_t* changed) {
  NFSP_REQUIRE(e, "null argument");
  int rc = tq_args(sweeps, dev_fill, dev_q, dev_tab);
  if (rc != NFSP_OK) return rc;
  MemView v;
  if ((rc = engine_view(e, "nfsp_engine_tabular_q", &v)) != NFSP_OK) return rc;
  std::vector<MtTab> tabs(2);
  for (int a = 0; a < 2; ++a)
    if ((rc = mt_engine_tab(e, v.agent[a], NFSP_MEM_TDQ, a, nullptr, &tabs[a])) != NFSP_OK) return rc;
  return mt_sweeps(e->ctx->stream, e->ctx->game, tabs, sweeps, dev_fill, dev_q, dev_tab, info, changed);
}

extern "C" int nfsp_group_tabular_q(nfsp_group* g, int sweeps, const float* dev_fill, float* dev_q, int64_t* dev_tab,
                                    nfsp_memtab_info* info, int32_t* changed) {
  NFSP_REQUIRE(g, "null argument");
  int rc = tq_args(sweeps, dev_fill, dev_q, dev_tab);
  if (rc != NFSP_OK) return rc;
  GroupState G;
  std::vector<MemView> v;
  if ((rc = group_view(g, "nfsp_group_tabular_q", &G, &v)) != NFSP_OK) return rc;
  std::vector<MtTab> tabs((size_t)2 * G.R);
  for (int r = 0; r < G.R; ++r)
    for (int a = 0; a < 2; ++a)
      if ((rc = mt_engine_tab(G.eng[r], v[r].agent[a], NFSP_MEM_TDQ, a, nullptr, &tabs[2 * r + a])) != NFSP_OK) return rc;
  return mt_sweeps(G.ctx->stream, G.ctx->game, tabs, sweeps, dev_fill, dev_q, dev_tab, info, changed);
}
