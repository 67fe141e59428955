// The lookup (seat, observation) -> information set that memtab.hip builds per game: an
// open-addressing table over the evaluator's rows (exploit_tree.h), shared by the memory tables'
// kernel (memtab.hip k_memtab) and the rollout's table variant (rollout.hip, tables that act).
// memtab.hip owns the host table and its per-device copies; both kernels stage a seat's keys and
// values to LDS and probe them with mt_find.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nfsp {
namespace eng {

constexpr int MT_H = 1024;              // hash slots per seat (Leduc: 195 keys)
constexpr int MT_HSHIFT = 22;           // 32 - log2(MT_H)
constexpr uint32_t MT_EMPTY = 0xFFFFFFFFu;   // no observation has bits 30, 31
constexpr int MT_MAX_ROWS = 128;        // decision rows of one seat (Leduc: 65)
static_assert(1 << (32 - MT_HSHIFT) == MT_H, "hash width");

__host__ __device__ inline uint32_t mt_hash(uint32_t x) { return (x * 0x9E3779B1u) >> MT_HSHIFT; }

// host: the lookup of a game
struct MtHost {
  int ndec = 0;
  int nrows[2] = {0, 0};
  int32_t rows[2][MT_MAX_ROWS];          // the seat's compact row -> decision row
  uint32_t keys[2][MT_H];
  uint16_t vals[2][MT_H];                // sid = 3 x compact row + rank
};

// sid of (seat, obs), -1: none.  The table is at most a third full, so a probe ends.
__host__ __device__ inline int mt_find(const uint32_t* keys, const uint16_t* vals, uint32_t x) {
  uint32_t h = mt_hash(x);
  for (int n = 0; n < MT_H; ++n) {
    const uint32_t k = keys[h];
    if (k == x) return vals[h];
    if (k == MT_EMPTY) return -1;
    h = (h + 1) & (MT_H - 1);
  }
  return -1;
}

// the current device's copies of a game's lookup (made on first use and kept)
struct MtDev {
  uint32_t* keys = nullptr;              // [2][MT_H]
  uint16_t* vals = nullptr;              // [2][MT_H]
  int32_t* rows = nullptr;               // [2][MT_MAX_ROWS]
};

// memtab.hip: the host lookup of `game` (built once), and with it the current device's copies
int mt_host(int game, const MtHost** out);
int mt_lookup(int game, const MtHost** host, MtDev* dev);

// tabq.hip: k_table_rows for n tables on `st` (include/nfsp.h nfsp_table_rows; no synchronisation)
int table_rows_enqueue(hipStream_t st, int ndec, int stat, const int64_t* dev_tab, const float* dev_fill,
                       const float* dev_prev, int n, float* dev_rows, int32_t* dev_changed);

}  // namespace eng
}  // namespace nfsp
