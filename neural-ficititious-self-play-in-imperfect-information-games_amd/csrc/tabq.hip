// From the memory tables' integers to the f32 rows a slot acts on (include/nfsp.h nfsp_table_rows;
// DESIGN.md §9, tabular NFSP).  k_table_rows turns one joint int64 table [ndec][3][3][3]
// (memtab.hip) into [ndec][3][3] floats: the mean TD value per (set, action) -- the step that
// closes a fitted-Q sweep, memtab.hip mt_sweeps -- or M_SL's average strategy by mass or by
// argmax counts.  An entry (a whole row for M_SL) without data takes the caller's `fill`.  It also
// counts the entries whose bits differ from a previous table's: a sweep's convergence test.
//
// One workgroup of 256 per table, an entry per lane and turn: at most 130 x 9 entries, so the
// launch is latency, and the count is reduced by shuffles, then over the 4 waves through LDS,
// and stored by one lane -- no global atomics, one barrier outside every loop.
#include "memtab_lookup.h"
#include "nfsp_internal.h"

using namespace nfsp::eng;

namespace {

constexpr int TR_WG = 256;

// One entry e = (row * 3 + rank) * 3 + action of table `tab`; *ok: whether the data decide it.
__device__ inline float row_value(const int64_t* __restrict__ tab, int e, int stat, bool* ok) {
#pragma clang fp contract(off)
  if (stat == NFSP_ROWS_TD_MEAN) {
    const int64_t c = tab[e * 3], S = tab[e * 3 + 1];
    *ok = c > 0;
    return (float)(((double)S / (double)(c > 0 ? c : 1)) * (1.0 / (double)(1 << NFSP_MEMTAB_FIX_SHIFT)));
  }
  const int64_t* t = tab + (e / 3) * 9;                  // the set's three actions x three fields
  const int64_t n = t[0] + t[3] + t[6];
  const int64_t m0 = t[1], m1 = t[4], m2 = t[7], M = (m0 + m1) + m2;
  *ok = n > 0 && M > 0 && m0 >= 0 && m1 >= 0 && m2 >= 0;
  const int f = stat == NFSP_ROWS_SL_MASS ? 1 : 0;
  const int64_t den = stat == NFSP_ROWS_SL_MASS ? M : n;
  return (float)((double)t[(e % 3) * 3 + f] / (double)(*ok ? den : 1));
}

__global__ void __launch_bounds__(TR_WG) k_table_rows(const int64_t* __restrict__ tab, const float* fill,
                                                      const float* prev, int ndec, int stat, float* rows, int32_t* changed) {
  __shared__ int red[TR_WG / 64];
  const size_t at = (size_t)blockIdx.x * ndec * 9;
  tab += at * 3;
  int diff = 0;
  for (int e = threadIdx.x; e < ndec * 9; e += TR_WG) {
    bool ok;
    float v = row_value(tab, e, stat, &ok);
    if (!ok) v = fill ? fill[at + e] : 0.f;
    if (prev) diff += __float_as_uint(prev[at + e]) != __float_as_uint(v);   // read before the store: prev may be rows
    rows[at + e] = v;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) diff += __shfl_xor(diff, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = diff;
  __syncthreads();
  if (threadIdx.x == 0 && changed) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < TR_WG / 64; ++w) s += red[w];
    changed[blockIdx.x] = s;
  }
}

}  // namespace

namespace nfsp {
namespace eng {
int table_rows_enqueue(hipStream_t st, int ndec, int stat, const int64_t* dev_tab, const float* dev_fill,
                       const float* dev_prev, int n, float* dev_rows, int32_t* dev_changed) {
  if (n <= 0) return NFSP_OK;
  k_table_rows<<<(unsigned)n, TR_WG, 0, st>>>(dev_tab, dev_fill, dev_prev, ndec, stat, dev_rows, dev_changed);
  NFSP_LAUNCHED("k_table_rows");
  return NFSP_OK;
}
}  // namespace eng
}  // namespace nfsp

extern "C" int nfsp_table_rows(nfsp_ctx* ctx, int game, int stat, const int64_t* dev_tab, const float* dev_fill,
                               const float* dev_prev, int n, float* dev_rows, int32_t* dev_changed) {
  NFSP_REQUIRE(ctx && (n == 0 || (dev_tab && dev_rows)), "null argument");
  NFSP_REQUIRE(stat == NFSP_ROWS_SL_MASS || stat == NFSP_ROWS_SL_ARGMAX || stat == NFSP_ROWS_TD_MEAN, "table rows: bad stat");
  NFSP_REQUIRE(n >= 0 && n <= NFSP_TABLE_ROWS_MAX, "table rows: bad table count");
  NFSP_REQUIRE(((uintptr_t)dev_tab & 7u) == 0 && (((uintptr_t)dev_fill | (uintptr_t)dev_prev | (uintptr_t)dev_rows |
                                                   (uintptr_t)dev_changed) & 3u) == 0,
               "table rows: misaligned table");
  const MtHost* M = nullptr;
  int rc = mt_host(game, &M);
  if (rc != NFSP_OK) return rc;
  if ((rc = table_rows_enqueue(ctx->stream, M->ndec, stat, dev_tab, dev_fill, dev_prev, n, dev_rows, dev_changed)) != NFSP_OK)
    return rc;
  NFSP_HIP(hipStreamSynchronize(ctx->stream));
  return NFSP_OK;
}
