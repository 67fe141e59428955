// The full-batch step of nets fitted to tables (include/nfsp.h nfsp_fit_tables states it), shared
// by the two kernels that run it with a net, its momentum state and a seat's rows in LDS:
// k_fit_tables (fit_tables.hip) and k_mccfr_net_apply (mccfr.hip).  One workgroup of FIT_WG
// threads per net; every function here is called by all of them with workgroup-uniform arguments.
// The body of the step loop is fit_step_body.inc, included where the loop stands: as a function it
// cost k_fit_tables a scalar register (78 for 77), and that kernel's code is to stay as it was.
//
// The hidden width H is a parameter of the step: a packed net is W1[30][H] | b1[H] | W2[H][3] | b2[3],
// NP(H) = 34 H + 3 floats at the offsets 0, 30 H, 31 H, 34 H (Width<H>).  The two kernels above are
// the width-64 ones, written against nn::H and the constants below as before; every other supported
// width (FIT_WIDTHS) is an instantiation of k_fit_tables_w<H> / k_mccfr_net_apply_w<H>, the same
// kernel text (fit_tables_kernel.inc, mccfr_net_apply_kernel.inc) under FIT_WIDTH_NAMES(H).  128
// is the largest width whose carve fits one workgroup's LDS on Leduc (147,744 B); FIT_WG >= 3 H + 3
// holds up to it.
//
// Per step, f32 with fp contract off, every gradient from the weights before the step:
//   z1[b][j]  = (sum over the SET bits i of obs[b], ascending, of W1[i][j]) + b1[j]
//               -- the bits of sgd_step's 30-input sum for finite weights: x is 0 or 1, and adding
//               0 * w = +-0 to a sum that started at +0 changes no bit
//   z[b][k]   = (sum over j ascending of relu(z1[b][j]) * W2[j][k]) + b2[k]
//   dz[b][k]  per row, as include/nfsp.h states for the (head, loss) pair
//   dW2[j][k] = sum over rows b ascending of relu(z1[b][j]) * dz[b][k];  db2[k] = sum_b dz[b][k]
//   dz1[b][j] = z1[b][j] > 0 ? (dz[b][0] W2[j][0] + dz[b][1] W2[j][1]) + dz[b][2] W2[j][2] : 0
//   dW1[i][j] = sum over the rows b with bit i set, ascending, of dz1[b][j];  db1[j] = sum_b dz1[b][j]
//   v <- mu v + g,  w <- w - lr v
// Every sum starts at +0 and runs in the order above, fixed by the net's rows alone: one thread
// owns one parameter, so no partial sums, no atomics, and the grid does not enter.  A zero-weight
// row and a masked entry contribute dz = +-0 and change no bit.
#ifndef NFSP_FIT_STEP_H
#define NFSP_FIT_STEP_H
#include <math.h>
#include <stdint.h>

#include "nfsp.h"
#include "nn_device.h"

namespace nfsp {
namespace fit {
namespace {

using namespace nfsp::nn;
using nfsp::NA;
using nfsp::OBS;

constexpr int FIT_WG = 512;
constexpr int FIT_SEAT_ROWS = 128;            // decision rows of one seat (Leduc: 65, Kuhn: 4)
constexpr int ZS = H + 1;                     // z1's row stride: breaks the 64-float stride of column walks
constexpr int NPP = (NP + 3) & ~3;            // keeps every carve offset a multiple of 16 bytes
static_assert(FIT_WG >= H * NA + NA, "one W2 / b2 entry per thread");

// the layout of a packed net of width HH; Width<nn::H> is nn's
template <int HH>
struct Width {
  static constexpr int H = HH, NP = OBS * HH + HH + HH * NA + NA;
  static constexpr int OW1 = 0, OB1 = OBS * HH, OW2 = OB1 + HH, OB2 = OW2 + HH * NA;
  static constexpr int ZS = HH + 1, NPP = (NP + 3) & ~3;
  static_assert(FIT_WG >= HH * NA + NA, "one W2 / b2 entry per thread");
};
static_assert(Width<nn::H>::NP == nn::NP && Width<nn::H>::OB2 == nn::OB2 && Width<nn::H>::NPP == NPP, "Width<64> is nn's");

// The names the shared kernel text and fit_step_body.inc use, for width HH, inside a kernel
// instantiated per width; the width-64 kernels see nn's and this header's instead.
#define FIT_WIDTH_NAMES(HH)                                                                                   \
  constexpr int H = nfsp::fit::Width<HH>::H, NP = nfsp::fit::Width<HH>::NP, OW1 = nfsp::fit::Width<HH>::OW1,   \
                OB1 = nfsp::fit::Width<HH>::OB1, OW2 = nfsp::fit::Width<HH>::OW2, OB2 = nfsp::fit::Width<HH>::OB2, \
                ZS = nfsp::fit::Width<HH>::ZS;                                                                \
  (void)OW1; (void)OB1

// the supported widths, and whether `hidden` is one
constexpr int FIT_WIDTHS[4] = {16, 32, 64, 128};
inline bool fit_width_ok(int hidden) { return hidden == 16 || hidden == 32 || hidden == 64 || hidden == 128; }
inline size_t fit_np(int hidden) { return (size_t)(OBS + 1 + NA) * hidden + NA; }
#define NFSP_FIT_WIDTHS_TEXT "16, 32, 64 and 128"

// LDS carve, in floats, for at most nm (a multiple of 4) rows
struct FitLds {
  float *w, *v, *t, *m, *wh, *o, *dz, *lt, *z;
  uint32_t* x;
};
__host__ __device__ inline size_t fit_lds_floats(int nm) { return 2 * (size_t)NPP + (size_t)nm * (3 + 4 * NA + ZS); }
inline size_t fit_lds_floats_h(int hidden, int nm) {
  return 2 * ((fit_np(hidden) + 3) & ~(size_t)3) + (size_t)nm * (3 + 4 * NA + hidden + 1);
}
template <int HH = nn::H>
__device__ inline FitLds fit_carve(char* raw, int nm) {
  constexpr int NPP = Width<HH>::NPP;
  FitLds S;
  S.w = (float*)raw;
  S.v = S.w + NPP;
  S.x = (uint32_t*)(S.v + NPP);
  S.wh = (float*)(S.x + nm);
  S.lt = S.wh + nm;
  S.t = S.lt + nm;
  S.m = S.t + NA * nm;
  S.o = S.m + NA * nm;
  S.dz = S.o + NA * nm;
  S.z = S.dz + NA * nm;
  return S;
}

// z1 and the raw head sums of every row from the weights in LDS; ends behind a barrier
template <int HH = nn::H>
__device__ inline void fit_forward(const FitLds& S, int N) {
#pragma clang fp contract(off)
  constexpr int H = Width<HH>::H, OW1 = Width<HH>::OW1, OB1 = Width<HH>::OB1, OW2 = Width<HH>::OW2,
                OB2 = Width<HH>::OB2, ZS = Width<HH>::ZS;
  const int tid = threadIdx.x;
  for (int e = tid; e < N * H; e += FIT_WG) {
    const int b = e / H, j = e - b * H;
    uint32_t bits = S.x[b];
    float acc = 0.f;
    while (bits) {
      const int i = __builtin_ctz(bits);
      bits &= bits - 1;
      acc = acc + S.w[OW1 + i * H + j];
    }
    S.z[b * ZS + j] = acc + S.w[OB1 + j];
  }
  __syncthreads();
  for (int e = tid; e < N * NA; e += FIT_WG) {
    const int b = e / NA, k = e - b * NA;
    float acc = 0.f;
    for (int j = 0; j < H; ++j) {
      const float z = S.z[b * ZS + j];
      acc = acc + (z > 0.f ? z : 0.f) * S.w[OW2 + j * NA + k];
    }
    S.o[e] = acc + S.w[OB2 + k];
  }
  __syncthreads();
}

// dz and the loss term of every row from the head sums; ends behind a barrier
__device__ inline void fit_rows(const FitLds& S, int N, int head, int loss) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b < N; b += FIT_WG) {
    const float z[3] = {S.o[3 * b], S.o[3 * b + 1], S.o[3 * b + 2]};
    const float t[3] = {S.t[3 * b], S.t[3 * b + 1], S.t[3 * b + 2]};
    const float wh = S.wh[b];
    float d[3], l;
    if (loss == NFSP_FIT_CE) {
      const float mx = fmaxf(fmaxf(z[0], z[1]), z[2]);
      const float c0 = z[0] - mx, c1 = z[1] - mx, c2 = z[2] - mx;
      const float e0 = expf(c0), e1 = expf(c1), e2 = expf(c2);
      const float s = (e0 + e1) + e2;
      const float T = (t[0] + t[1]) + t[2];
      d[0] = wh * ((e0 / s) * T - t[0]);
      d[1] = wh * ((e1 / s) * T - t[1]);
      d[2] = wh * ((e2 / s) * T - t[2]);
      const float ls = logf(s);
      l = -((t[0] * (c0 - ls) + t[1] * (c1 - ls)) + t[2] * (c2 - ls));
    } else {
      float lk[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const bool on = head == NFSP_ACT_LINEAR || z[k] > 0.f;
        const float e = (on ? z[k] : 0.f) - t[k];
        const float a = fabsf(e);
        const bool clip = loss == NFSP_FIT_HUBER && a > 1.0f;
        const float g = clip ? (e > 0.f ? 1.0f : -1.0f) : e;
        d[k] = on ? (wh * S.m[3 * b + k]) * g : 0.f;
        lk[k] = S.m[3 * b + k] * (clip ? a - 0.5f : (0.5f * e) * e);
      }
      l = (lk[0] + lk[1]) + lk[2];
    }
    S.dz[3 * b] = d[0];
    S.dz[3 * b + 1] = d[1];
    S.dz[3 * b + 2] = d[2];
    S.lt[b] = wh * l;
  }
  __syncthreads();
}

}  // namespace
}  // namespace fit
}  // namespace nfsp
#endif  // NFSP_FIT_STEP_H
