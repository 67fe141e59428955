// Device code that the two writers of BR targets share -- k_br_targets (learner.hip, one workgroup
// per update) and the helper workgroups of the persistent group BR kernel (br_persist.hip): one
// update's targets (br_targets_item), the step records they end in (emit_recs, also k_ar_prep's),
// and the helpers that make a job field loaded into VGPRs scalar again.  In an unnamed namespace:
// each translation unit inlines its own copy, as when learner.hip held them.
#pragma once
#include "learner_internal.h"

namespace nfsp {
namespace eng {
namespace {

// A workgroup-uniform value that arrived in VGPRs (a job read with vector loads), in SGPRs again:
// readfirstlane per 32-bit half.  The compiler then knows it is uniform -- scalar branches and
// arithmetic, and no readfirstlane loop around every buffer descriptor built from it.
__device__ __forceinline__ uint32_t uniform32(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  const uint32_t lo = uniform32((uint32_t)x), hi = uniform32((uint32_t)(x >> 32));
  return ((uint64_t)hi << 32) | lo;
}
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p) { return reinterpret_cast<T*>(uniform64(reinterpret_cast<uint64_t>(p))); }
__device__ __forceinline__ double uniform_f64(double x) {
  return __longlong_as_double((long long)uniform64((uint64_t)__double_as_longlong(x)));
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

// One BR update's targets by the calling workgroup (256 threads), for k_br_persist's helpers:
// k_br_targets' body (learner.hip includes the same file; as a call of this function the kernel
// came out with another register allocation).  bx: the update within J's segment; gamma, quirks,
// lr0: the job's own, scalar.
__device__ __forceinline__ void br_targets_item(const TargetJob J, int64_t bx, int B, int E, double gamma,
                                                unsigned quirks, double lr0) {
#include "br_targets_body.inc"
}

}  // namespace
}  // namespace eng
}  // namespace nfsp
