// The host side of the persistent group BR kernel (br_persist.hip, nfsp_group_sched.br_persist),
// as group.hip's learner call uses it: the kernel's bail flags, its tables within the call's
// table set, and its launch.  The kernel, its protocol and its arguments are br_persist.hip's.
#pragma once
#include "learner_internal.h"

namespace nfsp {
namespace eng {

constexpr int BRP_CHUNK = 16;               // updates per chain piece (readiness is checked per piece)

// The bail flags: int32_t[4], pinned host memory mapped into the device, zeroed.  The kernel's
// waits are bounded: a hand-off that never came ends it with the flags set.  brp_flags_take
// reports (NFSP_EHIP) and clears them; call it once the kernel has completed.
hipError_t brp_flags_alloc(int32_t** flags);
void brp_flags_free(int32_t* flags);
int brp_flags_take(int32_t* flags);

// Offsets of the kernel's tables in the call's table set, in this order
struct BrpTabs {
  size_t seg_job, seg_tgt, seg_chunk0, job_seg0, slots, ctr, chunk_done;
};
BrpTabs brp_tabs_take(TabCursor& cur, const plan::PersistPlan& q);
// the host side of the tables: every segment's chain and targets job (of eng[r], L[r]), the
// queue with the first segments' items, zeroed counters
void brp_tabs_fill(char* h_tab, const BrpTabs& o, const plan::PersistPlan& q, nfsp_engine* const* eng,
                   const LearnPlan* L);
// The whole BR call in one launch on `s` (none if the plan has no BR work).  d_tab: the device
// copy of the table set; cfg: replica 0's (batch, epochs; gamma, lr_br and quirks are the same
// in every replica); spin: the bound of every wait in s_sleep 8 rounds (<= 1: the default).
int brp_launch(char* d_tab, const BrpTabs& o, const plan::PersistPlan& q, const nfsp_engine_cfg& cfg, int spin,
               int32_t* flags, hipStream_t s);

}  // namespace eng
}  // namespace nfsp
