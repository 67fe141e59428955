// The BR work plan of an engine group's learner call (group.hip group_update), as pure host
// functions over segment lists: which piece of which (replica, agent) job runs in which round
// of which partition, where each segment's targets are launched, and the persistent kernel's
// chunked work queue.  Standard headers only, so the invariants are tested without a GPU
// (tests/test_group_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "learn_plan.h"   // Segment

namespace nfsp {
namespace plan {

// job 2 r + a: the segments of (replica r, agent a) in order; null or empty: no BR work
using Jobs = std::vector<const std::vector<Segment>*>;

struct Piece {         // one chain workgroup of a round: updates [u, v) of job (r, a)
  int r, a;
  int64_t u, v;
  bool sync;           // the last piece of a syncing segment
};
struct SegRef {        // segment `seg` of job (r, a)
  int r, a;
  size_t seg;
};
struct Round {
  int p;                   // partition (stream)
  size_t b0, b1, t0, t1;   // its pieces / targets in RoundsPlan::pieces / targets
  int64_t rn;              // the longest segment starting in it (targets grid)
};
struct RoundsPlan {
  std::vector<Piece> pieces;
  std::vector<SegRef> targets;
  std::vector<Round> rounds;
  int64_t max_rounds = 0;  // the largest round count over the partitions
};

// partition p of nbs holds replicas [part_begin(p), part_begin(p + 1))
inline int part_begin(int p, int R, int nbs) { return p * R / nbs; }

// BR rounds: round k = one targets launch (the targets of the segments that start in it, whole
// segments) + one chain launch (every (replica, agent) with BR work left: the next piece of its
// current segment, at most `cap` updates; a target sync ends the last piece of its segment).
// cap 0: one round per segment index, every job's k-th segment in round k.
// A round lasts as long as its longest piece, so with whole segments the round structure waits
// for the longest segment of every round: a sliced group's BR stream ran 1.9 ms per slice
// against 1.2 ms for its busiest job (tools/group_timeline.py).  A segment's pieces resume
// from the weights in memory: the same SGD steps, bit for bit.
// Partitions: each runs its own rounds over its own replicas' jobs (on its own stream), so a
// round waits only for the longest piece among its partition's jobs.  Each job's pieces and
// targets are the same as with one partition, so are its SGD steps.
inline void plan_rounds(const Jobs& jobs, int R, int nbs, int64_t cap, bool pace_br, RoundsPlan& out) {
  struct Cursor {
    int r, a;
    size_t s;        // current segment
    int64_t pos;     // next update of it
  };
  out = RoundsPlan{};
  for (int p = 0; p < nbs; ++p) {
    std::vector<Cursor> bc;
    for (int r = part_begin(p, R, nbs); r < part_begin(p + 1, R, nbs); ++r)
      for (int a = 0; a < 2; ++a)
        if (jobs[2 * r + a] && !jobs[2 * r + a]->empty()) bc.push_back({r, a, 0, (*jobs[2 * r + a])[0].u});
    // Paced pieces (capped groups): the partition's busiest job (most BR updates in this call)
    // splits each of its segments into equal pieces of at most `cap`, and in every round the
    // other jobs take at most the busiest job's piece of that round, so no round outlasts the
    // busiest job's own piece and its last piece of a segment is not a short one.  (Plain caps:
    // a 150-update segment ran as 40 + 40 + 40 + 30, and every job's round took 40.)
    std::vector<int64_t> pace;                 // the busiest job's piece per round
    if (cap > 0 && pace_br) {
      int64_t most = -1;
      const std::vector<Segment>* bs = nullptr;
      for (const Cursor& c : bc) {
        int64_t n = 0;
        for (const Segment& sg : *jobs[2 * c.r + c.a]) n += sg.v - sg.u;
        if (n > most) most = n, bs = jobs[2 * c.r + c.a];
      }
      if (bs)
        for (const Segment& sg : *bs) {
          const int64_t len = sg.v - sg.u, np = (len + cap - 1) / cap;
          for (int64_t k = 0; k < np; ++k) pace.push_back(len / np + (k < len % np ? 1 : 0));
        }
    }
    int64_t nr = 0;
    for (;;) {
      const size_t b0 = out.pieces.size(), t0 = out.targets.size();
      int64_t rn = 0;
      const int64_t pk = (size_t)nr < pace.size() ? pace[(size_t)nr] : cap;
      for (Cursor& c : bc) {
        const std::vector<Segment>& segs = *jobs[2 * c.r + c.a];
        if (c.s >= segs.size()) continue;
        const Segment& sg = segs[c.s];
        if (c.pos == sg.u) {
          out.targets.push_back({c.r, c.a, c.s});
          rn = sg.v - sg.u > rn ? sg.v - sg.u : rn;
        }
        const int64_t end = pk > 0 && c.pos + pk < sg.v ? c.pos + pk : sg.v;
        out.pieces.push_back({c.r, c.a, c.pos, end, sg.sync && end == sg.v});
        c.pos = end;
        if (end == sg.v && ++c.s < segs.size()) c.pos = segs[c.s].u;
      }
      if (out.pieces.size() == b0) break;
      out.rounds.push_back({p, b0, out.pieces.size(), t0, out.targets.size(), rn});
      ++nr;
    }
    out.max_rounds = nr > out.max_rounds ? nr : out.max_rounds;
  }
}

// The persistent BR kernel's tables (learner.hip k_br_persist): every segment in job order, its
// first chunk counter, each job's segment range, and the work queue holding the first segments'
// items -- segment << 16 | update in it -- chunk by chunk across the jobs; the chains queue the
// later segments' items themselves, so the rest of the queue starts empty.
constexpr uint32_t SLOT_EMPTY = 0xFFFFFFFFu;
struct PersistPlan {
  std::vector<SegRef> segs;      // [nseg] job order
  std::vector<int32_t> chunk0;   // [nseg] the running sum of ceil(n / chunk)
  std::vector<int32_t> jseg0;    // [njobs + 1] job j's segments: [jseg0[j], jseg0[j + 1])
  std::vector<uint32_t> slots;   // [nitems]
  uint32_t npre = 0;             // queued items
  int32_t nchunks = 0;
};
// 0, or -1 and the limit that was exceeded in *msg (the item encoding's 16 + 16 bits)
inline int plan_persist(const Jobs& jobs, int R, int chunk, PersistPlan& out, const char** msg) {
  out = PersistPlan{};
  std::vector<int64_t> len;      // [nseg]
  for (int r = 0; r < R; ++r)
    for (int a = 0; a < 2; ++a) {
      if (!jobs[2 * r + a] || jobs[2 * r + a]->empty()) continue;
      const std::vector<Segment>& segs = *jobs[2 * r + a];
      out.jseg0.push_back((int32_t)out.segs.size());
      for (size_t s = 0; s < segs.size(); ++s) {
        const int64_t n = segs[s].v - segs[s].u;
        if (n >= 65536) {
          *msg = "a BR segment of >= 65536 updates";
          return -1;
        }
        out.segs.push_back({r, a, s});
        len.push_back(n);
        out.chunk0.push_back(out.nchunks);
        out.nchunks += (int32_t)((n + chunk - 1) / chunk);
      }
    }
  if (out.segs.size() >= 65536) {
    *msg = "too many BR segments in one learner call";
    return -1;
  }
  const int njobs = (int)out.jseg0.size();
  out.jseg0.push_back((int32_t)out.segs.size());
  int64_t nitems = 0, maxn = 0;
  for (int64_t n : len) nitems += n;
  for (int j = 0; j < njobs; ++j) maxn = len[out.jseg0[j]] > maxn ? len[out.jseg0[j]] : maxn;
  out.slots.assign((size_t)nitems, SLOT_EMPTY);
  for (int64_t c0 = 0; c0 < maxn; c0 += chunk)
    for (int j = 0; j < njobs; ++j) {
      const int sgi = out.jseg0[j];
      const int64_t n = len[sgi], c1 = c0 + chunk < n ? c0 + chunk : n;
      for (int64_t i = c0; i < c1; ++i) out.slots[out.npre++] = ((uint32_t)sgi << 16) | (uint32_t)i;
    }
  return 0;
}

}  // namespace plan
}  // namespace nfsp
