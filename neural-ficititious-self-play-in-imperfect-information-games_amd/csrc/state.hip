// Checkpoint and bit-exact resume of an engine or an engine group (include/nfsp.h
// nfsp_*_state_*; the format, with byte offsets: DESIGN.md §10, csrc/state_blob.h).
//
// A blob holds what the next step's results depend on, and nothing else:
//   HOST   cfg and game, hands per lane g = rollouts / slices, learn_tag, the schedule mirror hs
//   ST     EngineDev, raw, with `rollouts` holding g (rollouts itself counts slices)
//   NETS   the six nets [2][3][NP]
//   RL     each agent's live M_RL records, oldest first (unwrapped from the circular log, so
//          the bytes do not depend on log_cap and therefore not on the slicing)
//   SL     each agent's M_SL rows [0, sl_size)
// (a group: R, flags, calls, w0_valid and w0, then its replicas' payloads).  In the payload
// cfg.slices, cfg.slice_lag and cfg.sched are 1, 1, 0; the saving engine's are in the header,
// outside the digest, so one training state has one payload whatever its slicing.
//
// NOT stored -- session settings, or rebuilt before they are read: the rollout staging and the
// pending M_SL list (empty at a step boundary), the learner buffers, res_head / res_next /
// res_slot, the slice_lag 2 snapshots (rebuilt at each step's start), the fp32 export views and
// the debug views, timing, the loss log, the update limit, a group's schedule and trace, and the
// exchange transport with its cadence (at a boundary W0 == W_AR: the caller re-issues
// nfsp_engine_set_exchange / nfsp_group_set_exchange after the load).
//
// res_head entries carry the learn_tag of the call that wrote them.  A load restores learn_tag
// exactly and CLEARS res_head, so an entry an engine wrote before the load can never match a
// restored tag (tags start at 1; a cleared entry has tag 0).
//
// k_state_digest reads the restored state where it lies, through a table of at most 12
// segments: a load proves that every byte landed without reading any of it back.
//
// Which records are live and where they lie is mem_view.h's: the entry points open with
// engine_view / group_view (at rest, with the view of the memories), and the digest, the writer,
// the loader and the size checks walk its segments.  Only the C ABI is called from other files.
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "mem_view.h"
#include "state_blob.h"

namespace nn = nfsp::nn;
using namespace nfsp::eng;
using namespace nfsp::blob;

namespace {

// ---------------------------------------------------------------------------
// the digest kernel
// ---------------------------------------------------------------------------
constexpr int DIGEST_WG = 256;
constexpr int DIGEST_MAX_SEG = 12;
constexpr int DIGEST_MAX_BLOCKS = 2048;       // 8 workgroups per CU of an MI355X

struct DigestSeg {
  const uint64_t* p;   // device, 8-byte aligned
  uint64_t words;
  uint64_t first;      // payload index of p[0]
};
struct DigestTable {
  int n;
  DigestSeg seg[DIGEST_MAX_SEG];
};

// the workgroup's sums -> lane 0 of wave 0
__device__ inline void wg_reduce(uint64_t& d0, uint64_t& d1, uint64_t (*lds)[2]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d0 += __shfl_down(d0, off, 64);
    d1 += __shfl_down(d1, off, 64);
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds[wave][0] = d0;
    lds[wave][1] = d1;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < DIGEST_WG / 64; ++k) {
      d0 += lds[k][0];
      d1 += lds[k][1];
    }
}

// Grid-stride over every segment: 16-byte loads over the 16-byte aligned body, the (at most
// one) word before it and the (at most one) word after it by thread 0 of the grid.  One partial
// {D0, D1} per workgroup, written with plain stores; k_state_digest_sum adds them up.
__global__ void __launch_bounds__(DIGEST_WG) k_state_digest(DigestTable T, uint64_t* __restrict__ partial) {
  __shared__ uint64_t lds[DIGEST_WG / 64][2];
  const uint64_t tid = (uint64_t)blockIdx.x * DIGEST_WG + threadIdx.x;
  const uint64_t nt = (uint64_t)gridDim.x * DIGEST_WG;
  uint64_t d0 = 0, d1 = 0;
  for (int s = 0; s < T.n; ++s) {
    const uint64_t* p = T.seg[s].p;
    const uint64_t n = T.seg[s].words, first = T.seg[s].first;
    if (n == 0) continue;
    const uint64_t head = ((uintptr_t)p & 8u) ? 1 : 0;
    const uint64_t pairs = (n - head) >> 1;
    const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p + head);
    // (four loads in flight per lane, by hand, measured slower at C3 size: 18.3 against 16.7 us)
    for (uint64_t k = tid; k < pairs; k += nt) {
      const ulonglong2 v = q[k];
      const uint64_t i = first + head + 2 * k;
      digest_add(d0, d1, v.x, i);
      digest_add(d0, d1, v.y, i + 1);
    }
    if (tid == 0) {
      if (head) digest_add(d0, d1, p[0], first);
      if ((n - head) & 1) digest_add(d0, d1, p[n - 1], first + n - 1);
    }
  }
  wg_reduce(d0, d1, lds);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x + 0] = d0;
    partial[2 * blockIdx.x + 1] = d1;
  }
}

__global__ void __launch_bounds__(DIGEST_WG) k_state_digest_sum(const uint64_t* __restrict__ partial, int n,
                                                                uint64_t* __restrict__ out) {
  __shared__ uint64_t lds[DIGEST_WG / 64][2];
  uint64_t d0 = 0, d1 = 0;
  for (int k = threadIdx.x; k < n; k += DIGEST_WG) {
    d0 += partial[2 * k + 0];
    d1 += partial[2 * k + 1];
  }
  wg_reduce(d0, d1, lds);
  if (threadIdx.x == 0) {
    out[0] = d0;
    out[1] = d1;
  }
}

// out[2] += the digest of the table's segments; launches on the ctx stream and synchronises it.
// The partials live in a buffer of the engine's (allocated on first use).
int digest_run(nfsp_engine* e, const DigestTable& T, uint64_t out[2], float* ms = nullptr) {
  uint64_t words = 0;
  for (int s = 0; s < T.n; ++s) words += T.seg[s].words;
  if (words == 0) return NFSP_OK;
  if (!e->digest_buf) {
    NFSP_HIP(hipMalloc((void**)&e->digest_buf, sizeof(uint64_t) * 2 * (DIGEST_MAX_BLOCKS + 1)));
    e->allocs.push_back(e->digest_buf);
  }
  // 4 x 16 bytes per lane before the grid stops growing
  int64_t blocks = (int64_t)((words / 2 + 4 * DIGEST_WG - 1) / (4 * DIGEST_WG));
  blocks = blocks < 1 ? 1 : blocks > DIGEST_MAX_BLOCKS ? DIGEST_MAX_BLOCKS : blocks;
  hipStream_t s = e->ctx->stream;
  uint64_t* res = e->digest_buf + 2 * DIGEST_MAX_BLOCKS;
  hipEvent_t t0 = nullptr, t1 = nullptr;
  if (ms) {
    t0 = take_event(e);
    t1 = take_event(e);
    NFSP_HIP(hipEventRecord(t0, s));
  }
  k_state_digest<<<(unsigned)blocks, DIGEST_WG, 0, s>>>(T, e->digest_buf);
  NFSP_LAUNCHED("k_state_digest");
  k_state_digest_sum<<<1, DIGEST_WG, 0, s>>>(e->digest_buf, (int)blocks, res);
  NFSP_LAUNCHED("k_state_digest_sum");
  if (ms) NFSP_HIP(hipEventRecord(t1, s));
  uint64_t h[2];
  NFSP_HIP(hipMemcpyAsync(h, res, sizeof(h), hipMemcpyDeviceToHost, s));
  NFSP_HIP(hipStreamSynchronize(s));
  if (ms) {
    NFSP_HIP(hipEventElapsedTime(ms, t0, t1));
    e->pool.push_back(t0);
    e->pool.push_back(t1);
  }
  out[0] += h[0];
  out[1] += h[1];
  return NFSP_OK;
}

// ---------------------------------------------------------------------------
// the payload's host records
// ---------------------------------------------------------------------------
struct HostRec {               // section HOST, 192 bytes (padding bytes are zero)
  nfsp_engine_cfg cfg;         //   0  slices = slice_lag = 1, sched = 0
  int32_t game;                // 104
  int32_t pad0;                // 108
  int64_t g;                   // 112  hands per lane so far
  uint32_t learn_tag;          // 120
  uint32_t pad1;               // 124
  int64_t iteration[2];        // 128  hs
  int64_t target_count[2];     // 144
  int64_t target_syncs[2];     // 160
  double epsilon[2];           // 176
};
static_assert(sizeof(nfsp_engine_cfg) == 104 && sizeof(HostRec) == 192, "HostRec layout");
static_assert(offsetof(HostRec, g) == 112 && offsetof(HostRec, iteration) == 128, "HostRec layout");
static_assert(sizeof(EngineDev) == 296 && offsetof(EngineDev, rollouts) == 168, "EngineDev layout");
static_assert(sizeof(RlRec) == 32 && sizeof(SlRec) == 16, "record layout");

struct GroupRec {              // head of section GROUP, 24 bytes; w0 [3][2][NP] f32 follows
  int32_t R;                   //   0
  uint32_t flags;              //   4
  int64_t calls;               //   8
  uint32_t w0_valid;           //  16
  uint32_t pad;                //  20
};
static_assert(sizeof(GroupRec) == 24, "GroupRec layout");

constexpr uint64_t NETS_BYTES = sizeof(float) * 6 * nn::NP;
constexpr uint64_t GROUP_BYTES = sizeof(GroupRec) + sizeof(float) * 6 * nn::NP;
static_assert(NETS_BYTES % 8 == 0 && GROUP_BYTES % 8 == 0, "sections are whole words");
constexpr uint64_t ST_ROLLOUTS_WORD = offsetof(EngineDev, rollouts) / 8;

inline uint64_t header_bytes(uint32_t n_sections) { return sizeof(BlobHeader) + sizeof(BlobSection) * (uint64_t)n_sections; }

HostRec host_rec(const nfsp_engine* e) {
  HostRec r;
  memset(&r, 0, sizeof(r));
  // field by field (engine_cfg.h's table), bytes into bytes: the struct's padding stays zero
  const nfsp_engine_cfg c = cfg_stored(e->cfg);
  memcpy(&r.cfg, &c, sizeof(c));
  r.game = e->ctx->game;
  r.g = (int64_t)(e->rollouts / (uint64_t)e->slices);
  r.learn_tag = e->learn_tag;
  for (int a = 0; a < 2; ++a) {
    r.iteration[a] = e->hs.iteration[a];
    r.target_count[a] = e->hs.target_count[a];
    r.target_syncs[a] = e->hs.target_syncs[a];
    r.epsilon[a] = e->hs.epsilon[a];
  }
  return r;
}

// ---------------------------------------------------------------------------
// parsing (host only)
// ---------------------------------------------------------------------------
struct BlobView {
  BlobHeader h;
  std::vector<BlobSection> sec;
  const unsigned char* base = nullptr;
  const unsigned char* at(int k) const { return base + sec[k].offset; }
  // the first section of replica r's engine payload
  int engine_sec(int r) const { return (h.kind == KIND_GROUP ? 1 : 0) + ENGINE_SECTIONS * r; }
};

int bad(const std::string& msg) { return nfsp::fail(NFSP_EINVAL, "state blob: " + msg); }

// header, sizes, section bounds and the digest; then each engine payload's own consistency
int blob_parse(const void* buf, int64_t n, BlobView* v) {
  if (!buf || !v) return nfsp::fail(NFSP_EINVAL, "null argument");
  if (n < (int64_t)sizeof(BlobHeader)) return bad("truncated: shorter than its header");
  memcpy(&v->h, buf, sizeof(BlobHeader));
  const BlobHeader& h = v->h;
  if (memcmp(h.magic, MAGIC, sizeof(MAGIC)) != 0) return bad("wrong magic (not a libnfsp state blob)");
  if (h.version != VERSION) return bad("format version " + std::to_string(h.version) + ", this library reads " + std::to_string(VERSION));
  if (h.sz_cfg != sizeof(nfsp_engine_cfg) || h.sz_dev != sizeof(EngineDev) || h.sz_rl != sizeof(RlRec) ||
      h.sz_sl != sizeof(SlRec) || h.sz_host != sizeof(HostRec) || h.np != (uint32_t)nn::NP)
    return bad("struct sizes differ from this library's");
  if (h.kind != KIND_ENGINE && h.kind != KIND_GROUP) return bad("unknown kind");
  if (h.replicas < 1 || h.replicas > NFSP_GROUP_MAX_REPLICAS || (h.kind == KIND_ENGINE && h.replicas != 1))
    return bad("bad replica count");
  const uint32_t want = (h.kind == KIND_GROUP ? 1u : 0u) + ENGINE_SECTIONS * h.replicas;
  if (h.n_sections != want) return bad("bad section count");
  if (h.slices < 1 || (h.slice_lag != 1 && h.slice_lag != 2) || h.reserved != 0) return bad("bad slicing fields");
  const uint64_t hb = header_bytes(h.n_sections);
  if (h.payload_offset != hb || h.total_bytes < hb || h.payload_bytes != h.total_bytes - hb)
    return bad("inconsistent header sizes");
  if ((uint64_t)n < h.total_bytes)
    return bad("truncated: " + std::to_string(n) + " bytes of " + std::to_string(h.total_bytes));
  v->base = static_cast<const unsigned char*>(buf);
  v->sec.resize(h.n_sections);
  memcpy(v->sec.data(), v->base + sizeof(BlobHeader), sizeof(BlobSection) * h.n_sections);
  static const uint32_t order[ENGINE_SECTIONS] = {SEC_HOST, SEC_ST, SEC_NETS, SEC_RL, SEC_SL};
  uint64_t at = hb;
  for (uint32_t k = 0; k < h.n_sections; ++k) {
    const BlobSection& s = v->sec[k];
    const bool grp = h.kind == KIND_GROUP && k == 0;
    const uint32_t q = k - (h.kind == KIND_GROUP ? 1u : 0u);
    const uint32_t kind = grp ? (uint32_t)SEC_GROUP : order[q % ENGINE_SECTIONS];
    const uint32_t rep = grp ? 0u : q / ENGINE_SECTIONS;
    if (s.kind != kind || s.replica != rep) return bad("section " + std::to_string(k) + ": unexpected kind or replica");
    if (s.offset > h.total_bytes || s.bytes > h.total_bytes - s.offset)
      return bad("section " + std::to_string(k) + " points past the end");
    if (s.offset != at || s.bytes % 8 != 0) return bad("section " + std::to_string(k) + ": not contiguous or not whole words");
    const uint64_t fixed = kind == SEC_HOST ? sizeof(HostRec) : kind == SEC_ST ? sizeof(EngineDev)
                           : kind == SEC_NETS ? NETS_BYTES : kind == SEC_GROUP ? GROUP_BYTES : s.bytes;
    if (s.bytes != fixed) return bad("section " + std::to_string(k) + ": wrong size");
    at += s.bytes;
  }
  if (at != h.total_bytes) return bad("sections do not fill the payload");
  uint64_t d[2] = {0, 0};
  digest_words(d, v->base + hb, h.payload_bytes / 8, 0);
  if (d[0] != h.digest[0] || d[1] != h.digest[1]) return bad("digest mismatch (corrupted payload)");
  // each engine payload against itself
  for (uint32_t r = 0; r < h.replicas; ++r) {
    const int k0 = v->engine_sec((int)r);
    HostRec hr;
    EngineDev st;
    memcpy(&hr, v->at(k0 + 0), sizeof(hr));
    memcpy(&st, v->at(k0 + 1), sizeof(st));
    const nfsp_engine_cfg& c = hr.cfg;
    if (c.n_lanes < 1 || c.rl_capacity < 1 || c.sl_capacity < 1 || c.slices != 1 || c.slice_lag != 1 || c.sched != 0)
      return bad("bad cfg in the payload");
    int rc = st_check(st, c, "state blob");
    if (rc != NFSP_OK) return rc;
    if (hr.g < 0 || st.rollouts != hr.g) return bad("hand counters disagree");
    const MemTotals m = mem_totals(st, c.rl_capacity);
    if (v->sec[k0 + 3].bytes != (uint64_t)m.rl * sizeof(RlRec) || v->sec[k0 + 4].bytes != (uint64_t)m.sl * sizeof(SlRec))
      return bad("memory sections do not match the counters");
  }
  if (h.kind == KIND_GROUP) {
    GroupRec gr;
    memcpy(&gr, v->at(0), sizeof(gr));
    if (gr.R != (int32_t)h.replicas || gr.calls < 0 || (gr.w0_valid & ~(NFSP_XCHG_AR | NFSP_XCHG_BR)) || gr.pad != 0)
      return bad("bad group record");
  }
  return NFSP_OK;
}

void fill_info(const BlobView& v, nfsp_state_info* info) {
  memset(info, 0, sizeof(*info));
  info->version = (int32_t)v.h.version;
  info->kind = (int32_t)v.h.kind;
  info->replicas = (int32_t)v.h.replicas;
  info->n_sections = (int32_t)v.h.n_sections;
  info->slices = v.h.slices;
  info->slice_lag = v.h.slice_lag;
  info->sched = v.h.sched;
  if (v.h.kind == KIND_GROUP) {
    GroupRec gr;
    memcpy(&gr, v.at(0), sizeof(gr));
    info->group_flags = gr.flags;
  }
  info->total_bytes = (int64_t)v.h.total_bytes;
  info->payload_offset = (int64_t)v.h.payload_offset;
  info->payload_bytes = (int64_t)v.h.payload_bytes;
  info->digest[0] = v.h.digest[0];
  info->digest[1] = v.h.digest[1];
}

// ---------------------------------------------------------------------------
// engine <-> payload
// ---------------------------------------------------------------------------
uint64_t engine_payload_bytes(const MemView& v) {
  return sizeof(HostRec) + sizeof(EngineDev) + NETS_BYTES + v.total.bytes();
}
uint64_t group_bytes(const std::vector<MemView>& v) {
  uint64_t total = header_bytes(1 + ENGINE_SECTIONS * (uint32_t)v.size()) + GROUP_BYTES;
  for (const MemView& m : v) total += engine_payload_bytes(m);
  return total;
}

// Digest of the engine's payload as it would be saved now, its first word at payload index
// `base`: the HOST section (and the canonical `rollouts` word of ST) on the host, everything
// else by the kernel, in place, along the view's segments.  Adds into out.
int engine_digest(nfsp_engine* e, const MemView& v, uint64_t base, uint64_t out[2], float* ms = nullptr,
                  uint64_t* bytes = nullptr) {
  const HostRec hr = host_rec(e);
  digest_words(out, &hr, sizeof(hr) / 8, base);
  DigestTable T{};
  uint64_t at = base + sizeof(hr) / 8;
  auto add = [&](const void* p, uint64_t words) {
    T.seg[T.n++] = DigestSeg{static_cast<const uint64_t*>(p), words, at};
    at += words;
  };
  const uint64_t st_first = at;
  add(e->st, sizeof(EngineDev) / 8);
  add(e->w, NETS_BYTES / 8);
  for (const AgentView& A : v.agent)
    for (int k = 0; k < A.n_rl; ++k) add(A.rl[k], (uint64_t)A.rl_n[k] * (sizeof(RlRec) / 8));
  for (const AgentView& A : v.agent) add(A.sl, (uint64_t)A.sl_n * (sizeof(SlRec) / 8));
  static_assert(2 + 4 + 2 <= DIGEST_MAX_SEG, "segment table");
  if (bytes) *bytes = (at - base) * 8;
  int rc = digest_run(e, T, out, ms);
  if (rc != NFSP_OK) return rc;
  // ST.rollouts counts slices on the device and hands per lane in the payload
  uint64_t dev[2] = {0, 0}, canon[2] = {0, 0};
  digest_add(dev[0], dev[1], (uint64_t)v.st.rollouts, st_first + ST_ROLLOUTS_WORD);
  digest_add(canon[0], canon[1], (uint64_t)hr.g, st_first + ST_ROLLOUTS_WORD);
  out[0] += canon[0] - dev[0];
  out[1] += canon[1] - dev[1];
  return NFSP_OK;
}

// The blob's two memory sections along the view's segments, saved from them or (load: the
// sections are only read) loaded into them: RL, each agent's records oldest first, then SL.
int copy_memories(const MemView& v, unsigned char* rl, unsigned char* sl, bool load) {
  auto copy = [load](unsigned char*& host, void* dev, size_t nb) {
    if (nb) NFSP_HIP(load ? hipMemcpy(dev, host, nb, hipMemcpyHostToDevice) : hipMemcpy(host, dev, nb, hipMemcpyDeviceToHost));
    host += nb;
    return (int)NFSP_OK;
  };
  int rc = NFSP_OK;
  for (const AgentView& A : v.agent)
    for (int k = 0; k < A.n_rl; ++k)
      if ((rc = copy(rl, A.rl[k], (size_t)A.rl_n[k] * sizeof(RlRec))) != NFSP_OK) return rc;
  for (const AgentView& A : v.agent)
    if ((rc = copy(sl, A.sl, (size_t)A.sl_n * sizeof(SlRec))) != NFSP_OK) return rc;
  return NFSP_OK;
}

// the engine's five sections at `at` of the blob (the engine at rest, v = its view)
int engine_write(nfsp_engine* e, const MemView& v, unsigned char* buf, uint64_t* at, BlobSection* sec, uint32_t rep) {
  auto begin = [&](int k, uint32_t kind, uint64_t bytes) {
    sec[k] = BlobSection{kind, rep, *at, bytes};
    unsigned char* p = buf + *at;
    *at += bytes;
    return p;
  };
  const HostRec hr = host_rec(e);
  memcpy(begin(0, SEC_HOST, sizeof(hr)), &hr, sizeof(hr));
  EngineDev st = v.st;
  st.rollouts = hr.g;
  memcpy(begin(1, SEC_ST, sizeof(st)), &st, sizeof(st));
  NFSP_HIP(hipMemcpy(begin(2, SEC_NETS, NETS_BYTES), e->w, NETS_BYTES, hipMemcpyDeviceToHost));
  unsigned char* rl = begin(3, SEC_RL, (uint64_t)v.total.rl * sizeof(RlRec));
  unsigned char* sl = begin(4, SEC_SL, (uint64_t)v.total.sl * sizeof(SlRec));
  return copy_memories(v, rl, sl, false);
}

void header_init(BlobHeader* h, uint32_t kind, uint32_t replicas, const nfsp_engine* e0) {
  memset(h, 0, sizeof(*h));
  memcpy(h->magic, MAGIC, sizeof(MAGIC));
  h->version = VERSION;
  h->kind = kind;
  h->sz_cfg = sizeof(nfsp_engine_cfg);
  h->sz_dev = sizeof(EngineDev);
  h->sz_rl = sizeof(RlRec);
  h->sz_sl = sizeof(SlRec);
  h->sz_host = sizeof(HostRec);
  h->np = nn::NP;
  h->replicas = replicas;
  h->n_sections = (kind == KIND_GROUP ? 1u : 0u) + ENGINE_SECTIONS * replicas;
  h->slices = e0->cfg.slices;
  h->slice_lag = e0->cfg.slice_lag;
  h->sched = e0->cfg.sched;
  h->payload_offset = header_bytes(h->n_sections);
}

// header (with the payload's digest) and section table into the finished blob
void header_finish(BlobHeader* h, const std::vector<BlobSection>& sec, unsigned char* buf, uint64_t total) {
  h->total_bytes = total;
  h->payload_bytes = total - h->payload_offset;
  h->digest[0] = h->digest[1] = 0;
  digest_words(h->digest, buf + h->payload_offset, h->payload_bytes / 8, 0);
  memcpy(buf, h, sizeof(*h));
  memcpy(buf + sizeof(*h), sec.data(), sizeof(BlobSection) * sec.size());
}

// what a blob's engine payload must share with the engine it is loaded into (replica >= 0: a
// group's replica, named in the message -- its replicas' cfgs may differ from each other)
int compat_check(const nfsp_engine* e, const HostRec& hr, int replica = -1) {
  const char* f = cfg_first_diff(e->cfg, hr.cfg, CFG_SHAPE | CFG_HYPER);   // every stored field
  if (!f && e->ctx->game != hr.game) f = "game";
  if (f && replica >= 0)
    return nfsp::fail(NFSP_EINVAL, std::string("state blob: replica ") + std::to_string(replica) + ": " + f +
                                       " differs from the group's replica " + std::to_string(replica));
  if (f) return nfsp::fail(NFSP_EINVAL, std::string("state blob: ") + f + " differs from the engine's");
  return NFSP_OK;
}

// Replica payload k0.. of the blob into the engine (validated, compatible, streams idle).  The
// target's own slicing: rollouts = g * slices, and the blob's counters viewed in the target's
// memories, so record k lands at row k % log_cap.
int engine_restore(nfsp_engine* e, const BlobView& v, int k0) {
  HostRec hr;
  EngineDev st;
  memcpy(&hr, v.at(k0 + 0), sizeof(hr));
  memcpy(&st, v.at(k0 + 1), sizeof(st));
  hipStream_t s = e->ctx->stream;
  const uint64_t rollouts = (uint64_t)hr.g * (uint64_t)e->slices;
  EngineDev dev = st;
  dev.rollouts = (int64_t)rollouts;
  // synchronous copies from the caller's (pageable) buffer; nothing else runs on the engine
  NFSP_HIP(hipMemcpy(e->st, &dev, sizeof(dev), hipMemcpyHostToDevice));
  NFSP_HIP(hipMemcpy(e->w, v.at(k0 + 2), NETS_BYTES, hipMemcpyHostToDevice));
  int rc = copy_memories(mem_view(e, st), const_cast<unsigned char*>(v.at(k0 + 3)), const_cast<unsigned char*>(v.at(k0 + 4)), true);
  if (rc != NFSP_OK) return rc;
  // no res_head entry of an earlier life may match a restored learn_tag
  NFSP_HIP(hipMemsetAsync(e->LBs[0].res_head, 0, sizeof(unsigned long long) * 2 * (size_t)e->M.sl_cap, s));
  if (e->xchg_w0)                       // W0 = the restored AR nets (nfsp_engine_set_exchange's rule)
    for (int a = 0; a < 2; ++a)
      NFSP_HIP(hipMemcpyAsync(e->xchg_w0 + a * nn::NP, e->w + (a * 3) * nn::NP, sizeof(float) * nn::NP,
                              hipMemcpyDeviceToDevice, s));
  NFSP_HIP(hipStreamSynchronize(s));
  e->rollouts = rollouts;
  e->learn_tag = hr.learn_tag;
  e->pending_update = false;
  e->xchg_calls = 0;
  for (int a = 0; a < 2; ++a) {
    e->hs.iteration[a] = hr.iteration[a];
    e->hs.target_count[a] = hr.target_count[a];
    e->hs.target_syncs[a] = hr.target_syncs[a];
    e->hs.epsilon[a] = hr.epsilon[a];
    e->last_U[a] = e->last_Ubr[a] = 0;
  }
  return NFSP_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int nfsp_state_check(const void* buf, int64_t n, nfsp_state_info* info) {
  BlobView v;
  int rc = blob_parse(buf, n, &v);
  if (rc != NFSP_OK) return rc;
  if (info) fill_info(v, info);
  return NFSP_OK;
}

extern "C" int nfsp_state_cfg(const void* buf, int64_t n, int replica, nfsp_engine_cfg* cfg, int32_t* game) {
  BlobView v;
  int rc = blob_parse(buf, n, &v);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(replica >= 0 && replica < (int)v.h.replicas, "no such replica in the state blob");
  HostRec hr;
  memcpy(&hr, v.at(v.engine_sec(replica)), sizeof(hr));
  if (cfg) {
    *cfg = hr.cfg;
    cfg->slices = v.h.slices;
    cfg->slice_lag = v.h.slice_lag;
    cfg->sched = v.h.sched;
  }
  if (game) *game = hr.game;
  return NFSP_OK;
}

extern "C" int nfsp_state_digest(const void* payload, int64_t n, uint64_t out[2]) {
  NFSP_REQUIRE(out && n >= 0 && n % 8 == 0 && (payload || n == 0), "the payload must be whole 8-byte words");
  out[0] = out[1] = 0;
  digest_words(out, payload, (uint64_t)n / 8, 0);
  return NFSP_OK;
}

extern "C" int nfsp_engine_state_digest(nfsp_engine* e, uint64_t out[2]) {
  NFSP_REQUIRE(e && out, "null argument");
  MemView v;
  int rc = engine_view(e, "nfsp_engine_state_digest", &v);
  if (rc != NFSP_OK) return rc;
  out[0] = out[1] = 0;
  return engine_digest(e, v, 0, out);
}

extern "C" int nfsp_engine_state_digest_timed(nfsp_engine* e, uint64_t out[2], double* ms, int64_t* bytes) {
  NFSP_REQUIRE(e && out && ms && bytes, "null argument");
  MemView v;
  int rc = engine_view(e, "nfsp_engine_state_digest_timed", &v);
  if (rc != NFSP_OK) return rc;
  out[0] = out[1] = 0;
  float t = 0.f;
  uint64_t nb = 0;
  if ((rc = engine_digest(e, v, 0, out, &t, &nb)) != NFSP_OK) return rc;
  *ms = t;
  *bytes = (int64_t)(nb - sizeof(HostRec));     // what the kernel read
  return NFSP_OK;
}

extern "C" int nfsp_engine_state_bytes(nfsp_engine* e, int64_t* out) {
  NFSP_REQUIRE(e && out, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is saved by nfsp_group_save_state");
  MemView v;
  int rc = engine_view(e, "nfsp_engine_state_bytes", &v);
  if (rc != NFSP_OK) return rc;
  *out = (int64_t)(header_bytes(ENGINE_SECTIONS) + engine_payload_bytes(v));
  return NFSP_OK;
}

extern "C" int nfsp_engine_save_state(nfsp_engine* e, void* host_buf, int64_t cap, int64_t* written) {
  NFSP_REQUIRE(e && host_buf && written, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is saved by nfsp_group_save_state");
  MemView v;
  int rc = engine_view(e, "nfsp_engine_save_state", &v);
  if (rc != NFSP_OK) return rc;
  BlobHeader hd;
  header_init(&hd, KIND_ENGINE, 1, e);
  const uint64_t total = hd.payload_offset + engine_payload_bytes(v);
  NFSP_REQUIRE(cap >= 0 && (uint64_t)cap >= total, "nfsp_engine_save_state: the buffer is smaller than nfsp_engine_state_bytes");
  unsigned char* buf = static_cast<unsigned char*>(host_buf);
  std::vector<BlobSection> sec(hd.n_sections);
  uint64_t at = hd.payload_offset;
  if ((rc = engine_write(e, v, buf, &at, sec.data(), 0)) != NFSP_OK) return rc;
  header_finish(&hd, sec, buf, at);
  *written = (int64_t)at;
  return NFSP_OK;
}

extern "C" int nfsp_engine_load_state(nfsp_engine* e, const void* host_buf, int64_t n) {
  NFSP_REQUIRE(e && host_buf, "null argument");
  NFSP_REQUIRE(standalone(e), "a replica of an engine group is loaded by nfsp_group_load_state");
  // everything that can refuse the blob comes before the first write (and before any device work)
  BlobView v;
  int rc = blob_parse(host_buf, n, &v);
  if (rc != NFSP_OK) return rc;
  NFSP_REQUIRE(v.h.kind == KIND_ENGINE, "state blob: a group's (nfsp_group_load_state)");
  HostRec hr;
  memcpy(&hr, v.at(0), sizeof(hr));
  if ((rc = compat_check(e, hr)) != NFSP_OK) return rc;
  if ((rc = engine_rest(e, "nfsp_engine_load_state", true)) != NFSP_OK) return rc;
  if ((rc = engine_restore(e, v, 0)) != NFSP_OK) return rc;
  // the device now holds the blob's payload: prove it in place
  MemView mv;
  if ((rc = engine_view(e, "nfsp_engine_load_state", &mv)) != NFSP_OK) return rc;
  uint64_t d[2] = {0, 0};
  if ((rc = engine_digest(e, mv, 0, d)) != NFSP_OK) return rc;
  if (d[0] != v.h.digest[0] || d[1] != v.h.digest[1])
    return nfsp::fail(NFSP_EHIP, "nfsp_engine_load_state: the device state's digest differs from the blob's after the copy");
  return NFSP_OK;
}

// ---- groups
extern "C" int nfsp_group_state_bytes(nfsp_group* g, int64_t* out) {
  NFSP_REQUIRE(g && out, "null argument");
  GroupState G;
  std::vector<MemView> v;
  int rc = group_view(g, "nfsp_group_state_bytes", &G, &v);
  if (rc != NFSP_OK) return rc;
  *out = (int64_t)group_bytes(v);
  return NFSP_OK;
}

extern "C" int nfsp_group_save_state(nfsp_group* g, void* host_buf, int64_t cap, int64_t* written) {
  NFSP_REQUIRE(g && host_buf && written, "null argument");
  GroupState G;
  std::vector<MemView> v;
  int rc = group_view(g, "nfsp_group_save_state", &G, &v);
  if (rc != NFSP_OK) return rc;
  const uint64_t total = group_bytes(v);
  NFSP_REQUIRE(cap >= 0 && (uint64_t)cap >= total, "nfsp_group_save_state: the buffer is smaller than nfsp_group_state_bytes");
  unsigned char* buf = static_cast<unsigned char*>(host_buf);
  BlobHeader hd;
  header_init(&hd, KIND_GROUP, (uint32_t)G.R, G.eng[0]);
  std::vector<BlobSection> sec(hd.n_sections);
  uint64_t at = hd.payload_offset;
  sec[0] = BlobSection{SEC_GROUP, 0, at, GROUP_BYTES};
  GroupRec gr{};
  gr.R = G.R;
  gr.flags = G.flags;
  gr.calls = *G.calls;
  gr.w0_valid = *G.w0_valid;
  memcpy(buf + at, &gr, sizeof(gr));
  float* w0 = reinterpret_cast<float*>(buf + at + sizeof(gr));
  NFSP_HIP(hipMemcpy(w0, G.w0, sizeof(float) * 6 * nn::NP, hipMemcpyDeviceToHost));
  // w0 is [net][agent][NP]; a net that was never exchanged has no W0 yet: zeros, not whatever
  // the allocation held.  The target net's W0 is never read (it rides with the BR net's flag).
  for (int net = 0; net < 3; ++net) {
    const unsigned bit = net == 0 ? NFSP_XCHG_AR : NFSP_XCHG_BR;
    if (!(gr.w0_valid & bit)) memset(w0 + (size_t)net * 2 * nn::NP, 0, sizeof(float) * 2 * nn::NP);
  }
  at += GROUP_BYTES;
  for (int r = 0; r < G.R; ++r)
    if ((rc = engine_write(G.eng[r], v[r], buf, &at, sec.data() + 1 + ENGINE_SECTIONS * r, (uint32_t)r)) != NFSP_OK)
      return rc;
  header_finish(&hd, sec, buf, at);
  *written = (int64_t)at;
  return NFSP_OK;
}

extern "C" int nfsp_group_load_state(nfsp_group* g, const void* host_buf, int64_t n) {
  NFSP_REQUIRE(g && host_buf, "null argument");
  GroupState G;
  int rc = group_state(g, &G);
  if (rc != NFSP_OK) return rc;
  BlobView v;
  if ((rc = blob_parse(host_buf, n, &v)) != NFSP_OK) return rc;
  NFSP_REQUIRE(v.h.kind == KIND_GROUP, "state blob: a single engine's (nfsp_engine_load_state)");
  GroupRec gr;
  memcpy(&gr, v.at(0), sizeof(gr));
  NFSP_REQUIRE(gr.R == G.R && gr.flags == G.flags, "state blob: replicas or flags differ from the group's");
  for (int r = 0; r < G.R; ++r) {
    HostRec hr;
    memcpy(&hr, v.at(v.engine_sec(r)), sizeof(hr));
    if ((rc = compat_check(G.eng[r], hr, r)) != NFSP_OK) return rc;
  }
  if ((rc = group_rest(g, "nfsp_group_load_state", true)) != NFSP_OK) return rc;
  NFSP_HIP(hipMemcpy(G.w0, v.at(0) + sizeof(gr), sizeof(float) * 6 * nn::NP, hipMemcpyHostToDevice));
  for (int r = 0; r < G.R; ++r)
    if ((rc = engine_restore(G.eng[r], v, v.engine_sec(r))) != NFSP_OK) return rc;
  *G.w0_valid = gr.w0_valid;
  *G.w0_loaded = gr.w0_valid;
  // calls matters modulo the exchange cadence only, and a boundary is a multiple of it
  *G.calls = (G.xchg_every > 0 && gr.calls % G.xchg_every != 0) ? 0 : gr.calls;
  // prove the device state: the group record on the host, w0 and every replica in place
  uint64_t d[2] = {0, 0};
  digest_words(d, &gr, sizeof(gr) / 8, 0);
  DigestTable T{};
  T.n = 1;
  T.seg[0] = DigestSeg{reinterpret_cast<const uint64_t*>(G.w0), sizeof(float) * 6 * nn::NP / 8, sizeof(gr) / 8};
  if ((rc = digest_run(G.eng[0], T, d)) != NFSP_OK) return rc;
  for (int r = 0; r < G.R; ++r) {
    MemView mv;
    if ((rc = engine_view(G.eng[r], "nfsp_group_load_state", &mv)) != NFSP_OK) return rc;
    const uint64_t base = (v.sec[v.engine_sec(r)].offset - v.h.payload_offset) / 8;
    if ((rc = engine_digest(G.eng[r], mv, base, d)) != NFSP_OK) return rc;
  }
  if (d[0] != v.h.digest[0] || d[1] != v.h.digest[1])
    return nfsp::fail(NFSP_EHIP, "nfsp_group_load_state: the device state's digest differs from the blob's after the copy");
  return NFSP_OK;
}
