// Everything the host derives from an nfsp_engine_cfg, as pure functions: the sizes of an engine's
// buffers (engine_sizes), the rules a cfg must satisfy (engine_cfg_rule), and the table of the
// struct's fields with what each is to an engine group and to a state blob (CFG_FIELDS,
// cfg_first_diff, cfg_stored).  Standard headers and nfsp.h only, so it is tested without a GPU
// (tests/test_engine_cfg.py).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "nfsp.h"

namespace nfsp {
namespace eng {

constexpr int MAX_BATCH = 128;     // learner minibatch (config MiniBatchSize)
constexpr int CHAIN_MB = 32;       // fit minibatch of the SGD chains (Keras batch_size)
constexpr int CFG_HIDDEN = 64;               // nn::H and sizeof(StepRec): engine_internal.h pins
constexpr int64_t STEP_REC_BYTES = 2560;     // both where those are defined

struct EngineSizes {
  int N;               // lanes per rollout (one slice): staging and learner bounds
  int nblk;            // 256-lane blocks of the scans and the commit
  // an agent makes <= 4 decisions per hand: <= 4 RL and <= 4 SL records per lane
  int64_t log_cap;     // rows of an agent's circular M_RL log
  int64_t pend_cap;    // an agent's pending SL records of one rollout
  int64_t umax;        // <= 4N RL inserts per agent per rollout -> <= 4N / c + 2 update triggers
  int64_t steps;       // SGD steps (step records) of one update: [epochs][batch / 32]
  int64_t rec_bytes;   // one agent's step records of a learner call: [umax][steps] StepRec
};

// of a cfg with slices >= 1 and inserts_per_update >= 1 (engine_cfg_rule checks those first)
inline EngineSizes engine_sizes(const nfsp_engine_cfg& c) {
  EngineSizes z;
  z.N = c.n_lanes / c.slices;
  z.nblk = (z.N + 255) / 256;
  z.log_cap = c.rl_capacity + 4 * (int64_t)z.N;
  z.pend_cap = 4 * (int64_t)z.N;
  z.umax = 4 * (int64_t)z.N / c.inserts_per_update + 2;
  z.steps = (int64_t)c.epochs * (c.batch / CHAIN_MB);
  z.rec_bytes = z.umax * z.steps * STEP_REC_BYTES;
  return z;
}

// What any engine's cfg must satisfy: the first broken rule's message, or nullptr.
inline const char* engine_cfg_rule(const nfsp_engine_cfg& c) {
  if (c.hidden != CFG_HIDDEN) return "only hidden == 64 is built";
  if (!(c.n_lanes > 0 && c.n_lanes < (1 << 24))) return "n_lanes must be in [1, 2^24)";
  if (!(c.slices >= 1 && c.n_lanes % c.slices == 0)) return "slices must be >= 1 and divide n_lanes";
  if (!(c.slice_lag == 1 || c.slice_lag == 2)) return "slice_lag must be 1 or 2";
  if (c.fit_batch != CHAIN_MB) return "the SGD chains are built for fit_batch == 32";
  if (!(c.batch >= CHAIN_MB && c.batch <= MAX_BATCH && c.batch % CHAIN_MB == 0))
    return "batch must be 32, 64, 96 or 128";
  if (!(c.epochs >= 1 && c.epochs <= 4)) return "epochs must be in [1, 4]";
  if (!(c.rl_capacity > c.batch && c.sl_capacity > c.batch)) return "capacities must exceed the batch";
  // reservoir slots are int32 in the learner (LearnBufs::res_slot)
  if (!(c.sl_capacity < (1ll << 31))) return "sl_capacity must be < 2^31";
  if (!(c.rl_capacity < (1ll << 40))) return "rl_capacity too large";
  if (!(c.inserts_per_update >= 1 && c.target_every >= 1)) return "bad cadence";
  if (c.quirks & ~(NFSP_QUIRKS_REFERENCE | NFSP_TEXTBOOK_MSE)) return "unknown bits in quirks (NFSP_QUIRK_* | NFSP_EXT_*)";
  if ((c.quirks & NFSP_EXT_MSE_Q) && !(c.quirks & NFSP_EXT_LINEAR_Q)) return "NFSP_EXT_MSE_Q requires NFSP_EXT_LINEAR_Q";
  // the chains read an agent's step records through a buffer descriptor with 32-bit offsets
  // (k_chain3): [umax][epochs][batch / 32] records of one learner call must stay below 2 GiB
  if (!(engine_sizes(c).rec_bytes < (1ll << 31)))
    return "one slice's step records exceed 2 GiB: use more slices (or more inserts per update)";
  return nullptr;
}

// What a field is to an engine group and to a state blob:
//   SHAPE    shapes the group's shared launches (lanes, batch, epochs, the buffers sized from
//            them, the memories' sizes): the replicas share it; stored in a blob
//   HYPER    a hyperparameter a replica may own; stored in a blob
//   SESSION  a setting the training state does not depend on: the replicas share it; a blob's
//            payload holds 1, 1, 0 (slices, slice_lag, sched) whatever the saving engine's were
enum CfgClass : unsigned { CFG_SHAPE = 1u, CFG_HYPER = 2u, CFG_SESSION = 4u };
struct CfgField {
  const char* name;
  size_t offset, size;
  CfgClass cls;
};
#define NFSP_CFG_ROW(f, cls) {#f, offsetof(nfsp_engine_cfg, f), sizeof(nfsp_engine_cfg::f), cls}
constexpr CfgField CFG_FIELDS[] = {   // every field of nfsp_engine_cfg, in declaration order
    NFSP_CFG_ROW(n_lanes, CFG_SHAPE),
    NFSP_CFG_ROW(hidden, CFG_SHAPE),
    NFSP_CFG_ROW(rl_capacity, CFG_SHAPE),
    NFSP_CFG_ROW(sl_capacity, CFG_SHAPE),
    NFSP_CFG_ROW(batch, CFG_SHAPE),
    NFSP_CFG_ROW(inserts_per_update, CFG_SHAPE),
    NFSP_CFG_ROW(target_every, CFG_HYPER),
    NFSP_CFG_ROW(epochs, CFG_SHAPE),
    NFSP_CFG_ROW(fit_batch, CFG_SHAPE),
    // the one exception: the bits CFG_SHARED_QUIRKS of this hyperparameter select the BR chain
    // kernel of a shared launch (k_chain3<1 / 2 / 3>), so a group's replicas share them
    NFSP_CFG_ROW(quirks, CFG_HYPER),
    NFSP_CFG_ROW(eta, CFG_HYPER),
    NFSP_CFG_ROW(lr_br, CFG_HYPER),
    NFSP_CFG_ROW(lr_ar, CFG_HYPER),
    NFSP_CFG_ROW(gamma, CFG_HYPER),
    NFSP_CFG_ROW(epsilon, CFG_HYPER),
    NFSP_CFG_ROW(seed, CFG_HYPER),
    NFSP_CFG_ROW(slices, CFG_SESSION),
    NFSP_CFG_ROW(slice_lag, CFG_SESSION),
    NFSP_CFG_ROW(sched, CFG_SESSION),
};
#undef NFSP_CFG_ROW
constexpr uint32_t CFG_SHARED_QUIRKS = NFSP_EXT_LINEAR_Q | NFSP_EXT_MSE_Q;

// the rows and the struct's two padding words (before gamma and at the end) tile the struct: a
// new field does not compile without a row
constexpr bool cfg_fields_tile() {
  size_t pos = 0;
  int pads = 0;
  for (const CfgField& f : CFG_FIELDS) {
    if (f.offset == pos + 4) { pos += 4; pads++; }
    if (f.offset != pos) return false;
    pos += f.size;
  }
  return pads == 1 && pos + 4 == sizeof(nfsp_engine_cfg);
}
static_assert(cfg_fields_tile(), "CFG_FIELDS must list every field of nfsp_engine_cfg, in order");

// The first field of the classes `mask` in which b differs from a (by its bytes: -0.0 and 0.0 are
// different cfgs), or nullptr.  quirks: the whole word as a hyperparameter, else its shared bits
// as a shape.
inline const char* cfg_first_diff(const nfsp_engine_cfg& a, const nfsp_engine_cfg& b, unsigned mask) {
  for (const CfgField& f : CFG_FIELDS) {
    if ((mask & f.cls) && memcmp((const char*)&a + f.offset, (const char*)&b + f.offset, f.size)) return f.name;
    if (f.offset == offsetof(nfsp_engine_cfg, quirks) && (mask & CFG_SHAPE) && ((a.quirks ^ b.quirks) & CFG_SHARED_QUIRKS))
      return "quirks (NFSP_EXT_LINEAR_Q | NFSP_EXT_MSE_Q)";
  }
  return nullptr;
}

// c as a state blob stores it: the shape and hyperparameter fields, the session fields 1, 1, 0,
// padding bytes zero
inline nfsp_engine_cfg cfg_stored(const nfsp_engine_cfg& c) {
  nfsp_engine_cfg r;
  memset(&r, 0, sizeof(r));
  for (const CfgField& f : CFG_FIELDS)
    if (f.cls != CFG_SESSION) memcpy((char*)&r + f.offset, (const char*)&c + f.offset, f.size);
  r.slices = r.slice_lag = 1;
  return r;
}

}  // namespace eng
}  // namespace nfsp
