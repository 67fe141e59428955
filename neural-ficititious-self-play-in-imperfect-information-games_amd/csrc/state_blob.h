// The state blob (checkpoint format, version 1) and its digest: shared by the digest kernel
// and the host parser of state.hip, and by nothing else.  DESIGN.md §10 has the byte offsets.
//
//   header   BlobHeader (104 B) + n_sections x BlobSection (24 B), little-endian
//   payload  the sections back to back, each a multiple of 8 bytes
//
// Digest of the payload as little-endian u64 words w[i], i = the word's index in the payload:
//   D0 = sum_i mix64(w[i] ^ (i + 1) * C0)   mod 2^64
//   D1 = sum_i mix64(w[i] + (i + 1) * C1)   mod 2^64
// mix64 = the splitmix64 finaliser.  The sums commute, so any parallel order (and any split
// between the device and the host) gives the same value; the terms depend on i, so a
// reordered payload does not.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NFSP_BLOB_HD __host__ __device__
#else
#define NFSP_BLOB_HD
#endif

namespace nfsp {
namespace blob {

constexpr uint64_t C0 = 0x9E3779B97F4A7C15ull;
constexpr uint64_t C1 = 0xC2B2AE3D27D4EB4Full;

NFSP_BLOB_HD inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// word w at payload index i, added to both sums
NFSP_BLOB_HD inline void digest_add(uint64_t& d0, uint64_t& d1, uint64_t w, uint64_t i) {
  d0 += mix64(w ^ ((i + 1) * C0));
  d1 += mix64(w + (i + 1) * C1);
}
// words [0, n) of p, the first at payload index `first` (host side)
inline void digest_words(uint64_t d[2], const void* p, uint64_t n, uint64_t first) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (uint64_t k = 0; k < n; ++k) {
    uint64_t w = 0;
    for (int j = 7; j >= 0; --j) w = (w << 8) | b[8 * k + j];   // little-endian, any alignment
    digest_add(d[0], d[1], w, first + k);
  }
}

constexpr char MAGIC[8] = {'N', 'F', 'S', 'P', 'S', 'T', 'A', 'T'};
constexpr uint32_t VERSION = 1;
enum : uint32_t { KIND_ENGINE = 1, KIND_GROUP = 2 };
// section kinds; an engine payload is HOST, ST, NETS, RL, SL in this order, a group payload
// GROUP and then its replicas' engine payloads
enum : uint32_t { SEC_HOST = 1, SEC_ST = 2, SEC_NETS = 3, SEC_RL = 4, SEC_SL = 5, SEC_GROUP = 6 };
constexpr int ENGINE_SECTIONS = 5;

struct BlobHeader {
  char magic[8];             //   0  "NFSPSTAT"
  uint32_t version;          //   8  1
  uint32_t kind;             //  12  KIND_ENGINE | KIND_GROUP
  uint64_t total_bytes;      //  16  header + payload
  uint64_t payload_offset;   //  24  = 104 + 24 * n_sections
  uint64_t payload_bytes;    //  32
  uint64_t digest[2];        //  40  D0, D1 of the payload
  uint32_t sz_cfg;           //  56  sizeof(nfsp_engine_cfg)
  uint32_t sz_dev;           //  60  sizeof(EngineDev)
  uint32_t sz_rl;            //  64  sizeof(RlRec) = 32
  uint32_t sz_sl;            //  68  sizeof(SlRec) = 16
  uint32_t sz_host;          //  72  sizeof(HostRec)
  uint32_t np;               //  76  f32 parameters per net
  uint32_t replicas;         //  80  1 for an engine
  uint32_t n_sections;       //  84  5 (engine) | 1 + 5 * replicas (group)
  int32_t slices;            //  88  the saving engine's cfg.slices,
  int32_t slice_lag;         //  92    cfg.slice_lag
  uint32_t sched;            //  96    and cfg.sched (the payload holds 1, 1, 0)
  uint32_t reserved;         // 100  0
};
struct BlobSection {
  uint32_t kind;             //   0  SEC_*
  uint32_t replica;          //   4
  uint64_t offset;           //   8  from the start of the blob
  uint64_t bytes;            //  16  a multiple of 8
};
static_assert(sizeof(BlobHeader) == 104 && sizeof(BlobSection) == 24, "blob header layout");

}  // namespace blob
}  // namespace nfsp
