// Stand-alone driver of csrc/engine_cfg.h for tests/test_engine_cfg.py (built with
// -fsanitize=address,undefined).  `engine_cfg_main fields` prints the field table, one row per
// line: name offset size class.  Otherwise it reads one command per line from stdin, a cfg being
// its 19 fields in declaration order (the floats as the hex of their 32 bits, the doubles of
// their 64):
//   c <cfg>               the broken rule's message, or the sizes
//   d <mask> <cfg> <cfg>  cfg_first_diff's field name, or "-"
//   s <cfg>               cfg_stored's 104 bytes in hex
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "engine_cfg.h"

using namespace nfsp::eng;

static bool read_cfg(nfsp_engine_cfg* c) {
  uint32_t f[3];
  uint64_t d[2];
  memset(c, 0xA5, sizeof(*c));      // the padding too: nothing may depend on it
  if (scanf("%" SCNd32 " %" SCNd32 " %" SCNd64 " %" SCNd64 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32 " %" SCNd32
            " %" SCNu32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx64 " %" SCNx64 " %" SCNu64 " %" SCNd32 " %" SCNd32
            " %" SCNu32,
            &c->n_lanes, &c->hidden, &c->rl_capacity, &c->sl_capacity, &c->batch, &c->inserts_per_update,
            &c->target_every, &c->epochs, &c->fit_batch, &c->quirks, &f[0], &f[1], &f[2], &d[0], &d[1], &c->seed,
            &c->slices, &c->slice_lag, &c->sched) != 19)
    return false;
  memcpy(&c->eta, &f[0], 4);
  memcpy(&c->lr_br, &f[1], 4);
  memcpy(&c->lr_ar, &f[2], 4);
  memcpy(&c->gamma, &d[0], 8);
  memcpy(&c->epsilon, &d[1], 8);
  return true;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "fields")) {
    for (const CfgField& f : CFG_FIELDS)
      printf("%s %zu %zu %s\n", f.name, f.offset, f.size,
             f.cls == CFG_SHAPE ? "shape" : f.cls == CFG_HYPER ? "hyper" : "session");
    return 0;
  }
  char cmd[2];
  while (scanf("%1s", cmd) == 1) {
    nfsp_engine_cfg a, b;
    if (cmd[0] == 'c' && read_cfg(&a)) {
      if (const char* rule = engine_cfg_rule(a)) {
        printf("err %s\n", rule);
        continue;
      }
      const EngineSizes z = engine_sizes(a);
      printf("ok N=%d nblk=%d log_cap=%" PRId64 " pend_cap=%" PRId64 " umax=%" PRId64 " steps=%" PRId64
             " rec_bytes=%" PRId64 "\n", z.N, z.nblk, z.log_cap, z.pend_cap, z.umax, z.steps, z.rec_bytes);
    } else if (unsigned mask; cmd[0] == 'd' && scanf("%u", &mask) == 1 && read_cfg(&a) && read_cfg(&b)) {
      const char* f = cfg_first_diff(a, b, mask);
      printf("%s\n", f ? f : "-");
    } else if (cmd[0] == 's' && read_cfg(&a)) {
      const nfsp_engine_cfg r = cfg_stored(a);
      unsigned char raw[sizeof(r)];
      memcpy(raw, &r, sizeof(r));
      for (unsigned char x : raw) printf("%02x", x);
      printf("\n");
    } else {
      return 2;                       // a malformed line
    }
  }
  return 0;
}
