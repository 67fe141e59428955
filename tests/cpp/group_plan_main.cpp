// Stand-alone driver of csrc/group_plan.h for tests/test_group_plan.py (built with
// -fsanitize=address,undefined).  "fixed": prints the plans of the fixed cases, which the
// test compares with its expectations.  "sweep <n> <seed>": checks the planner's invariants
// over n random inputs; the first violation is printed and the exit status is 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "group_plan.h"

using namespace nfsp::plan;

typedef std::vector<std::vector<Segment>> JobSegs;   // [2 R], job 2 r + a

static Jobs jobs_of(const JobSegs& js) {
  Jobs j;
  for (const auto& v : js) j.push_back(&v);
  return j;
}

static void print_rounds(const char* name, const JobSegs& js, int R, int nbs, int64_t cap, bool pace) {
  RoundsPlan P;
  plan_rounds(jobs_of(js), R, nbs, cap, pace, P);
  printf("case %s\n", name);
  std::vector<int> k_of(nbs, 0);
  for (const Round& rd : P.rounds) {
    const int k = k_of[rd.p]++;
    printf("round p=%d k=%d pieces=%zu targets=%zu rn=%lld\n", rd.p, k, rd.b1 - rd.b0, rd.t1 - rd.t0, (long long)rd.rn);
    for (size_t i = rd.b0; i < rd.b1; ++i)
      printf("piece p=%d k=%d r=%d a=%d u=%lld v=%lld sync=%d\n", rd.p, k, P.pieces[i].r, P.pieces[i].a,
             (long long)P.pieces[i].u, (long long)P.pieces[i].v, (int)P.pieces[i].sync);
    for (size_t i = rd.t0; i < rd.t1; ++i)
      printf("target p=%d k=%d r=%d a=%d seg=%zu\n", rd.p, k, P.targets[i].r, P.targets[i].a, P.targets[i].seg);
  }
  printf("max_rounds %lld\n", (long long)P.max_rounds);
}

static void print_persist(const char* name, const JobSegs& js, int R, int chunk) {
  PersistPlan Q;
  const char* msg = "";
  const int rc = plan_persist(jobs_of(js), R, chunk, Q, &msg);
  printf("case %s\nrc %d %s\n", name, rc, rc ? msg : "");
  if (rc) return;
  printf("npre %u nchunks %d nitems %zu\n", Q.npre, Q.nchunks, Q.slots.size());
  printf("segs");
  for (const SegRef& s : Q.segs) printf(" %d.%d.%zu", s.r, s.a, s.seg);
  printf("\nchunk0");
  for (int32_t c : Q.chunk0) printf(" %d", c);
  printf("\njseg0");
  for (int32_t c : Q.jseg0) printf(" %d", c);
  printf("\nqueue");
  for (uint32_t i = 0; i < Q.npre; ++i) printf(" %u:%u", Q.slots[i] >> 16, Q.slots[i] & 0xFFFFu);
  size_t empty = 0;
  for (size_t i = Q.npre; i < Q.slots.size(); ++i) empty += Q.slots[i] == SLOT_EMPTY;
  printf("\nempty_after %zu\n", empty);
}

static int fixed() {
  {  // one job, one syncing segment [0, 150)
    JobSegs js = {{{0, 150, true}}, {}};
    print_rounds("one_paced", js, 1, 1, 40, true);
    print_rounds("one_unpaced", js, 1, 1, 40, false);
    print_rounds("one_cap0", js, 1, 1, 0, true);
  }
  {  // two jobs in one partition
    JobSegs js = {{{0, 150, true}}, {{0, 30, true}, {30, 100, false}}};
    print_rounds("two_paced", js, 1, 1, 40, true);
    print_rounds("two_cap0", js, 1, 1, 0, true);
  }
  {  // R = 3, two partitions: replicas [0, 1) and [1, 3)
    JobSegs js = {{{0, 50, false}}, {}, {}, {{5, 45, false}}, {{0, 90, true}, {90, 100, false}}, {}};
    print_rounds("parts", js, 3, 2, 40, true);
  }
  {  // the persist queue: first segments of 20 and 5 items, chunk 16
    JobSegs js = {{{0, 20, true}, {20, 50, false}}, {{0, 5, true}, {5, 12, false}}};
    print_persist("persist", js, 1, 16);
    JobSegs big = {{{0, 65536, false}}, {}};
    print_persist("persist_big_segment", big, 1, 16);
    JobSegs ok = {{{0, 65535, false}}, {}};
    PersistPlan Q;
    const char* msg = "";
    printf("case persist_65535\nrc %d\n", plan_persist(jobs_of(ok), 1, 16, Q, &msg));
  }
  return 0;
}

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("violated: %s: ", #cond);            \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      return false;                               \
    }                                             \
  } while (0)

// every invariant of one rounds plan
static bool check_rounds(const JobSegs& js, int R, int nbs, int64_t cap, bool pace, const RoundsPlan& P) {
  struct Placed { int64_t k; Piece pc; };
  std::vector<std::vector<Placed>> placed(2 * R);                  // per job, in plan order
  std::vector<std::vector<int>> ntarget(2 * R);                    // per job and segment
  std::vector<std::vector<int64_t>> target_round(2 * R);
  for (int j = 0; j < 2 * R; ++j) ntarget[j].assign(js[j].size(), 0), target_round[j].assign(js[j].size(), -1);
  std::vector<int64_t> nrounds(nbs, 0);
  size_t b = 0, t = 0;
  int last_p = 0;
  for (const Round& rd : P.rounds) {
    CHECK(rd.p >= last_p && rd.p < nbs, "partition order, p=%d", rd.p);
    last_p = rd.p;
    CHECK(rd.b0 == b && rd.t0 == t && rd.b1 > rd.b0 && rd.t1 >= rd.t0, "round ranges");
    b = rd.b1, t = rd.t1;
    const int64_t k = nrounds[rd.p]++;
    const int r_lo = part_begin(rd.p, R, nbs), r_hi = part_begin(rd.p + 1, R, nbs);
    CHECK(r_lo == rd.p * R / nbs && r_hi == (rd.p + 1) * R / nbs, "partition bounds");
    for (size_t i = rd.b0; i < rd.b1; ++i) {
      const Piece& pc = P.pieces[i];
      CHECK(pc.r >= r_lo && pc.r < r_hi && (pc.a == 0 || pc.a == 1), "piece of r=%d in partition %d", pc.r, rd.p);
      placed[2 * pc.r + pc.a].push_back({k, pc});
    }
    int64_t rn = 0;
    for (size_t i = rd.t0; i < rd.t1; ++i) {
      const SegRef& tg = P.targets[i];
      CHECK(tg.r >= r_lo && tg.r < r_hi && (tg.a == 0 || tg.a == 1), "target of r=%d in partition %d", tg.r, rd.p);
      const int j = 2 * tg.r + tg.a;
      CHECK(tg.seg < js[j].size(), "target segment index");
      ++ntarget[j][tg.seg];
      target_round[j][tg.seg] = k;
      const int64_t len = js[j][tg.seg].v - js[j][tg.seg].u;
      rn = len > rn ? len : rn;
    }
    CHECK(rd.rn == rn, "rn %lld, longest segment starting in the round %lld", (long long)rd.rn, (long long)rn);
  }
  CHECK(b == P.pieces.size() && t == P.targets.size(), "pieces / targets outside every round");
  int64_t most_rounds = 0;
  for (int p = 0; p < nbs; ++p) most_rounds = nrounds[p] > most_rounds ? nrounds[p] : most_rounds;
  CHECK(P.max_rounds == most_rounds, "max_rounds %lld", (long long)P.max_rounds);
  for (int j = 0; j < 2 * R; ++j) {
    const std::vector<Segment>& segs = js[j];
    size_t s = 0;
    int64_t pos = segs.empty() ? 0 : segs[0].u;
    for (size_t i = 0; i < placed[j].size(); ++i) {
      const Piece& pc = placed[j][i].pc;
      CHECK(placed[j][i].k == (int64_t)i, "job %d: piece %zu in round %lld", j, i, (long long)placed[j][i].k);
      CHECK(s < segs.size(), "job %d: a piece past its last segment", j);
      CHECK(pc.u == pos && pc.v > pc.u && pc.v <= segs[s].v, "job %d: piece [%lld, %lld) at %lld of segment ending %lld",
            j, (long long)pc.u, (long long)pc.v, (long long)pos, (long long)segs[s].v);
      CHECK(pc.sync == (segs[s].sync && pc.v == segs[s].v), "job %d: sync of piece %zu", j, i);
      if (cap > 0) CHECK(pc.v - pc.u <= cap, "job %d: piece of %lld > cap", j, (long long)(pc.v - pc.u));
      if (pc.u == segs[s].u)
        CHECK(ntarget[j][s] == 1 && target_round[j][s] == (int64_t)i, "job %d: segment %zu's target in round %lld, first piece in %zu",
              j, s, (long long)target_round[j][s], i);
      pos = pc.v;
      if (pos == segs[s].v && ++s < segs.size()) pos = segs[s].u;
    }
    CHECK(s == segs.size(), "job %d: %zu of %zu segments run", j, s, segs.size());
    for (size_t q = 0; q < segs.size(); ++q) CHECK(ntarget[j][q] == 1, "job %d: segment %zu has %d targets", j, q, ntarget[j][q]);
  }
  for (int p = 0; p < nbs; ++p) {
    const int r_lo = part_begin(p, R, nbs), r_hi = part_begin(p + 1, R, nbs);
    if (cap == 0) {
      size_t most = 0;
      for (int j = 2 * r_lo; j < 2 * r_hi; ++j) most = js[j].size() > most ? js[j].size() : most;
      CHECK(nrounds[p] == (int64_t)most, "cap 0: partition %d has %lld rounds, %zu segments at most", p,
            (long long)nrounds[p], most);
    }
    if (cap > 0 && pace) {       // the busiest job: most updates, the first of equals
      int64_t most = -1;
      int busiest = -1;
      for (int j = 2 * r_lo; j < 2 * r_hi; ++j) {
        if (js[j].empty()) continue;
        int64_t n = 0;
        for (const Segment& sg : js[j]) n += sg.v - sg.u;
        if (n > most) most = n, busiest = j;
      }
      for (int j = 2 * r_lo; j < 2 * r_hi && busiest >= 0; ++j)
        for (size_t i = 0; i < placed[j].size() && i < placed[busiest].size(); ++i) {
          const Piece &pc = placed[j][i].pc, &bp = placed[busiest][i].pc;
          CHECK(pc.v - pc.u <= bp.v - bp.u, "job %d round %zu: piece of %lld, the busiest job's %lld", j, i,
                (long long)(pc.v - pc.u), (long long)(bp.v - bp.u));
        }
    }
  }
  return true;
}

static int sweep(int n, unsigned seed) {
  std::mt19937 rng(seed);
  auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
  static const int64_t caps[5] = {0, 1, 7, 16, 40};
  for (int it = 0; it < n; ++it) {
    const int R = rnd(1, 6), nbs = rnd(1, R < 4 ? R : 4);
    const int64_t cap = caps[rnd(0, 4)];
    const bool pace = rnd(0, 1) != 0;
    JobSegs js(2 * R);
    for (auto& segs : js) {
      int64_t u = rnd(0, 5);
      for (int k = rnd(0, 3); k > 0; --k) {
        const int64_t v = u + rnd(1, 120);
        segs.push_back({u, v, rnd(0, 1) != 0});
        u = v;
      }
    }
    RoundsPlan P;
    plan_rounds(jobs_of(js), R, nbs, cap, pace, P);
    if (!check_rounds(js, R, nbs, cap, pace, P)) {
      printf("input %d: R=%d nbs=%d cap=%lld pace=%d\n", it, R, nbs, (long long)cap, (int)pace);
      for (int j = 0; j < 2 * R; ++j) {
        printf(" job %d:", j);
        for (const Segment& sg : js[j]) printf(" [%lld,%lld)%s", (long long)sg.u, (long long)sg.v, sg.sync ? "s" : "");
        printf("\n");
      }
      return 1;
    }
  }
  printf("sweep ok %d\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !strcmp(argv[1], "fixed")) return fixed();
  if (argc >= 4 && !strcmp(argv[1], "sweep")) return sweep(atoi(argv[2]), (unsigned)strtoul(argv[3], nullptr, 10));
  fprintf(stderr, "usage: %s fixed | sweep <inputs> <seed>\n", argv[0]);
  return 2;
}
