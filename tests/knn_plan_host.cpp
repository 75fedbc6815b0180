// Host driver of graphlearning_amd/csrc/knn_plan.h for tests/test_knn_plan.py (no HIP header on the include path).
//   plans            one row per case of the grid below: "n d k nq long_lists overrides concat | <the KnnPlan>", cerr as a hex float
//   extras           the later decisions: S rows (seeding), E rows (escalation: the smallest count of flagged rows that escalates,
//                    and the decision either side of it and of 64 | 65), F rows (the wide fallback's sizes)
//   chain FILE M D   knn_chain_places of the M x D doubles in FILE: the places, one line
//   scale R ...      knn_filter_scale of every R (hex floats welcome): one "%a" per line
//   accept_eps CERR QNORM RMAX DK2S
//                    knn_accept_eps, the margin of the re-rank's acceptance test: one "%a"
//   plan N D K NQ LONG FILTER LISTS NSPLIT CONCAT
//                    the plan of one case under the overrides {FILTER, LISTS, NSPLIT, CONCAT} (glx_knn_options' numbers), one row in the
//                    format of `plans`; D and K may be ranges LO:HI (inclusive): one row per (d, k), d outermost
// The row formats are those of the table recorded in tests/golden/knn_plans.txt.
#include "knn_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static glx_knn_options g_opt = {0, 0, 0, -1};

static void plan_row(int64_t n, int d, int k, int64_t nq, bool long_lists) {
  const KnnPlan p = knn_make_plan(n, d, k, nq, long_lists, g_opt);
  printf("%lld %d %d %lld %d %d %d | %d %d %d %d %d %d %lld %d %d %d %d %lld %lld %d %d %d %d %a\n", (long long)n, d, k, (long long)nq,
         (int)long_lists, g_opt.filter * 1000 + g_opt.lists * 100 + g_opt.nsplit, g_opt.concat, p.KP, p.DH, p.nkb, p.NKB, p.dpa, p.BR,
         (long long)p.ntiles, p.nsplit, p.lists, p.ncand, p.M, (long long)p.chunk, (long long)p.nchunks, (int)p.short_lists, (int)p.wide,
         (int)p.use_bf16, p.cat, p.cerr);
}

static void plans() {
  const int64_t ns[] = {1, 2, 33, 257, 4096, 70000, 1000000, 10000000};
  const int ds[] = {1, 16, 17, 20, 21, 22, 33, 34, 35, 64, 65, 128, 129, 130, 131, 784, 16382};
  const int ks[] = {1, 12, 13, 28, 29, 60, 61, 128, 129, 512, 513, 1024};
  const glx_knn_options opts[] = {{0, 0, 0, -1}, {2, 0, 0, -1}, {0, 2, 0, -1}, {0, 0, 1, -1}, {0, 0, 3, -1}, {0, 0, 64, -1}, {0, 0, 0, 0}, {0, 0, 0, 1}};
  for (int oi = 0; oi < 8; ++oi) {
    g_opt = opts[oi];
    for (int64_t n : ns) {
      if (oi && n != 257 && n != 70000) continue;
      for (int d : ds)
        for (int k : ks) {
          if (k > n) continue;
          for (int ll = 0; ll < 2; ++ll) {
            plan_row(n, d, k, n, ll);
            if (n > 300) plan_row(n, d, k, 300, ll);
          }
        }
    }
  }
}

// share < 0: the first pass was not cell-pruned
static bool escalates(int64_t n, int d, int k, int64_t nq, bool ll, int64_t nbad, double share) {
  return knn_should_escalate(knn_make_plan(n, d, k, nq, ll, g_opt), n, d, k, nq, (size_t)nbad, share >= 0 ? share : 1.0);
}

static void escalation_row(int64_t n, int d, int k, int64_t nq, bool ll, double share) {
  int64_t lo = 0, hi = nq + 1;
  if (!escalates(n, d, k, nq, ll, nq, share)) {
    lo = hi = -1;
  } else {
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) / 2;
      if (escalates(n, d, k, nq, ll, mid, share)) hi = mid; else lo = mid;
    }
  }
  printf("E %lld %d %d %lld %d %d %.3f | %lld", (long long)n, d, k, (long long)nq, (int)ll, g_opt.filter, share, (long long)hi);
  for (int64_t nb : {(int64_t)0, (int64_t)64, (int64_t)65, hi - 1, hi, hi + 1, nq})
    if (nb >= 0 && nb <= nq) printf(" %lld:%d", (long long)nb, (int)escalates(n, d, k, nq, ll, nb, share));
  printf("\n");
}

static void extras() {
  for (int64_t n : {(int64_t)70000, (int64_t)10000000})
    for (int d : {20, 128})
      for (int k : {1, 12, 13, 28, 29, 60, 61, 64, 65, 128})
        for (int ll = 0; ll < 2; ++ll)
          for (int nc : {-1, 1, 2, 16, 64, 1024, 4096}) {   // (-1: rows that come in no cells)
            const KnnSeedPlan s = knn_seed_plan(knn_make_plan(n, d, k, n, ll, g_opt), k, nc < 0 ? 0 : nc);
            printf("S %lld %d %d %lld %d %d | %d %d\n", (long long)n, d, k, (long long)n, ll, nc, s.sub, (int)s.seeded);
          }
  for (int f : {0, 2}) {
    g_opt = {f, 0, 0, -1};
    for (int64_t n : {(int64_t)4096, (int64_t)70000, (int64_t)1000000})
      for (int d : {20, 128, 130, 131})
        for (int k : {12, 60, 61, 1024})
          for (int ll = 0; ll < 2; ++ll)
            for (double share : {-1.0, 0.005, 0.3}) {
              if (ll && share >= 0) continue;
              escalation_row(n, d, k, n, ll, share);
              escalation_row(n, d, k, 300, ll, share);
            }
  }
  g_opt = {0, 0, 0, -1};
  for (int k : {61, 64, 65, 128, 129, 256, 257, 512, 513, 1024})
    for (size_t nr : {(size_t)1, (size_t)100, (size_t)1332, (size_t)70000, (size_t)1000000, (size_t)10000000}) {
      const KnnWideFallbackPlan f = knn_wide_fallback_plan(k, nr);
      printf("F %d %zu | %d %zu\n", k, nr, f.cap, f.batch);
    }
}

static int chain(const char* path, int m, int d) {
  std::vector<double> cen((size_t)m * d);
  FILE* f = fopen(path, "rb");
  if (!f || fread(cen.data(), 8, cen.size(), f) != cen.size()) return 1;
  fclose(f);
  for (int p : knn_chain_places(cen, m, d)) printf("%d ", p);
  printf("\n");
  return 0;
}

static void range(const char* s, int* lo, int* hi) {
  *lo = *hi = atoi(s);
  if (const char* c = strchr(s, ':')) *hi = atoi(c + 1);
}

static int plan(char** a) {
  int d0, d1, k0, k1;
  range(a[1], &d0, &d1);
  range(a[2], &k0, &k1);
  const int64_t n = atoll(a[0]), nq = atoll(a[3]);
  g_opt = {atoi(a[5]), atoi(a[6]), atoi(a[7]), atoi(a[8])};
  if (n < 1 || nq < 1 || d0 < 1 || k0 < 1 || g_opt.filter < 0 || g_opt.filter > 2 || g_opt.lists < 0 || g_opt.lists > 2 || g_opt.nsplit < 0 ||
      g_opt.nsplit > 32 || g_opt.concat < -1 || g_opt.concat > 2)
    return 2;
  for (int d = d0; d <= d1; ++d)
    for (int k = k0; k <= k1; ++k) plan_row(n, d, k, nq, atoi(a[4]) != 0);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "plans")) { plans(); return 0; }
  if (argc == 2 && !strcmp(argv[1], "extras")) { extras(); return 0; }
  if (argc == 5 && !strcmp(argv[1], "chain")) return chain(argv[2], atoi(argv[3]), atoi(argv[4]));
  if (argc >= 3 && !strcmp(argv[1], "scale")) {
    for (int a = 2; a < argc; ++a) printf("%a\n", knn_filter_scale(strtod(argv[a], nullptr)));
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "accept_eps")) {
    printf("%a\n", knn_accept_eps(strtod(argv[2], nullptr), strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr)));
    return 0;
  }
  if (argc == 11 && !strcmp(argv[1], "plan")) return plan(argv + 2);
  fprintf(stderr, "usage: knn_plan_host plans | extras | chain FILE M D | scale R ... | accept_eps CERR QNORM RMAX DK2S | plan N D K NQ LONG FILTER LISTS NSPLIT CONCAT\n");
  return 2;
}
