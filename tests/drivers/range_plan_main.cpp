// range_plan_main.cpp -- the host-side pieces that every output made from an output shares, as a program of its own for
// tests/test_range_plan.py: the cuts and the block tables of batotp_amd/csrc/output_plan.h and the decision of a stretch round of
// batotp_amd/csrc/stretch_rounds.h.  No device, no library.
//
//   range_plan_main cuts BP BUDGET PER_PATH PER_BLOCK PER_POINT n0 n1 ...
//       a path of n points needs PER_PATH + PER_BLOCK * blocks + PER_POINT * n bytes; BUDGET is a C99 hex float.  Output:
//         cuts c0 c1 ...
//         max BYTES
//         range ka kb nBlocks            (one per range, then one line per path of it)
//         path k first nb                (first: place of its first block in the range; its blocks must follow as (k - ka, 0 .. nb - 1))
//       "range ka kb overflow" where pathBlocks refuses the range
//   range_plan_main rounds CASE
//       CASE: target max_rounds max_factor K with_scale, then K point counts, then any number of rounds of K records
//         peak[0..4] s n_static          (doubles as hex floats, "inf" or "nan")
//       Output per round: "round again" and per path "path k n_out rounds status capped"; then per path "report k n_in n_out factor
//       rounds status"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "output_plan.h"
#include "stretch_rounds.h"

using namespace bk;

static int cuts(int argc, char **argv)
{
   if (argc < 7) return 2;
   const int bp = atoi(argv[2]);
   const double budget = strtod(argv[3], nullptr);
   const size_t perPath = strtoull(argv[4], nullptr, 0), perBlock = strtoull(argv[5], nullptr, 0), perPoint = strtoull(argv[6], nullptr, 0);
   std::vector<int64_t> n;
   for (int i = 7; i < argc; ++i) n.push_back(strtoll(argv[i], nullptr, 0));
   std::vector<int> c;
   const size_t maxRange = cutRanges((int)n.size(), [&](int k) { return perPath + perBlock * (size_t)blocksOf(n[k], bp) + perPoint * (size_t)n[k]; }, budget, c);
   printf("cuts");
   for (int v : c) printf(" %d", v);
   printf("\nmax %zu\n", maxRange);
   std::vector<PathBlock> blocks;
   std::vector<int64_t> first;
   for (size_t ci = 0; ci + 1 < c.size(); ++ci)
   {
      const int ka = c[ci], kb = c[ci + 1];
      if (!pathBlocks(n.data(), ka, kb, bp, blocks, first)) { printf("range %d %d overflow\n", ka, kb); continue; }
      printf("range %d %d %zu\n", ka, kb, blocks.size());
      for (int k = ka; k < kb; ++k)
      {
         const int64_t nb = (k + 1 < kb ? first[k + 1 - ka] : (int64_t)blocks.size()) - first[k - ka];
         for (int64_t b = 0; b < nb; ++b)
         {
            const PathBlock &d = blocks[(size_t)(first[k - ka] + b)];
            if (d.path != k - ka || d.blk != b) { fprintf(stderr, "block %lld of path %d is (%d, %d)\n", (long long)b, k, d.path, d.blk); return 1; }
         }
         printf("path %d %lld %lld\n", k, (long long)first[k - ka], (long long)nb);
      }
   }
   return 0;
}

static FILE *in;
static bool token(std::string &t)
{
   char buf[128];
   if (fscanf(in, "%127s", buf) != 1) return false;
   t = buf;
   return true;
}
static double num()
{
   std::string t;
   if (!token(t)) { fprintf(stderr, "case file ends early\n"); exit(2); }
   return strtod(t.c_str(), nullptr);
}

static int rounds(const char *path)
{
   if (!(in = fopen(path, "r"))) return 2;
   const double target = num();
   const int32_t maxRounds = (int32_t)num();
   const double maxFactor = num();
   const int K = (int)num();
   const bool withScale = num() != 0;
   std::vector<int64_t> nIn((size_t)K);
   for (int k = 0; k < K; ++k) nIn[k] = (int64_t)num();
   std::vector<int64_t> n2(nIn);
   std::vector<StretchState> st((size_t)K);
   std::string t;
   while (token(t))
   {
      bool again = false;
      for (int k = 0; k < K; ++k)
      {
         batotp_path_audit a;
         batotp_path_tscale s;
         memset(&a, 0, sizeof(a));
         memset(&s, 0, sizeof(s));
         for (int f = 0; f < BATOTP_AUDIT_FAMILIES; ++f) a.fam[f].peak = (k == 0 && f == 0) ? strtod(t.c_str(), nullptr) : num();
         s.s = num();
         s.n_static = (int64_t)num();
         if (stretchDecide(a, withScale ? &s : nullptr, target, maxRounds, maxFactor, nIn[k], n2[k], st[k])) again = true;
      }
      printf("round %d\n", again ? 1 : 0);
      for (int k = 0; k < K; ++k) printf("path %d %lld %d %d %d\n", k, (long long)n2[k], st[k].rounds, st[k].status, st[k].capped ? 1 : 0);
   }
   fclose(in);
   for (int k = 0; k < K; ++k)
   {
      batotp_path_stretch r;
      memset(&r, 0, sizeof(r));
      stretchReport(nIn[k], n2[k], st[k], r);
      printf("report %d %lld %lld %a %d %d\n", k, (long long)r.n_in, (long long)r.n_out, r.factor, (int)r.rounds, (int)r.status);
   }
   return 0;
}

int main(int argc, char **argv)
{
   int rc = 2;
   if (argc >= 2 && !strcmp(argv[1], "cuts")) rc = cuts(argc, argv);
   if (argc == 3 && !strcmp(argv[1], "rounds")) rc = rounds(argv[2]);
   if (rc == 2) fprintf(stderr, "usage: range_plan_main cuts BP BUDGET PER_PATH PER_BLOCK PER_POINT n...  |  range_plan_main rounds CASE\n");
   return rc;
}
