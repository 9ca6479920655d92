// output_plan_main.cpp -- the host-side plan of the output stage (batotp_amd/csrc/output_plan.h) as a program of its own, for
// tests/test_output_plan.py: no device, no library, so it also runs under the host sanitizers.
//
//   output_plan_main CASE
//
// CASE is a text file of numbers (doubles as C99 hex floats or "nan"):
//   K path0 out_res out_smooth_fact R torque_step pose budget
//   then per path: n_fwd t_total status_rev status_fwd step
// Output, one record per line:
//   path k n off sres  nFwd n1 n2 nF window tStep vfactT  route need
//   plan totF mixed maxChunk
//   cuts c0 c1 ...
//   chunk ka kb staged
//   route r Kc t1 t2 tS tF                       (only routes with t1 > 0: the ones the stage launches)
//   at p off1 off2 offS offF offD n1 n2 nFwd nF  (the paths of that route)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "output_plan.h"

using namespace bk;

static FILE *in;
static std::string token()
{
   char buf[128];
   if (fscanf(in, "%127s", buf) != 1) { fprintf(stderr, "case file ends early\n"); exit(2); }
   return buf;
}
static double num() { return strtod(token().c_str(), nullptr); }
static long long integer() { return strtoll(token().c_str(), nullptr, 0); }

int main(int argc, char **argv)
{
   if (argc != 2 || !(in = fopen(argv[1], "r"))) { fprintf(stderr, "usage: output_plan_main CASE\n"); return 2; }
   const int K = (int)integer();
   const int32_t path0 = (int32_t)integer();
   const double outRes = num(), smoothFact = num();
   OutRows rows;
   rows.R = (int)integer(); rows.torqueStep = integer() != 0; rows.pose = integer() != 0;
   const double budget = num();
   if (K < 1 || rows.R < 1) { fprintf(stderr, "bad case\n"); return 2; }
   std::vector<batotp_path_result> res((size_t)K);
   std::vector<double> h((size_t)K);
   for (int k = 0; k < K; ++k)
   {
      memset(&res[k], 0, sizeof(res[k]));
      res[k].n_fwd = integer();
      res[k].t_total = num();
      res[k].status_rev = (uint32_t)integer();
      res[k].status_fwd = (uint32_t)integer();
      h[k] = num();
   }
   fclose(in);

   OutPlan pl;
   planOutput(res.data(), h.data(), K, path0, outRes, smoothFact, pl);
   cutChunks(pl, rows, budget);
   for (int k = 0; k < K; ++k)
   {
      const OutPath &q = pl.all[k];
      printf("path %d %lld %lld %a  %d %d %d %d %d %a %a  %d %zu\n", k, (long long)pl.n[k], (long long)pl.off[k], pl.sres[k], q.nFwd, q.n1, q.n2, q.nF, q.window,
             q.tStep, q.vfactT, pl.step[k].route, outScratchOf(q, pl.step[k], rows, pl.mixedCall));
   }
   printf("plan %lld %d %zu\n", (long long)pl.totF, pl.mixedCall ? 1 : 0, pl.maxChunk);
   printf("cuts");
   for (int c : pl.cuts) printf(" %d", c);
   printf("\n");
   for (size_t ci = 0; ci + 1 < pl.cuts.size(); ++ci)
   {
      const int ka = pl.cuts[ci], kb = pl.cuts[ci + 1];
      printf("chunk %d %d %d\n", ka, kb, routeLayout(pl, ka, kb, 0).staged ? 1 : 0);
      for (int route = 0; route < 4; ++route)
      {
         const RouteLayout L = routeLayout(pl, ka, kb, route);
         if (L.staged != routeLayout(pl, ka, kb, 0).staged) { fprintf(stderr, "staged depends on the route\n"); return 1; }
         if (L.t1 == 0) continue;
         printf("route %d %zu %lld %lld %lld %lld\n", route, L.pc.size(), (long long)L.t1, (long long)L.t2, (long long)L.tS, (long long)L.tF);
         for (const OutPath &q : L.pc)
            printf("at %d %lld %lld %lld %lld %lld %d %d %d %d\n", q.p, (long long)q.off1, (long long)q.off2, (long long)q.offS, (long long)q.offF, (long long)q.offD,
                   q.n1, q.n2, q.nFwd, q.nF);
      }
   }
   return 0;
}
