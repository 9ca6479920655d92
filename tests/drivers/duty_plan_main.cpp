// duty_plan_main.cpp -- the host rule of the continuous torque rating (batotp_amd/csrc/duty_rounds.h) and the decision of a stretch
// round with a duty record (batotp_amd/csrc/stretch_rounds.h) as a program of its own for tests/test_duty_cpu.py.  No device, no
// library.  Doubles are read as C99 hex floats, "inf" or "nan", and printed as hex floats.
//
//   duty_plan_main records CASE
//       CASE: n_links target, n_links ratings, then any number of paths: h, 56 sums S[joint][moment], W, peak_power, power_at, n_pts
//       Output per path: "duty k rms[0..7] util row n_hold s s_row energy peak_power power_at n_pts"
//   duty_plan_main rounds CASE
//       CASE: target max_rounds max_factor K, then K point counts, then any number of rounds of K records
//         peak[0..4] s n_static util n_hold duty_s
//       Output as range_plan_main rounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "duty_rounds.h"
#include "stretch_rounds.h"

using namespace bk;

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

static int records(const char *path)
{
   if (!(in = fopen(path, "r"))) return 2;
   const int nl = (int)num();
   const double target = num();
   double rated[BATOTP_MAX_LINKS] = {0};
   if (nl < 1 || nl > BATOTP_MAX_LINKS) return 2;
   for (int j = 0; j < nl; ++j) rated[j] = num();
   DutyRating R;
   dutyRating(nl, rated, target, R);
   std::string t;
   for (int k = 0; token(t); ++k)
   {
      const double h = strtod(t.c_str(), nullptr);
      batotp_path_duty_sums S;
      batotp_path_duty d;
      memset(&S, 0, sizeof(S));
      memset(&d, 0, sizeof(d));
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
         for (int m = 0; m < 7; ++m) S.S[j][m] = num();
      S.W = num(); S.peak_power = num(); S.power_at = (int64_t)num(); S.n_pts = (int64_t)num();
      dutyRecord(S, R, h, d);
      printf("duty %d", k);
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j) printf(" %a", d.rms[j]);
      printf(" %a %d %d %a %d %a %a %lld %lld\n", d.util, (int)d.row, (int)d.n_hold, d.s, (int)d.s_row, d.energy, d.peak_power, (long long)d.power_at,
             (long long)d.n_pts);
   }
   fclose(in);
   return 0;
}

static int rounds(const char *path)
{
   if (!(in = fopen(path, "r"))) return 2;
   const double target = num();
   const int32_t maxRounds = (int32_t)num();
   const double maxFactor = num();
   const int K = (int)num();
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
         batotp_path_duty d;
         memset(&a, 0, sizeof(a));
         memset(&s, 0, sizeof(s));
         memset(&d, 0, sizeof(d));
         for (int f = 0; f < BATOTP_AUDIT_FAMILIES; ++f) a.fam[f].peak = (k == 0 && f == 0) ? strtod(t.c_str(), nullptr) : num();
         s.s = num();
         s.n_static = (int64_t)num();
         d.util = num();
         d.n_hold = (int32_t)num();
         d.s = num();
         if (stretchDecide(a, &s, target, maxRounds, maxFactor, nIn[k], n2[k], st[k], &d)) again = true;
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
   if (argc == 3 && !strcmp(argv[1], "records")) rc = records(argv[2]);
   if (argc == 3 && !strcmp(argv[1], "rounds")) rc = rounds(argv[2]);
   if (rc == 2) fprintf(stderr, "usage: duty_plan_main records CASE  |  duty_plan_main rounds CASE\n");
   return rc;
}
