// tscale_batch_main.cpp -- BA::optimizeBatch with BA::setStretchToTorqueLimits and the audit on: dumps the finished rows of every path as
// raw doubles and prints BA::getLastStretch() and the torque peak of BA::getLastAudit(), for tests/test_gpu_tscale.py to compare with
// the C-ABI route on the same rows.
//
//   tscale_batch config.dat nPaths target
//
// dump.bin: per path  int64 n, nTheta, nCart, nTrq; double sres; then theta[nTheta][n], cart[nCart][n], trq[nTrq][n].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba.h"

using namespace BATOTP;

static void putRows(FILE *f, const std::vector<std::vector<double>> &rows, size_t count, size_t n)
{
   for (size_t j = 0; j < count; ++j) fwrite(rows[j].data(), sizeof(double), n, f);
}

int main(int argc, char *argv[])
{
   if (argc < 4) return 2;
   const int nPaths = atoi(argv[2]);
   BA planner;
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   planner.setIsAutoIntegRes(false);
   if (planner.readConfigData((std::string("./") + argv[1]).c_str()) == -1) return 1;
   planner.setStretchToTorqueLimits(atof(argv[3]));
   planner.setAuditTolerance(0.0);
   std::vector<Traj> paths((size_t)nPaths);
   if (planner.loadTrajectoryData(paths[0]) == -1) return 1;
   for (int p = 1; p < nPaths; ++p) paths[p] = paths[0];
   const int rc = planner.optimizeBatch(paths);
   printf("optimizeBatch %d\n", rc);
   if (rc != 0) return 3;
   FILE *f = fopen("dump.bin", "wb");
   if (!f) return 1;
   const std::vector<BatchAudit> &audit = planner.getLastAudit();
   const std::vector<BatchStretch> &st = planner.getLastStretch();
   if (audit.size() != paths.size() || st.size() != paths.size()) return 5;
   for (size_t p = 0; p < paths.size(); ++p)
   {
      const Traj &t = paths[p];
      const size_t n = t.nPts;
      size_t nCart = 0, nTrq = 0;
      while (nCart < t.cart.size() && t.cart[nCart].size() == n) ++nCart;
      while (nTrq < t.trq.size() && t.trq[nTrq].size() == n) ++nTrq;
      const long long head[4] = {(long long)n, (long long)t.theta.size(), (long long)nCart, (long long)nTrq};
      fwrite(head, sizeof(long long), 4, f);
      fwrite(&t.sres, sizeof(double), 1, f);
      putRows(f, t.theta, t.theta.size(), n);
      putRows(f, t.cart, nCart, n);
      putRows(f, t.trq, nTrq, n);
      unsigned long long bits = 0;
      memcpy(&bits, &audit[p].peak[4], sizeof(bits));
      printf("tscale %zu n_in %lld n_out %lld rounds %d status %d done %d trq_peak %016llx n_over %lld t_total %.17g\n", p, st[p].nIn, st[p].nOut, st[p].rounds,
             st[p].status, (int)st[p].done, bits, audit[p].nOver, t.tTotalTraj);
   }
   fclose(f);
   return 0;
}
