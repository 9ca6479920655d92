// invdyn_batch_main.cpp -- BA::optimizeBatch with torque rows for paths planned without torque limits (BA::setOutputTorques) and
// the audit on: dumps the finished rows of every path as raw doubles and prints the torque peak of BA::getLastAudit() as bit
// patterns, for tests/test_gpu_invdyn.py to compare with the C-ABI route on the same rows.
//
//   invdyn_batch config.dat nPaths on|off [--kuka-model]
//
// --kuka-model hands the built-in KUKA table to BA::setSerialModel (a robot type without a table of its own).
// dump.bin: per path  int64 n, nTheta, nCart, nTrq; double sres; then theta[nTheta][n], cart[nCart][n], trq[nTrq][n].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba.h"
#include "batotp_hip.h"

using namespace BATOTP;

static void putRows(FILE *f, const std::vector<std::vector<double>> &rows, size_t count, size_t n)
{
   for (size_t j = 0; j < count; ++j) fwrite(rows[j].data(), sizeof(double), n, f);
}

int main(int argc, char *argv[])
{
   if (argc < 4) return 2;
   const int nPaths = atoi(argv[2]);
   const bool on = std::string(argv[3]) == "on";
   BA planner;
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   planner.setIsAutoIntegRes(false);
   if (planner.readConfigData((std::string("./") + argv[1]).c_str()) == -1) return 1;
   if (argc >= 5 && std::string(argv[4]) == "--kuka-model")
   {
      batotp_serial_model m;
      if (batotp_hip_builtin_serial_model(BATOTP_ROBOT_KUKA, &m) != 0) return 1;
      planner.setSerialModel(&m);
   }
   planner.setOutputTorques(on);
   planner.setAuditTolerance(0.05);
   std::vector<Traj> paths((size_t)nPaths);
   if (planner.loadTrajectoryData(paths[0]) == -1) return 1;
   for (int p = 1; p < nPaths; ++p) paths[p] = paths[0];
   const int rc = planner.optimizeBatch(paths);
   printf("optimizeBatch %d\n", rc);
   if (rc != 0) return 3;
   FILE *f = fopen("dump.bin", "wb");
   if (!f) return 1;
   const std::vector<BatchAudit> &audit = planner.getLastAudit();
   if (audit.size() != paths.size()) return 5;
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
      printf("trq_peak %zu %016llx %lld %d audited %d n_pts %lld trq_rows %zu\n", p, bits, audit[p].at[4], audit[p].row[4], (int)audit[p].audited,
             audit[p].nPts, t.trq.size());
   }
   fclose(f);
   return 0;
}
