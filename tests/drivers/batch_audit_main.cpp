// batch_audit_main.cpp -- BA::optimizeBatch with the audit on (BA::setAuditTolerance): prints BA::getLastAudit() of every path
// with the peaks as bit patterns, for tests/test_gpu_audit.py to compare with the C-ABI's audit of the same batch.
//
//   batch_audit config.dat nPaths tol [--all-devices]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba.h"

using namespace BATOTP;

int main(int argc, char *argv[])
{
   if (argc < 4) return 2;
   const int nPaths = atoi(argv[2]);
   const double tol = atof(argv[3]);
   BA planner;
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   planner.setIsAutoIntegRes(false);
   if (planner.readConfigData((std::string("./") + argv[1]).c_str()) == -1) return 1;
   if (argc >= 5 && std::string(argv[4]) == "--all-devices") planner.useAllDevices();
   if (!planner.getLastAudit().empty()) return 5; // off by default
   planner.setAuditTolerance(tol);
   std::vector<Traj> paths((size_t)nPaths);
   if (planner.loadTrajectoryData(paths[0]) == -1) return 1;
   for (int p = 1; p < nPaths; ++p) paths[p] = paths[0];
   std::vector<Traj> fresh = paths;
   if (planner.optimizeBatch(paths) != 0) return 3;
   const std::vector<BatchAudit> &audit = planner.getLastAudit();
   printf("paths %zu output_calls %d\n", audit.size(), planner.getLastOutputCalls());
   for (size_t p = 0; p < audit.size(); ++p)
   {
      const BatchAudit &a = audit[p];
      unsigned long long bits = 0;
      memcpy(&bits, &a.sres, sizeof(bits));
      printf("path %zu audited %d n_pts %lld n_over %lld n_nonfinite %lld sres %016llx\n", p, (int)a.audited, a.nPts, a.nOver, a.nNonfinite, bits);
      for (int f = 0; f < 5; ++f)
      {
         memcpy(&bits, &a.peak[f], sizeof(bits));
         printf("peak %zu %d %016llx %lld %d\n", p, f, bits, a.at[f], a.row[f]);
      }
   }
   planner.setAuditTolerance(-1.0); // off again: the next batch leaves no audit
   if (planner.optimizeBatch(fresh) != 0) return 3;
   if (!planner.getLastAudit().empty()) return 6;
   return 0;
}
