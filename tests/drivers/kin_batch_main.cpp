// kin_batch_main.cpp -- test driver (tests/test_gpu_kin_chain.py): BA::optimizeBatch on a joint path of a UR arm with
// Cartesian limits, the tool point from a kinematic chain (include/batotp_hip_kin.h).  Linked with the HIP library.
//
//   kin_batch_main config.dat <copies> [--tool]
//
// The configuration and its taught path are read from the current directory; the chain model is the built-in nominal UR5
// (include/batotp_models.h: axes and offsets; no inertial parameters are needed without torque limits).  With --tool the tool
// point of that table is set, every copy's files are written into ./out_<p>/ and the path is optimised once more, alone,
// through BA::optimize (files in ./out_single/); without it the configuration is one the device resampler does not cover,
// and optimizeBatch says so and returns -1.  Prints "optimizeBatch <return value>" and "optimize <return value>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba.h"
#include "batotp_hip.h"
#include "batotp_models.h"
#include "util.h"

using namespace BATOTP;

// the planner of config.dat in the current folder with the nominal UR5 chain model and, if asked, its tool point
static int setUp(BA &planner, const char *config, bool tool)
{
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   if (planner.readConfigData((std::string("./") + config).c_str()) == -1) return -1;
   batotp_kin_chain c;
   batotp_serial_model m;
   if (batotp_builtin_kin_chain(BATOTP_ROBOT_UR, &c) != 0) return -1;
   memset(&m, 0, sizeof(m));
   m.n_links = c.n_links;
   m.degrees = c.degrees;
   for (int i = 0; i < c.n_links; ++i)
      for (int j = 0; j < 3; ++j) { m.link[i].axis[j] = c.axis[i][j]; m.link[i].off[j] = c.off[i][j]; }
   planner.setSerialModel(&m);
   if (tool) planner.setToolPoint(c.tool);
   return 0;
}

int main(int argc, char *argv[])
{
   if (argc < 3) { fprintf(stderr, "usage: kin_batch_main config.dat <copies> [--tool]\n"); return 2; }
   const int copies = atoi(argv[2]);
   const bool tool = argc > 3 && std::string(argv[3]) == "--tool";
   BA planner;
   if (setUp(planner, argv[1], tool) != 0) return 1;
   std::vector<Traj> paths((size_t)copies);
   for (int p = 0; p < copies; ++p)
      if (planner.loadTrajectoryData(paths[(size_t)p]) == -1) return 1;
   const int rc = planner.optimizeBatch(paths);
   printf("\noptimizeBatch %d\n", rc);
   if (rc != 0) return rc < 0 ? 4 : 3;
   for (int p = 0; p < copies; ++p)
   {
      const std::string dir = "./out_" + std::to_string(p) + "/";
      mkDirIfNec(dir.c_str());
      planner.setOutputFolder(dir.c_str());
      planner.writeOutputData(paths[(size_t)p]);
      printf("path %d points %u T %.17g cart_rows %d\n", p, paths[(size_t)p].nPts, paths[(size_t)p].tTotalTraj, (int)paths[(size_t)p].cart.size());
   }
   // the same path alone through the step-by-step calls (BA::optimize: interpInputData, sweep, sweep, interpOutputData)
   BA alone;
   Traj t;
   if (setUp(alone, argv[1], tool) != 0 || alone.loadTrajectoryData(t) == -1) return 1;
   const int rcAlone = alone.optimize(t);
   printf("\noptimize %d\n", rcAlone);
   if (rcAlone != 0) return 5;
   mkDirIfNec("./out_single/");
   alone.setOutputFolder("./out_single/");
   alone.writeOutputData(t);
   return 0;
}
