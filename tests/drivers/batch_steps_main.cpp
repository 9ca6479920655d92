// batch_steps_main.cpp -- test driver (tests/test_batch_output_steps.py): several taught paths, each with a configuration
// file of its own in the current directory, optimised as ONE batch with the automatic integration resolution on.
//
//   batch_steps_main config_0.dat config_1.dat ...
//
// Prints, for every path, the integration step the rule derives for it ("step <p> <%.17g>", from a planner of its own that
// only resamples that path) and the number of batotp_hip_output calls the batch took ("output_calls <n>"), then writes
// every path's files (traj_out.dat, s-sdot.dat) into ./out_<p>/.
#include <cstdio>
#include <string>
#include <vector>

#include "ba.h"
#include "batotp_hip.h"
#include "util.h"

using namespace BATOTP;

static void inCurrentFolder(BA &planner)
{
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   planner.setIsAutoIntegRes(true);
}

int main(int argc, char *argv[])
{
   if (argc < 2)
   {
      fprintf(stderr, "usage: batch_steps_main config_0.dat [config_1.dat ...]\n");
      return 2;
   }
   const int nPaths = argc - 1;
   std::vector<double> step((size_t)nPaths, 0.0);
   for (int p = 0; p < nPaths; ++p)
   {
      BA probe;
      Traj t;
      inCurrentFolder(probe);
      if (probe.readConfigData((std::string("./") + argv[1 + p]).c_str()) == -1) return 1;
      if (probe.loadTrajectoryData(t) == -1) return 1;
      if (probe.interpInputData(t) == -1) return 1;
      batotp_output_params O;
      probe.exportOutputParams(&O); // (the return value says whether the device stage covers the configuration; the step is filled either way)
      step[(size_t)p] = O.integ_res;
   }

   BA planner;
   inCurrentFolder(planner);
   std::vector<Traj> paths((size_t)nPaths);
   for (int p = 0; p < nPaths; ++p)
   {
      if (planner.readConfigData((std::string("./") + argv[1 + p]).c_str()) == -1) return 1;
      if (planner.loadTrajectoryData(paths[(size_t)p]) == -1) return 1;
   }
   const int failed = planner.optimizeBatch(paths);
   printf("\n");
   for (int p = 0; p < nPaths; ++p) printf("step %d %.17g\n", p, step[(size_t)p]);
   printf("output_calls %d\n", planner.getLastOutputCalls());
   printf("failed %d\n", failed);
   if (failed != 0) return 3;
   for (int p = 0; p < nPaths; ++p)
   {
      const std::string dir = "./out_" + std::to_string(p) + "/";
      mkDirIfNec(dir.c_str());
      planner.setOutputFolder(dir.c_str());
      planner.writeOutputData(paths[(size_t)p]);
   }
   return 0;
}
