// batest_batch_main.cpp -- command-line driver of the many-path extension BA::optimizeBatch().
//
//   batest_batch config.dat nPaths [--auto-integ-res] [--devices N | --all-devices] [--audit [tol]] [--torques] [--stretch [target]]
//                [--stretch-torques [target]] [--stretch-duty R1,R2,... [target]]
//
// --audit [tol] (builds with -DBATOTP_HAVE_AUDIT, i.e. the product's): the finished trajectories are audited against the
// limits on the device (BA::setAuditTolerance, include/batotp_hip_audit.h; tol defaults to 0) and one summary line names
// the worst peak of every family with its path and time, and the paths with points over 1 + tol.  Exit status 4 if a
// trajectory holds a value that is not finite.
// --torques (builds with -DBATOTP_HAVE_INVDYN, i.e. the product's): paths planned without torque limits get torque rows from the
// inverse dynamics of the chain model along the finished samples (BA::setOutputTorques, include/batotp_hip_invdyn.h); with
// --audit one more line per path gives the peak utilisation of the configuration's torque range.
// --stretch [target] (builds with -DBATOTP_HAVE_STRETCH, i.e. the product's): the finished trajectories are stretched in time, each by
// its own factor, until their velocity and acceleration peaks are within target (BA::setStretchToLimits,
// include/batotp_hip_stretch.h; target defaults to 1) -- before --torques and --audit, which then see the stretched samples.  One
// summary line: paths stretched, largest factor, paths not passing, paths skipped.
// --stretch-torques [target] (builds with -DBATOTP_HAVE_TSCALE, i.e. the product's): the finished trajectories are stretched until
// the torques of the chain model along them are within target of the configuration's torque range too
// (BA::setStretchToTorqueLimits, include/batotp_hip_tscale.h; target defaults to 1), and carry those torque rows.  One summary
// line: paths stretched, largest factor, paths not passing, of those the paths no stretch can help; with --audit one more line per
// path gives the peak utilisation of the torque range.
// --stretch-duty R1,R2,... [target] (builds with -DBATOTP_HAVE_DUTY, i.e. the product's): as --stretch-torques, and until the RMS
// torque of every joint is within target of its continuous torque R1, R2, ... too (BA::setStretchToRatedTorques,
// include/batotp_hip_duty.h; one rating per joint; target defaults to 1).  One summary line, and per path its utilisation of the
// ratings with the joint, its energy and its peak power.
// --auto-integ-res leaves BA's class default on (reference ba.h:309; the reference's own driver switches it off,
// test/main.cpp:53): every path then integrates with the step the rule of ba.cpp:493-556 derives from it.
// (--host-resample / --host-output are accepted and ignored: since round 4 both stages always run behind the C-ABI.)
//
// Loads the trajectory named by the configuration nPaths times, optimises all copies as one device
// batch and writes, for the first and the last path, the same files the single-path driver writes
// (traj_out.dat / s-sdot.dat) into ./out_first/ and ./out_last/.  Configuration, input and
// outputs live in the current directory.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ba.h"
#include "util.h"

using namespace BATOTP;

int main(int argc, char *argv[])
{
   if (argc < 3)
   {
      fprintf(stderr, "usage: batest_batch config.dat nPaths [--auto-integ-res] [--devices N | --all-devices] [--audit [tol]] [--torques] [--stretch [target]] [--stretch-torques [target]] [--stretch-duty R1,R2,... [target]]\n");
      return 2;
   }
   const int nPaths = atoi(argv[2]);
   if (nPaths < 1) return 2;
   bool hostResample = false, hostOutput = false, allDevices = false, autoIntegRes = false;
   int nDevices = 0;
#ifdef BATOTP_HAVE_AUDIT
   double auditTol = -1;
#endif
#ifdef BATOTP_HAVE_INVDYN
   bool torques = false;
#endif
#ifdef BATOTP_HAVE_STRETCH
   double stretchTarget = 0;
#endif
#ifdef BATOTP_HAVE_TSCALE
   double tscaleTarget = 0;
#endif
#ifdef BATOTP_HAVE_DUTY
   double dutyTarget = 0;
   std::vector<double> dutyRated;
#endif
   for (int k = 3; k < argc; ++k)
   {
#ifdef BATOTP_HAVE_DUTY
      if (std::string(argv[k]) == "--stretch-duty" && k + 1 < argc)
      {
         dutyTarget = 1;
         for (const char *at = argv[++k]; *at;)
         {
            char *end = nullptr;
            dutyRated.push_back(strtod(at, &end));
            if (end == at) { fprintf(stderr, "--stretch-duty: '%s' is not a list of ratings\n", argv[k]); return 2; }
            at = *end == ',' ? end + 1 : end;
         }
         char *end = nullptr;
         if (k + 1 < argc)
         {
            const double v = strtod(argv[k + 1], &end);
            if (end != argv[k + 1] && *end == 0 && v > 0 && v <= 1) { dutyTarget = v; ++k; }
         }
         continue;
      }
#endif
#ifdef BATOTP_HAVE_TSCALE
      if (std::string(argv[k]) == "--stretch-torques")
      {
         tscaleTarget = 1;
         char *end = nullptr;
         if (k + 1 < argc)
         {
            const double v = strtod(argv[k + 1], &end);
            if (end != argv[k + 1] && *end == 0 && v > 0 && v <= 1) { tscaleTarget = v; ++k; }
         }
         continue;
      }
#endif
#ifdef BATOTP_HAVE_INVDYN
      if (std::string(argv[k]) == "--torques") torques = true;
#endif
#ifdef BATOTP_HAVE_AUDIT
      if (std::string(argv[k]) == "--audit")
      {
         auditTol = 0;
         char *end = nullptr;
         if (k + 1 < argc)
         {
            const double v = strtod(argv[k + 1], &end);
            if (end != argv[k + 1] && *end == 0 && v >= 0) { auditTol = v; ++k; }
         }
         continue;
      }
#endif
#ifdef BATOTP_HAVE_STRETCH
      if (std::string(argv[k]) == "--stretch")
      {
         stretchTarget = 1;
         char *end = nullptr;
         if (k + 1 < argc)
         {
            const double v = strtod(argv[k + 1], &end);
            if (end != argv[k + 1] && *end == 0 && v > 0 && v <= 1) { stretchTarget = v; ++k; }
         }
         continue;
      }
#endif
      if (std::string(argv[k]) == "--host-resample") hostResample = true;
      if (std::string(argv[k]) == "--host-output") hostOutput = true;
      if (std::string(argv[k]) == "--all-devices") allDevices = true;
      if (std::string(argv[k]) == "--auto-integ-res") autoIntegRes = true;
      if (std::string(argv[k]) == "--devices" && k + 1 < argc) nDevices = atoi(argv[++k]);
   }

   BA planner;
   planner.setHomeFolder("./");
   planner.setInputFolder("./");
   planner.setOutputFolder("./");
   planner.setIsAutoIntegRes(autoIntegRes);
   planner.setDeviceResample(!hostResample);
   planner.setDeviceOutput(!hostOutput);
   if (planner.readConfigData((std::string("./") + argv[1]).c_str()) == -1) return 1;
#ifdef BATOTP_HAVE_AUDIT
   planner.setAuditTolerance(auditTol);
#endif
#ifdef BATOTP_HAVE_INVDYN
   planner.setOutputTorques(torques);
#endif
#ifdef BATOTP_HAVE_STRETCH
   planner.setStretchToLimits(stretchTarget);
#endif
#ifdef BATOTP_HAVE_TSCALE
   planner.setStretchToTorqueLimits(tscaleTarget);
#endif
#ifdef BATOTP_HAVE_DUTY
   planner.setStretchToRatedTorques(dutyRated, dutyTarget);
#endif
   if (allDevices) nDevices = planner.useAllDevices();
   else if (nDevices > 0)
   {
      std::vector<int> devices((size_t)nDevices);
      for (int d = 0; d < nDevices; ++d) devices[d] = d;
      planner.setDevices(devices);
   }

   std::vector<Traj> paths(nPaths);
   if (planner.loadTrajectoryData(paths[0]) == -1) return 1;
   for (int p = 1; p < nPaths; ++p) paths[p] = paths[0];

   const Time t0 = getTime();
   const int failed = planner.optimizeBatch(paths);
   const Time t1 = getTime();
   if (nDevices > 1) printf("\noptimizeBatch: paths sharded over %d devices\n", nDevices);
   printf("\noptimizeBatch: %d paths, %d failed, %.3f s (resampling %s: %.3f ms; output stage %s: %.3f ms, kernels %.3f ms)\n", nPaths, failed,
          diffTime(t1, t0), "device", planner.getLastResampleMs(), "device",
          planner.getLastOutputMs(), planner.getLastOutputKernelMs());
   if (failed < 0 || failed == nPaths) return 1;
   bool nonfinite = false;
#ifdef BATOTP_HAVE_STRETCH
   if (stretchTarget > 0)
   {
      const std::vector<BatchStretch> &st = planner.getLastStretch();
      int nStretched = 0, nNotPassing = 0, nSkipped = 0, worst = -1;
      for (size_t p = 0; p < st.size(); ++p)
      {
         if (st[p].skipped) ++nSkipped;
         if (!st[p].done) continue;
         if (st[p].nOut > st[p].nIn) ++nStretched;
         if (st[p].status != 0) ++nNotPassing;
         if (worst < 0 || st[p].factor > st[worst].factor) worst = (int)p;
      }
      printf("stretch (target %g): %d of %d paths stretched, largest factor %.6f (path %d), %d not passing, %d skipped\n", stretchTarget, nStretched,
             (int)st.size(), worst < 0 ? 1.0 : st[worst].factor, worst, nNotPassing, nSkipped);
   }
#endif
#ifdef BATOTP_HAVE_TSCALE
   if (tscaleTarget > 0)
   {
      const std::vector<BatchStretch> &st = planner.getLastStretch();
      int nDone = 0, nStretched = 0, nNotPassing = 0, nStatic = 0, worst = -1;
      for (size_t p = 0; p < st.size(); ++p)
      {
         if (!st[p].done) continue;
         ++nDone;
         if (st[p].nOut > st[p].nIn) ++nStretched;
         if (st[p].status != 0) ++nNotPassing;
         if (st[p].status == 3) ++nStatic;
         if (worst < 0 || st[p].factor > st[worst].factor) worst = (int)p;
      }
      if (nDone == 0) printf("stretch-torques (target %g): not applied (it needs a serial robot planned without torque limits, a chain model and a torque range)\n", tscaleTarget);
      else
         printf("stretch-torques (target %g): %d of %d paths stretched, largest factor %.6f (path %d), %d not passing, %d of them static\n", tscaleTarget,
                nStretched, (int)st.size(), st[worst].factor, worst, nNotPassing, nStatic);
   }
#endif
#ifdef BATOTP_HAVE_DUTY
   if (dutyTarget > 0)
   {
      const std::vector<BatchStretch> &st = planner.getLastStretch();
      const std::vector<BatchDuty> &du = planner.getLastDuty();
      int nDone = 0, nStretched = 0, nNotPassing = 0, nStatic = 0, worst = -1;
      for (size_t p = 0; p < st.size() && p < du.size(); ++p)
      {
         if (!st[p].done || !du[p].done) continue;
         ++nDone;
         if (st[p].nOut > st[p].nIn) ++nStretched;
         if (st[p].status != 0) ++nNotPassing;
         if (st[p].status == 3) ++nStatic;
         if (worst < 0 || st[p].factor > st[worst].factor) worst = (int)p;
      }
      if (nDone == 0)
         printf("stretch-duty (target %g): not applied (it needs a serial robot planned without torque limits, a chain model, a torque range and a rating per joint)\n",
                dutyTarget);
      else
      {
         printf("stretch-duty (target %g): %d of %d paths stretched, largest factor %.6f (path %d), %d not passing, %d of them static\n", dutyTarget, nStretched,
                (int)st.size(), st[worst].factor, worst, nNotPassing, nStatic);
         for (size_t p = 0; p < du.size(); ++p)
            if (du[p].done)
               printf("duty: path %d util %.6g (joint %d) energy %.6f peak_power %.6f (point %lld of %lld)\n", (int)p, du[p].util, du[p].row, du[p].energy,
                      du[p].peakPower, du[p].powerAt, du[p].nPts);
      }
   }
#endif
#ifdef BATOTP_HAVE_AUDIT
   if (auditTol >= 0)
   {
      static const char *const family[5] = {"jnt_vel", "jnt_acc", "cart_vel", "cart_acc", "trq"};
      const std::vector<BatchAudit> &audit = planner.getLastAudit();
      printf("audit (tol %g):", auditTol);
      for (int f = 0; f < 5; ++f)
      {
         int worst = -1;
         for (size_t p = 0; p < audit.size(); ++p)
            if (audit[p].audited && audit[p].peak[f] >= 0 && (worst < 0 || audit[p].peak[f] > audit[worst].peak[f])) worst = (int)p;
         if (worst < 0) printf(" %s -", family[f]);
         else printf(" %s %.6f (path %d, t %.6f s, row %d)", family[f], audit[worst].peak[f], worst, (double)audit[worst].at[f] * audit[worst].sres, audit[worst].row[f]);
      }
      printf("; over:");
      int nOverPaths = 0;
      for (size_t p = 0; p < audit.size(); ++p)
      {
         if (audit[p].nOver > 0) { printf(" %d(%lld)", (int)p, audit[p].nOver); ++nOverPaths; }
         if (audit[p].nNonfinite > 0) nonfinite = true;
      }
      printf(nOverPaths ? "\n" : " none\n");
      if (nonfinite) printf("audit: a trajectory holds values that are not finite\n");
#ifdef BATOTP_HAVE_INVDYN
      bool trqLines = torques;
#ifdef BATOTP_HAVE_TSCALE
      trqLines = trqLines || tscaleTarget > 0;
#endif
#ifdef BATOTP_HAVE_DUTY
      trqLines = trqLines || dutyTarget > 0;
#endif
      if (trqLines)
         for (size_t p = 0; p < audit.size(); ++p)
         {
            if (!audit[p].audited) printf("torques: path %d not audited\n", (int)p);
            else if (audit[p].peak[4] < 0) printf("torques: path %d trq -\n", (int)p);
            else printf("torques: path %d trq %.6f (t %.6f s, row %d)\n", (int)p, audit[p].peak[4], (double)audit[p].at[4] * audit[p].sres, audit[p].row[4]);
         }
#endif
   }
#endif

   const char *dirs[2] = {"./out_first/", "./out_last/"};
   const int which[2] = {0, nPaths - 1};
   for (int k = 0; k < 2; ++k)
   {
      mkDirIfNec(dirs[k]);
      planner.setOutputFolder(dirs[k]);
      planner.writeOutputData(paths[which[k]]);
   }
   if (nonfinite) return 4;
   return failed == 0 ? 0 : 3;
}
