// kin_chain_main.cpp -- test driver (tests/test_kin_chain_cpu.py): the host twin of the chain tool point
// (Robot::chainToolPoint, include/batotp_hip_kin.h) as hex floats, and the refusals of BA::exportResampleParams for a
// configuration without a tool point.  It is linked with the host library and ANY implementation of include/batotp_hip.h
// (the CPU checker): it names Robot and BA::exportResampleParams only, never BA::setToolPoint.
//
//   kin_chain_main points <file>     the file holds any number of records
//        builtin <KUKA|RR|UR> <npts>            | chain <n_links> <degrees> <npts>
//        <n_links rows of npts joint values>    | <n_links rows: axis(3) off(3)>  <tool(3)>  <n_links rows of npts joint values>
//      (numbers in any form strtod reads, hex floats included); prints per record "points <npts>" and three rows of %a values
//   kin_chain_main refusals          prints "<case> <return value of exportResampleParams>" per case
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ba.h"
#include "batotp_hip.h"
#include "batotp_models.h"

using namespace BATOTP;

static bool readDouble(std::istream &in, double &v)
{
   std::string w;
   if (!(in >> w)) return false;
   char *end = nullptr;
   v = strtod(w.c_str(), &end);
   return end && *end == 0;
}

static void modelOfChain(const batotp_kin_chain &c, batotp_serial_model &m)
{
   memset(&m, 0, sizeof(m));
   m.n_links = c.n_links;
   m.degrees = c.degrees;
   for (int i = 0; i < c.n_links; ++i)
      for (int j = 0; j < 3; ++j) { m.link[i].axis[j] = c.axis[i][j]; m.link[i].off[j] = c.off[i][j]; }
}

static int points(const char *file)
{
   std::ifstream in(file);
   if (!in) { fprintf(stderr, "cannot open %s\n", file); return 2; }
   std::string kind;
   while (in >> kind)
   {
      batotp_kin_chain c;
      memset(&c, 0, sizeof(c));
      int npts = 0;
      if (kind == "builtin")
      {
         std::string name;
         in >> name >> npts;
         const int id = name == "KUKA" ? BATOTP_ROBOT_KUKA : (name == "RR" ? BATOTP_ROBOT_RR : (name == "UR" ? BATOTP_ROBOT_UR : 0));
         if (batotp_builtin_kin_chain(id, &c) != 0) { fprintf(stderr, "no built-in chain %s\n", name.c_str()); return 2; }
      }
      else if (kind == "chain")
      {
         in >> c.n_links >> c.degrees >> npts;
         if (c.n_links < 1 || c.n_links > BATOTP_MAX_LINKS) return 2;
         for (int i = 0; i < c.n_links; ++i)
         {
            for (int j = 0; j < 3; ++j) if (!readDouble(in, c.axis[i][j])) return 2;
            for (int j = 0; j < 3; ++j) if (!readDouble(in, c.off[i][j])) return 2;
         }
         for (int j = 0; j < 3; ++j) if (!readDouble(in, c.tool[j])) return 2;
      }
      else return 2;
      Robot::Channels theta((size_t)c.n_links, std::vector<double>((size_t)npts)), cart;
      for (int i = 0; i < c.n_links; ++i)
         for (int k = 0; k < npts; ++k) if (!readDouble(in, theta[(size_t)i][(size_t)k])) return 2;
      Robot robot;
      robot.call_set_robotType("GENJNT");
      batotp_serial_model m;
      modelOfChain(c, m);
      robot.setSerialModel(m);
      robot.setToolPoint(c.tool);
      // through the public dispatcher: a robot without a closed form, with a model and a tool point
      if (robot.call_fwdKin(theta, cart) != 0) return 3;
      printf("points %d\n", npts);
      for (int r = 0; r < 3; ++r)
      {
         for (int k = 0; k < npts; ++k) printf("%a ", cart[(size_t)r][(size_t)k]);
         printf("\n");
      }
   }
   return 0;
}

static int refusals()
{
   struct Case { const char *name, *robot; bool cartVel, model; } cases[] = {
      {"GENJNT_cartvel", "GENJNT", true, false},
      {"GENJNT_cartvel_model_only", "GENJNT", true, true},
      {"GENJNT_plain", "GENJNT", false, false},
      {"UR_joint", "UR", false, false},
      {"UR_joint_cartvel", "UR", true, false},
      {"UR_joint_model_only", "UR", true, true},
   };
   for (const Case &cs : cases)
   {
      BA::Config conf;
      conf.robotTypeStr = cs.robot;
      conf.pathType = "JOINT";
      conf.nJoints = 6;
      conf.nCart = 3;
      conf.isCartVelConOn = cs.cartVel;
      conf.isCarAccConOn = false;
      BA ba;
      if (ba.loadConfigData(conf) != 0) return 3;
      if (cs.model)
      {
         batotp_kin_chain c;
         batotp_serial_model m;
         batotp_builtin_kin_chain(BATOTP_ROBOT_UR, &c);
         modelOfChain(c, m);
         ba.setSerialModel(&m);
      }
      Traj t;
      t.nPts = 10;
      batotp_resample_params R;
      printf("%s %d\n", cs.name, ba.exportResampleParams(t, &R));
   }
   // ... and the dispatcher of the robot itself: no model or no tool point, no kinematics
   Robot robot;
   robot.call_set_robotType("UR");
   Robot::Channels theta(6, std::vector<double>(2, 0.0)), cart;
   printf("UR_call_fwdKin %d\n", robot.call_fwdKin(theta, cart));
   return 0;
}

int main(int argc, char **argv)
{
   if (argc >= 3 && std::string(argv[1]) == "points") return points(argv[2]);
   if (argc >= 2 && std::string(argv[1]) == "refusals") return refusals();
   fprintf(stderr, "usage: kin_chain_main points <file> | refusals\n");
   return 2;
}
