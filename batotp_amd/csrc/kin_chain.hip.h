// kin_chain.hip.h -- the tool point of a serial arm from its kinematic chain (include/batotp_hip_kin.h has the definition;
// this project's own, the reference has no counterpart).  Used where the closed forms of resample.hip.h (fwdkin_point) are
// used, for robots that have none: after each pass of the resampler, before them when a Cartesian constraint is on, and at the
// output points.  The closed forms and their kernels keep their code; these kernels stand beside them.
// Included by batotp_hip.hip.  fp64, no contraction, the order of the header.  One lane per point.
#pragma once
#include "batotp_hip_kin.h"
#include "resample.hip.h"
#include "output.hip.h"

namespace bk
{

// Cartesian rows 0..2 of point i of a path from its joint rows: th / ca point at row 0 of the joint / Cartesian rows, both
// with row stride n; trig = this path's table [2 * n_links][n] (cos q_j rows, then sin q_j rows: kind 2 of hostTrigTables) or
// nullptr for the device libm.  The chain is a kernel argument: its entries are wavefront-uniform loads, the loop over the
// links carries three doubles.
__device__ __forceinline__ void chain_tool_point(const batotp_kin_chain &ch, const double *__restrict__ th, double *__restrict__ ca,
                                                 const double *__restrict__ trig, int64_t n, int64_t i)
{
   const int nL = ch.n_links;
   const double unit = ch.degrees ? KIN_DEG2RAD : 1.0;
   double p0 = ch.tool[0], p1 = ch.tool[1], p2 = ch.tool[2];
   for (int l = nL - 1; l >= 0; --l)
   {
      double c, s;
      if (trig) { c = trig[(int64_t)l * n + i]; s = trig[(int64_t)(nL + l) * n + i]; }
      else
      {
         const double q = unit * th[(int64_t)l * n + i];
         c = cos(q);
         s = sin(q);
      }
      const double a0 = ch.axis[l][0], a1 = ch.axis[l][1], a2 = ch.axis[l][2];
      const double d = (a0 * p0 + a1 * p1) + a2 * p2;
      const double x0 = a1 * p2 - a2 * p1, x1 = a2 * p0 - a0 * p2, x2 = a0 * p1 - a1 * p0;
      const double k = d * (1.0 - c);
      const double n0 = ch.off[l][0] + ((p0 * c + x0 * s) + a0 * k);
      const double n1 = ch.off[l][1] + ((p1 * c + x1 * s) + a1 * k);
      const double n2 = ch.off[l][2] + ((p2 * c + x2 * s) + a2 * k);
      p0 = n0; p1 = n1; p2 = n2;
   }
   ca[i] = p0; ca[n + i] = p1; ca[2 * n + i] = p2;
}

// the chain in k_rs_fwdkin's place: stage array x [C][n] per path, Cartesian rows nJ..nJ+2 from the joint rows
__global__ void k_rs_fwdkin_chain(RsParams P, batotp_kin_chain ch, const RsPath *__restrict__ paths, int B, double *__restrict__ x,
                                  const double *__restrict__ trig, int64_t total)
{
   const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= total) return;
   const int lo = rs_find_path(paths, B, g);
   const RsPath pp = paths[lo];
   const int i = (int)(g - pp.off), n = pp.n;
   if (i >= n || pp.status) return;
   double *__restrict__ xb = x + pp.off * P.C;
   chain_tool_point(ch, xb, xb + (int64_t)P.nJ * n, trig ? trig + pp.off * (2 * ch.n_links) : nullptr, n, i);
}

// the chain in k_out_fwdkin's place: stage array x [R][n1] per path of the output stage
__global__ void k_out_fwdkin_chain(OutParams P, batotp_kin_chain ch, const OutPath *__restrict__ paths, int K, double *__restrict__ x,
                                   const double *__restrict__ trig, int64_t total)
{
   const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
   if (g >= total) return;
   const OutPath op = paths[out_find_path(paths, K, g, 1)];
   const int i = (int)(g - op.off1), n1 = op.n1;
   if (i >= n1) return;
   double *__restrict__ xb = x + op.off1 * P.R;
   chain_tool_point(ch, xb, xb + (int64_t)P.nJ * n1, trig ? trig + op.off1 * (2 * ch.n_links) : nullptr, n1, i);
}

} // namespace bk
