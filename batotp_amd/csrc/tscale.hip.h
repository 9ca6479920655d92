// tscale.hip.h -- kernels of batotp_hip_output_torque_scale / _stretch_torques (include/batotp_hip_tscale.h has the definition they implement).
//
// k_tscale          the grid and the lanes of k_invdyn, and its point: invdyn_point (invdyn.hip.h) copies the joint and Cartesian rows,
//                   writes the torque rows and hands back t2, fv qd and t4, from which the two candidates of every joint are formed in
//                   unrolled loops: no per-lane array is added to those of k_invdyn.  A lane keeps ONE candidate (x, point, joint, side)
//                   and one static flag; the workgroup reduces them in-wave (__shfl_down) and then through LDS to one partial per block.
//                   Lanes past the end of the path take part in the reduction with "no candidate", so no lane leaves before the barrier.
// k_tscale_finish   one wavefront per path reduces the path's partials into its batotp_path_tscale.
//
// The audit's discipline (audit.hip.h): candidates under the total order "x ascending, point ascending, joint ascending, upper side
// before lower", integer counts, no floating-point atomics, nothing depends on the order of arrival: the same bits for any grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batotp_hip_tscale.h"
#include "invdyn.hip.h"

namespace bk
{

constexpr int TSCALE_BP = BATOTP_TSCALE_BLOCK_POINTS;
constexpr int TSCALE_THREADS = TSCALE_BP; // one lane per point
static_assert(TSCALE_THREADS % 64 == 0, "whole wavefronts");
static_assert(TSCALE_BP == INVDYN_BP, "the blocks of k_invdyn_pack and the lanes of invdyn_stage_model");

// bounds of the call (kernel argument), formed on the host
struct TscaleConst
{
   double hi[BATOTP_MAX_LINKS], lo[BATOTP_MAX_LINKS];
};

struct TscalePath
{
   InvdynPath p; // first: k_invdyn_pack reads a table of these with their stride
   int64_t pOff; // first partial of the path in its range; block blk of the path writes partial pOff + blk
};

struct TscalePartial
{
   double x;
   long long at;
   int row, side;
   long long nStatic;
};

// "no candidate" is (+Inf, -1, -1, 0): every candidate has a finite x and is ahead of it
struct TscaleBest
{
   double x;
   long long a;
   int r, sd;
   __device__ __forceinline__ void none() { x = __builtin_inf(); a = -1; r = -1; sd = 0; }
   __device__ __forceinline__ void merge(double ox, long long oa, int orow, int osd)
   {
      if (ox < x || (ox == x && (oa < a || (oa == a && (orow < r || (orow == r && osd > sd)))))) { x = ox; a = oa; r = orow; sd = osd; }
   }
   // the candidate of a x^2 + b x + c, c < 0, at (point, joint, side)
   __device__ __forceinline__ void offer(double ca, double cb, double cc, long long at, int row, int side)
   {
      const double disc = cb * cb - (4.0 * ca) * cc;
      const double q = cb + sqrt(disc);
      const double rx = (2.0 * (-cc)) / q;
      if (disc >= 0.0 && q > 0.0 && q <= 1.7976931348623157e308 && rx <= 1.7976931348623157e308) merge(rx, at, row, side);
   }
   __device__ __forceinline__ void waveReduce()
   {
      for (int d = 32; d >= 1; d >>= 1)
      {
         const double ox = __shfl_down(x, d);
         const long long oa = __shfl_down(a, d);
         const int orow = __shfl_down(r, d);
         const int osd = __shfl_down(sd, d);
         merge(ox, oa, orow, osd);
      }
   }
};

__device__ __forceinline__ long long tscale_wave_sum(long long v)
{
   for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d);
   return v;
}

__global__ __launch_bounds__(TSCALE_THREADS) void k_tscale(const batotp_serial_model *__restrict__ model, TscaleConst C, const TscalePath *__restrict__ paths,
                                                           const PathBlock *__restrict__ blocks, int nBlocks, const double *__restrict__ src, int nCart,
                                                           const double *__restrict__ trig, double *__restrict__ dst, TscalePartial *__restrict__ partials)
{
   constexpr int NW = TSCALE_THREADS / 64;
   __shared__ batotp_serial_model sm;
   __shared__ double redX[NW];
   __shared__ long long redA[NW], redN[NW];
   __shared__ int redR[NW], redS[NW];
   invdyn_stage_model(model, sm);
   __syncthreads();
   if ((int)blockIdx.x >= nBlocks) return; // the whole workgroup
   const PathBlock bd = blocks[blockIdx.x];
   const TscalePath pd = paths[bd.path];
   const int64_t i = (int64_t)bd.blk * TSCALE_BP + (int)threadIdx.x;

   TscaleBest best;
   best.none();
   long long nStatic = 0;
   if (i < pd.p.n)
   {
      const int nl = sm.n_links;
      double t2[BATOTP_MAX_LINKS], fvq[BATOTP_MAX_LINKS], t4[BATOTP_MAX_LINKS];
      invdyn_point(sm, pd.p, i, src, nCart, trig, dst, t2, fvq, t4);
      bool isStatic = false;
#pragma unroll
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
         if (j < nl && !(t4[j] - C.hi[j] < 0.0 && C.lo[j] - t4[j] < 0.0)) isStatic = true;
      nStatic = isStatic ? 1 : 0;
      if (!isStatic)
      {
#pragma unroll
         for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
            if (j < nl)
            {
               const double A = t2[j], B = fvq[j], G = t4[j];
               best.offer(A, B, G - C.hi[j], i, j, +1);
               best.offer(-A, -B, C.lo[j] - G, i, j, -1);
            }
      }
   }

   // workgroup reduction: in-wave, then through LDS
   const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
   nStatic = tscale_wave_sum(nStatic);
   best.waveReduce();
   if (lane == 0) { redX[wave] = best.x; redA[wave] = best.a; redR[wave] = best.r; redS[wave] = best.sd; redN[wave] = nStatic; }
   __syncthreads();
   if (threadIdx.x == 0)
   {
      long long ns = redN[0];
      for (int w = 1; w < NW; ++w) { best.merge(redX[w], redA[w], redR[w], redS[w]); ns += redN[w]; }
      TscalePartial *out = partials + (pd.pOff + bd.blk);
      out->x = best.x; out->at = best.a; out->row = best.r; out->side = best.sd; out->nStatic = ns;
   }
}

// one wavefront per path of the range
__global__ __launch_bounds__(64) void k_tscale_finish(const TscalePath *__restrict__ paths, int nPaths, const TscalePartial *__restrict__ partials,
                                                      batotp_path_tscale *__restrict__ out)
{
   const int k = (int)blockIdx.x;
   if (k >= nPaths) return;
   const TscalePath pd = paths[k];
   const int lane = (int)threadIdx.x;
   const int64_t nblk = (pd.p.n + TSCALE_BP - 1) / TSCALE_BP;
   TscaleBest best;
   best.none();
   long long ns = 0;
   for (int64_t b = lane; b < nblk; b += 64)
   {
      const TscalePartial *p = partials + (pd.pOff + b);
      best.merge(p->x, p->at, p->row, p->side);
      ns += p->nStatic;
   }
   ns = tscale_wave_sum(ns);
   best.waveReduce();
   if (lane == 0)
   {
      batotp_path_tscale *o = out + k;
      o->s = best.x; o->at = best.a; o->row = best.r; o->side = best.sd; o->n_static = ns; o->reserved = 0;
   }
}

} // namespace bk
