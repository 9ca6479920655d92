// tscale.hip.h -- kernels of batotp_hip_output_torque_scale / _stretch_torques (include/batotp_hip_tscale.h has the definition they implement).
//
// k_tscale          the shape of k_invdyn (invdyn.hip.h): one workgroup of TSCALE_THREADS lanes per block of BATOTP_TSCALE_BLOCK_POINTS
//                   points of ONE path, one lane per point, a host-built table of (path, block) descriptors, the chain model staged in
//                   LDS, the two passes of rnea_pass (kernels.hip.h) unchanged.  It copies the joint and Cartesian rows and writes the
//                   torque rows (t2 + fv qd) + t4 -- the expression of k_invdyn, hence its bits -- and, from the same t2, fv qd and t4,
//                   forms the two candidates of every joint in unrolled loops: no per-lane array is added to those of k_invdyn.  A lane
//                   keeps ONE candidate (x, point, joint, side) and one static flag; the workgroup reduces them in-wave (__shfl_down)
//                   and then through LDS to one partial per block.  Lanes past the end of the path take part in the reduction with
//                   "no candidate", so no lane leaves before the barrier.
// k_tscale_finish   one wavefront per path reduces the path's partials into its batotp_path_tscale.
//
// The audit's discipline (audit.hip.h): candidates under the total order "x ascending, point ascending, joint ascending, upper side
// before lower", integer counts, no floating-point atomics, nothing depends on the order of arrival: the same bits for any grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batotp_hip_tscale.h"
#include "kernels.hip.h"

namespace bk
{

constexpr int TSCALE_BP = BATOTP_TSCALE_BLOCK_POINTS;
constexpr int TSCALE_THREADS = TSCALE_BP; // one lane per point
static_assert(TSCALE_THREADS % 64 == 0, "whole wavefronts");

// bounds of the call (kernel argument), formed on the host
struct TscaleConst
{
   double hi[BATOTP_MAX_LINKS], lo[BATOTP_MAX_LINKS];
};

struct TscalePath
{
   int64_t off;   // first point of the path in the rows of the source and of the result (points)
   int64_t n;     // points
   int64_t tOff;  // first point of the path in the packed joint rows / trig tables of its range
   int64_t pOff;  // first partial of the path in its range
   double c1, c2; // 1 / (2 h), 1 / (h h)
};

struct TscaleBlock
{
   int32_t path, blk; // points [blk * TSCALE_BP, (blk + 1) * TSCALE_BP) of the path (path: index into the range's descriptors); partial pOff + blk
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

// joint rows of an output with Cartesian rows, packed [n_links][n] per path for the host trig tables (as k_invdyn_pack, on this
// header's descriptors)
__global__ __launch_bounds__(TSCALE_THREADS) void k_tscale_pack(const TscalePath *__restrict__ paths, const TscaleBlock *__restrict__ blocks, int nBlocks,
                                                                const double *__restrict__ src, int nl, int nCart, double *__restrict__ pack)
{
   if ((int)blockIdx.x >= nBlocks) return;
   const TscaleBlock bd = blocks[blockIdx.x];
   const TscalePath pd = paths[bd.path];
   const int64_t n = pd.n, i = (int64_t)bd.blk * TSCALE_BP + (int)threadIdx.x;
   if (i >= n) return;
   const double *sb = src + pd.off * (nl + nCart);
   double *pb = pack + pd.tOff * nl;
   for (int j = 0; j < nl; ++j) pb[(int64_t)j * n + i] = sb[(int64_t)j * n + i];
}

__global__ __launch_bounds__(TSCALE_THREADS) void k_tscale(const batotp_serial_model *__restrict__ model, TscaleConst C, const TscalePath *__restrict__ paths,
                                                           const TscaleBlock *__restrict__ blocks, int nBlocks, const double *__restrict__ src, int nCart,
                                                           const double *__restrict__ trig, double *__restrict__ dst, TscalePartial *__restrict__ partials)
{
   constexpr int NW = TSCALE_THREADS / 64;
   __shared__ batotp_serial_model sm;
   __shared__ double redX[NW];
   __shared__ long long redA[NW], redN[NW];
   __shared__ int redR[NW], redS[NW];
   {
      // cooperative copy of the table (8-byte words)
      const double *from = reinterpret_cast<const double *>(model);
      double *to = reinterpret_cast<double *>(&sm);
      for (int k = threadIdx.x; k < (int)(sizeof(batotp_serial_model) / 8); k += TSCALE_THREADS) to[k] = from[k];
   }
   __syncthreads();
   if ((int)blockIdx.x >= nBlocks) return; // the whole workgroup
   const TscaleBlock bd = blocks[blockIdx.x];
   const TscalePath pd = paths[bd.path];
   const int64_t n = pd.n, i = (int64_t)bd.blk * TSCALE_BP + (int)threadIdx.x;

   TscaleBest best;
   best.none();
   long long nStatic = 0;
   if (i < n)
   {
      const int nl = sm.n_links, R = nl + nCart;
      const double *__restrict__ sb = src + pd.off * R;
      double *__restrict__ db = dst + pd.off * (R + nl);
      const double *__restrict__ tg = trig ? trig + pd.tOff * 2 * nl : nullptr;
      const double kDeg2Rad = 3.14159265358979323846 / 180.0;
      const double unit = sm.degrees ? kDeg2Rad : 1.0;
      // the end points take the differences of their interior neighbour; fewer than three points: none
      const bool diff = n >= 3;
      const int64_t ic = i < 1 ? 1 : (i > n - 2 ? n - 2 : i);
      const double c1 = pd.c1, c2 = pd.c2;

      double cq[BATOTP_MAX_LINKS], sq[BATOTP_MAX_LINKS], q1[BATOTP_MAX_LINKS], q2[BATOTP_MAX_LINKS], z[BATOTP_MAX_LINKS];
#pragma unroll
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
      {
         cq[j] = 1; sq[j] = 0; q1[j] = 0; q2[j] = 0; z[j] = 0;
         if (j < nl)
         {
            const double *__restrict__ x = sb + (int64_t)j * n;
            const double xi = x[i];
            db[(int64_t)j * n + i] = xi;
            double v = 0.0, a = 0.0;
            if (diff)
            {
               const double xm = x[ic - 1], x0 = x[ic], xp = x[ic + 1];
               v = (xp - xm) * c1;
               a = ((xp - x0) - (x0 - xm)) * c2;
            }
            const double q = unit * xi;
            q1[j] = unit * v;
            q2[j] = unit * a;
            if (tg) { cq[j] = tg[(int64_t)j * n + i]; sq[j] = tg[(int64_t)(nl + j) * n + i]; }
            else { cq[j] = cos(q); sq[j] = sin(q); } // device libm: not bit-identical to glibc (BATOTP_F_HOST_TRIG)
         }
      }
      for (int r = nl; r < R; ++r) db[(int64_t)r * n + i] = sb[(int64_t)r * n + i];

      const double zero3[3] = {0, 0, 0};
      const double g0[3] = {-sm.gravity[0], -sm.gravity[1], -sm.gravity[2]};
      double t2[BATOTP_MAX_LINKS], t4[BATOTP_MAX_LINKS];
      rnea_pass(sm, cq, sq, q1, q2, zero3, t2);
      rnea_pass(sm, cq, sq, z, z, g0, t4);
      bool isStatic = false;
#pragma unroll
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
         if (j < nl)
         {
            db[(int64_t)(R + j) * n + i] = (t2[j] + sm.link[j].fv * q1[j]) + t4[j];
            if (!(t4[j] - C.hi[j] < 0.0 && C.lo[j] - t4[j] < 0.0)) isStatic = true;
         }
      nStatic = isStatic ? 1 : 0;
      if (!isStatic)
      {
#pragma unroll
         for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
            if (j < nl)
            {
               const double A = t2[j], B = sm.link[j].fv * q1[j], G = t4[j];
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
   const int64_t nblk = (pd.n + TSCALE_BP - 1) / TSCALE_BP;
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
