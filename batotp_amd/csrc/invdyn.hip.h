// invdyn.hip.h -- kernels of batotp_hip_output_torques (include/batotp_hip_invdyn.h has the definition they implement).
//
// k_invdyn        one workgroup of INVDYN_THREADS lanes per block of BATOTP_INVDYN_BLOCK_POINTS points of ONE path, one lane per
//                 point; the grid is a host-built table of (path, block) descriptors as in the audit, so a ragged batch wastes no
//                 workgroup and no lane searches for its path.  The chain model is staged in LDS and read as broadcasts (as
//                 k_dyn_serial does).  Lanes run along the point index (rows are [R][n] per path), so the three loads per joint row
//                 (i-1, i, i+1) are coalesced and their overlap comes from the cache: the recursion costs well over 1e3 fp64 operations per
//                 point against 8 bytes per row value, so a tile with halo in LDS would buy nothing and cost registers the two passes
//                 need.  The same lane copies the joint and Cartesian rows of its point into the new output: the rows are read once.
// k_invdyn_pack   joint rows of an output with Cartesian rows, packed [n_links][n] per path for the host trig tables
//                 (BATOTP_F_HOST_TRIG; an output without Cartesian rows already is that array).
//
// invdyn_point    everything a lane does for its point, shared with k_tscale (tscale.hip.h), which goes on from the three addends.
//
// Both passes are rnea_pass of kernels.hip.h exactly as the dynamics precompute calls it: the bits of a torque row are those of
// a2 + a3 + a4 of k_dyn_serial for (q, dq/dt, d2q/dt2).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batotp_hip_invdyn.h"
#include "kernels.hip.h"
#include "output_plan.h" // PathBlock

namespace bk
{

constexpr int INVDYN_BP = BATOTP_INVDYN_BLOCK_POINTS;
constexpr int INVDYN_THREADS = INVDYN_BP; // one lane per point

// the fields every torque kernel reads of a path; TscalePath (tscale.hip.h) begins with one, so a table of either is read through
// invdyn_path_at with its own stride
struct InvdynPath
{
   int64_t off;   // first point of the path in the rows of the source and of the result (points)
   int64_t n;     // points
   int64_t tOff;  // first point of the path in the packed joint rows / trig tables of its range
   double c1, c2; // 1 / (2 h), 1 / (h h)
};

__device__ __forceinline__ const InvdynPath &invdyn_path_at(const void *paths, int stride, int k)
{
   return *reinterpret_cast<const InvdynPath *>(static_cast<const char *>(paths) + (int64_t)k * stride);
}

// cooperative copy of the chain model into LDS (8-byte words); the caller synchronises
__device__ __forceinline__ void invdyn_stage_model(const batotp_serial_model *__restrict__ model, batotp_serial_model &sm)
{
   const double *from = reinterpret_cast<const double *>(model);
   double *to = reinterpret_cast<double *>(&sm);
   for (int k = threadIdx.x; k < (int)(sizeof(batotp_serial_model) / 8); k += INVDYN_THREADS) to[k] = from[k];
}

// Point i < pd.n of a path: copies its joint and Cartesian rows, writes its torque rows (t2 + fv qd) + t4 and leaves the three
// addends of every joint of the model in t2, fvq and t4, and the joint velocities unit * v in q1 (0 beyond n_links; k_duty, duty.hip.h,
// forms the power from them).  Every array is indexed by unrolled loops only: they stay in registers.
__device__ __forceinline__ void invdyn_point(const batotp_serial_model &sm, const InvdynPath &pd, int64_t i, const double *__restrict__ src, int nCart,
                                             const double *__restrict__ trig, double *__restrict__ dst, double (&t2)[BATOTP_MAX_LINKS],
                                             double (&fvq)[BATOTP_MAX_LINKS], double (&t4)[BATOTP_MAX_LINKS], double (&q1)[BATOTP_MAX_LINKS])
{
   const int64_t n = pd.n;
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

   double cq[BATOTP_MAX_LINKS], sq[BATOTP_MAX_LINKS], q2[BATOTP_MAX_LINKS], z[BATOTP_MAX_LINKS];
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
   rnea_pass(sm, cq, sq, q1, q2, zero3, t2);
   rnea_pass(sm, cq, sq, z, z, g0, t4);
#pragma unroll
   for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
      if (j < nl)
      {
         fvq[j] = sm.link[j].fv * q1[j];
         db[(int64_t)(R + j) * n + i] = (t2[j] + fvq[j]) + t4[j];
      }
}

// the same for a caller that goes on from the three addends alone
__device__ __forceinline__ void invdyn_point(const batotp_serial_model &sm, const InvdynPath &pd, int64_t i, const double *__restrict__ src, int nCart,
                                             const double *__restrict__ trig, double *__restrict__ dst, double (&t2)[BATOTP_MAX_LINKS],
                                             double (&fvq)[BATOTP_MAX_LINKS], double (&t4)[BATOTP_MAX_LINKS])
{
   double q1[BATOTP_MAX_LINKS];
   invdyn_point(sm, pd, i, src, nCart, trig, dst, t2, fvq, t4, q1);
}

// blocks: points [blk * INVDYN_BP, (blk + 1) * INVDYN_BP) of the path (path: index into the range's descriptors, pathStride bytes each)
__global__ __launch_bounds__(INVDYN_THREADS) void k_invdyn_pack(const void *__restrict__ paths, int pathStride, const PathBlock *__restrict__ blocks, int nBlocks,
                                                                const double *__restrict__ src, int nl, int nCart, double *__restrict__ pack)
{
   if ((int)blockIdx.x >= nBlocks) return;
   const PathBlock bd = blocks[blockIdx.x];
   const InvdynPath pd = invdyn_path_at(paths, pathStride, bd.path);
   const int64_t n = pd.n, i = (int64_t)bd.blk * INVDYN_BP + (int)threadIdx.x;
   if (i >= n) return;
   const double *sb = src + pd.off * (nl + nCart);
   double *pb = pack + pd.tOff * nl;
   for (int j = 0; j < nl; ++j) pb[(int64_t)j * n + i] = sb[(int64_t)j * n + i];
}

__global__ __launch_bounds__(INVDYN_THREADS) void k_invdyn(const batotp_serial_model *__restrict__ model, const InvdynPath *__restrict__ paths,
                                                           const PathBlock *__restrict__ blocks, int nBlocks, const double *__restrict__ src, int nCart,
                                                           const double *__restrict__ trig, double *__restrict__ dst)
{
   __shared__ batotp_serial_model sm;
   invdyn_stage_model(model, sm);
   __syncthreads();
   if ((int)blockIdx.x >= nBlocks) return;
   const PathBlock bd = blocks[blockIdx.x];
   const InvdynPath pd = paths[bd.path];
   const int64_t i = (int64_t)bd.blk * INVDYN_BP + (int)threadIdx.x;
   if (i >= pd.n) return;
   double t2[BATOTP_MAX_LINKS], fvq[BATOTP_MAX_LINKS], t4[BATOTP_MAX_LINKS];
   invdyn_point(sm, pd, i, src, nCart, trig, dst, t2, fvq, t4);
}

} // namespace bk
