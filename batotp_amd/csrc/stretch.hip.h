// stretch.hip.h -- kernel of batotp_hip_output_stretch_to / _by / _audit (include/batotp_hip_stretch.h has the definition it implements).
//
// k_stretch   one workgroup of STRETCH_THREADS lanes per block of BATOTP_STRETCH_BLOCK_POINTS NEW points of ONE path, one lane per new
//             point, looping over the rows; the grid is a host-built table of (path, block) descriptors as in the audit and the torque
//             rows, so a ragged batch wastes no workgroup and no lane searches for its path.  The position of a point (j, f) is the
//             same for every row and is formed once per lane.
//             The factor is >= 1, so the new points [p0, p1] of a block read the source points [max(j(p0) - 1, 0), min(j(p1) + 2, n - 1)]
//             and, because rk <= 1, j(p1) - j(p0) <= STRETCH_BP: a window of at most STRETCH_BP + 4 points per row.  The block stages
//             that window of up to STRETCH_TILE_ROWS rows in LDS with coalesced loads (one load instruction per wavefront and row) and
//             every lane takes its four values per row from there.  The first form of this kernel read them with four global loads per
//             lane and row -- coalesced, their overlap served by the cache --; this one takes 15 - 32 % less time (profiles/stretch_bench.txt): that one
//             issued five memory instructions per 512 bytes written where this one issues two, and the kernel's time follows the
//             memory instructions, not the bytes (at factor 2 it reads half of what a copy reads and was no faster than the copy).
//             A path that is copied (n2 == n, or fewer than two points) goes straight from global memory to global memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batotp_hip_stretch.h"
#include "output_plan.h" // PathBlock

namespace bk
{

constexpr int STRETCH_BP = BATOTP_STRETCH_BLOCK_POINTS;
constexpr int STRETCH_THREADS = STRETCH_BP; // one lane per new point
constexpr int STRETCH_TILE = STRETCH_BP + 8; // points of a row's window in LDS (at most STRETCH_BP + 4 are used)
constexpr int STRETCH_TILE_ROWS = 8;         // rows staged per pass: 16.5 KB of LDS

struct StretchPath
{
   int64_t offIn, nIn;   // first point of the path in the rows of the source (points), its points
   int64_t offOut, nOut; // the same in the result
   double rk;            // (double)(nIn - 1) / (double)(nOut - 1); unused where the path is copied
};

__global__ __launch_bounds__(STRETCH_THREADS) void k_stretch(const StretchPath *__restrict__ paths, const PathBlock *__restrict__ blocks, int nBlocks,
                                                             const double *__restrict__ src, int R, double *__restrict__ dst)
{
   __shared__ double tile[STRETCH_TILE_ROWS][STRETCH_TILE];
   if ((int)blockIdx.x >= nBlocks) return;
   const PathBlock bd = blocks[blockIdx.x]; // new points [blk * STRETCH_BP, (blk + 1) * STRETCH_BP) of path `path` of the range
   const StretchPath pd = paths[bd.path];
   const int64_t n = pd.nIn, n2 = pd.nOut, p0 = (int64_t)bd.blk * STRETCH_BP, p = p0 + (int)threadIdx.x;
   const double *__restrict__ sb = src + pd.offIn * R;
   double *__restrict__ db = dst + pd.offOut * R;
   if (n2 == n || n < 2) // the same in every lane of the block: a path copied as it is
   {
      if (p < n2)
         for (int r = 0; r < R; ++r) db[(int64_t)r * n2 + p] = sb[(int64_t)r * n + p];
      return;
   }
   // the window, from the first and the last new point of the block (the arithmetic of their own lanes; j is monotone in p)
   const int64_t p1 = (p0 + STRETCH_BP < n2 ? p0 + STRETCH_BP : n2) - 1;
   int64_t ja = (int64_t)((double)p0 * pd.rk), jb = (int64_t)((double)p1 * pd.rk);
   if (ja > n - 2) ja = n - 2;
   if (jb > n - 2) jb = n - 2;
   const int64_t w0 = ja >= 1 ? ja - 1 : 0, w1 = jb + 2 <= n - 1 ? jb + 2 : n - 1;
   int count = (int)(w1 - w0 + 1);
   if (count > STRETCH_TILE) count = STRETCH_TILE; // (cannot happen, see above: never write past the tile)

   const bool live = p < n2, last = p == n2 - 1;
   const double u = (double)p * pd.rk;
   int64_t j = (int64_t)u;
   if (j > n - 2 || !live) j = n - 2;
   const double f = u - (double)j;
   const bool lo = j >= 1, hi = j + 2 <= n - 1;
   // places in the window: of x[j], of x[j-1] and x[j+2] (in range whether or not the value is used), of x[n-1]
   const int t0 = (int)(j - w0), tm = lo ? t0 - 1 : t0, tp = hi ? t0 + 2 : t0 + 1, tl = (int)(n - 1 - w0);
   for (int rb = 0; rb < R; rb += STRETCH_TILE_ROWS)
   {
      const int rn = R - rb < STRETCH_TILE_ROWS ? R - rb : STRETCH_TILE_ROWS;
      if (rb) __syncthreads(); // the pass before has been read
      for (int r = 0; r < rn; ++r)
         for (int i = threadIdx.x; i < count; i += STRETCH_THREADS) tile[r][i] = sb[(int64_t)(rb + r) * n + w0 + i];
      __syncthreads();
      if (live)
         for (int r = 0; r < rn; ++r)
         {
            double y;
            if (last) y = tile[r][tl]; // x[n-1], by rule (the last block's window ends there)
            else
            {
               const double xm = tile[r][tm], x0 = tile[r][t0], x1 = tile[r][t0 + 1], xp = tile[r][tp];
               const double d = x1 - x0;
               const double m0 = lo ? (x1 - xm) * 0.5 : d;
               const double m1 = hi ? (xp - x0) * 0.5 : d;
               const double c2 = (3.0 * d - 2.0 * m0) - m1;
               const double c3 = (m0 + m1) - 2.0 * d;
               y = x0 + f * (m0 + f * (c2 + f * c3));
            }
            db[(int64_t)(rb + r) * n2 + p] = y;
         }
   }
}

} // namespace bk
