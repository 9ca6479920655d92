// audit.hip.h -- kernels of batotp_hip_output_audit (include/batotp_hip_audit.h has the definition they implement).
//
// k_audit_blocks   one workgroup of AUDIT_THREADS lanes per block of BATOTP_AUDIT_BLOCK_POINTS points of ONE path; the grid is a
//                  host-built table of (path, block) descriptors, so a ragged batch wastes no workgroup.  Lanes run along the point
//                  index (rows are [R][n] per path: coalesced).  A row's tile and its halo of one point on each side go through LDS,
//                  so every row value is read from HBM once (8 R bytes per point; the halo points are read again by the neighbouring
//                  workgroup, 2 in 1024); the next row's loads are in flight while a row is evaluated.  No division: the reciprocals
//                  come in the constant block.  Each lane keeps one candidate per family, the workgroup reduces them in-wave
//                  (__shfl_down) and then through LDS to ONE partial per family.
// k_audit_finish   one wavefront per path reduces the path's partials and writes its batotp_path_audit.
//
// Candidates are (value, point, row) under the total order "value descending, point ascending, row ascending", and the counts are
// integer sums: no floating-point atomics, nothing depends on the order of arrival, and the result is the same bits for every
// block size and grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "batotp_hip_audit.h"
#include "output_plan.h" // PathBlock

namespace bk
{

constexpr int AUDIT_BP = BATOTP_AUDIT_BLOCK_POINTS;
constexpr int AUDIT_THREADS = 256;
constexpr int AUDIT_PPT = AUDIT_BP / AUDIT_THREADS; // points per lane
constexpr int AUDIT_NF = BATOTP_AUDIT_FAMILIES;
static_assert(AUDIT_BP % AUDIT_THREADS == 0 && AUDIT_PPT >= 1 && AUDIT_PPT <= 32, "a lane's points are flags of one 32-bit word");

// limits of the call as the kernel needs them (kernel argument): reciprocals formed on the host
struct AuditConst
{
   int nTheta, nCart, nTrq, nPos; // rows; nPos = min(3, nCart) position rows
   unsigned fams;                 // bit f: family f is audited
   int pad;
   double lim;                    // 1.0 + tol
   double rv[BATOTP_MAX_JOINTS], ra[BATOTP_MAX_JOINTS];
   double mid[BATOTP_MAX_JOINTS], rt[BATOTP_MAX_JOINTS];
   double rcv, rca;
};

struct AuditPath
{
   int64_t off;   // first point of the path in the rows (points: the path's block starts at off * R doubles)
   int64_t n;     // points
   int64_t pOff;  // first partial of the path
   double c1, c2; // 1 / (2 h), 1 / (h h)
};

struct AuditPartial
{
   double val[AUDIT_NF];
   long long at[AUDIT_NF];
   int row[AUDIT_NF];
   int pad;
   long long nOver, nNonfinite;
};

// is candidate (v, a, r) ahead of (bv, ba, br)?
__device__ __forceinline__ bool audit_ahead(double v, long long a, int r, double bv, long long ba, int br)
{
   return v > bv || (v == bv && (a < ba || (a == ba && r < br)));
}

struct AuditBest
{
   double v;
   long long a;
   int r;
   __device__ __forceinline__ void offer(double u, long long at, int row)
   {
      // a utilisation that is not finite (NaN fails every comparison, Inf the first) takes no part
      if (u <= 1.7976931348623157e308 && audit_ahead(u, at, row, v, a, r)) { v = u; a = at; r = row; }
   }
   __device__ __forceinline__ void merge(double ov, long long oa, int orow)
   {
      if (audit_ahead(ov, oa, orow, v, a, r)) { v = ov; a = oa; r = orow; }
   }
   __device__ __forceinline__ void waveReduce()
   {
      for (int d = 32; d >= 1; d >>= 1)
      {
         const double ov = __shfl_down(v, d);
         const long long oa = __shfl_down(a, d);
         const int orow = __shfl_down(r, d);
         merge(ov, oa, orow);
      }
   }
};

__device__ __forceinline__ long long audit_wave_sum(long long x)
{
   for (int d = 32; d >= 1; d >>= 1) x += __shfl_down(x, d);
   return x;
}

__global__ __launch_bounds__(AUDIT_THREADS) void k_audit_blocks(AuditConst C, const AuditPath *__restrict__ paths, const PathBlock *__restrict__ blocks,
                                                                int nBlocks, const double *__restrict__ rows, AuditPartial *__restrict__ partials)
{
   __shared__ double tile[2][AUDIT_BP + 2];
   constexpr int NW = AUDIT_THREADS / 64;
   __shared__ double redV[NW][AUDIT_NF];
   __shared__ long long redA[NW][AUDIT_NF];
   __shared__ int redR[NW][AUDIT_NF];
   __shared__ long long redN[NW][2];

   if ((int)blockIdx.x >= nBlocks) return;
   const PathBlock bd = blocks[blockIdx.x]; // points [blk * AUDIT_BP, (blk + 1) * AUDIT_BP) of the path; partial pOff + blk
   const AuditPath pd = paths[bd.path];
   const int t = (int)threadIdx.x;
   const int64_t n = pd.n, p0 = (int64_t)bd.blk * AUDIT_BP;
   const int R = C.nTheta + C.nCart + C.nTrq;
   const double *base = rows + pd.off * R;
   const double c1 = pd.c1, c2 = pd.c2;
   const bool fJV = C.fams & (1u << BATOTP_AUDIT_JNT_VEL), fJA = C.fams & (1u << BATOTP_AUDIT_JNT_ACC);
   const bool fCV = C.fams & (1u << BATOTP_AUDIT_CART_VEL), fCA = C.fams & (1u << BATOTP_AUDIT_CART_ACC);
   const bool fT = C.fams & (1u << BATOTP_AUDIT_TRQ);

   // what this lane stages of a row: its AUDIT_PPT points and, lanes 0 and 1, the halo (0.0 outside the path: never evaluated)
   const int64_t haloAt = t == 0 ? p0 - 1 : p0 + AUDIT_BP;
   const bool haloLane = t < 2, haloIn = haloLane && haloAt >= 0 && haloAt < n;
   double stage[AUDIT_PPT], stageHalo = 0.0;
   auto loadRow = [&](int r) {
      const double *x = base + (int64_t)r * n;
#pragma unroll
      for (int j = 0; j < AUDIT_PPT; ++j)
      {
         const int64_t i = p0 + t + j * AUDIT_THREADS;
         stage[j] = i < n ? x[i] : 0.0;
      }
      stageHalo = haloIn ? x[haloAt] : 0.0;
   };

   AuditBest best[AUDIT_NF];
#pragma unroll
   for (int f = 0; f < AUDIT_NF; ++f) { best[f].v = -1.0; best[f].a = -1; best[f].r = -1; }
   double sv[AUDIT_PPT], sa[AUDIT_PPT]; // sums of squares of the Cartesian velocity / acceleration components
#pragma unroll
   for (int j = 0; j < AUDIT_PPT; ++j) { sv[j] = 0.0; sa[j] = 0.0; }
   unsigned over = 0;   // bit j: an audited utilisation of point j of this lane exceeds the bound
   long long nonfinite = 0;

   if (R > 0) loadRow(0);
   for (int r = 0; r < R; ++r)
   {
      double *tl = tile[r & 1];
#pragma unroll
      for (int j = 0; j < AUDIT_PPT; ++j) tl[1 + t + j * AUDIT_THREADS] = stage[j];
      if (haloLane) tl[t == 0 ? 0 : AUDIT_BP + 1] = stageHalo;
      // one barrier per row: the tile written two rows ago is rewritten only after every lane has passed the barrier of the row
      // in between, i.e. has finished reading it
      __syncthreads();
      if (r + 1 < R) loadRow(r + 1); // in flight while this row is evaluated

      const bool joint = r < C.nTheta;
      const int cr = r - C.nTheta;                   // Cartesian row
      const bool pos = cr >= 0 && cr < C.nPos && (fCV || fCA);
      const int tr = r - C.nTheta - C.nCart;         // torque row
      const bool trq = tr >= 0 && fT;
      const double rvr = joint ? C.rv[r] : 0.0, rar = joint ? C.ra[r] : 0.0;
      const double midr = trq ? C.mid[tr] : 0.0, rtr = trq ? C.rt[tr] : 0.0;
#pragma unroll
      for (int j = 0; j < AUDIT_PPT; ++j)
      {
         const int li = t + j * AUDIT_THREADS;
         const int64_t i = p0 + li;
         if (i >= n) continue;
         const double xm = tl[li], x0 = tl[li + 1], xp = tl[li + 2];
         if (!(fabs(x0) <= 1.7976931348623157e308)) ++nonfinite;
         if (trq)
         {
            const double u = fabs(x0 - midr) * rtr;
            best[BATOTP_AUDIT_TRQ].offer(u, i, tr);
            if (u <= 1.7976931348623157e308 && u > C.lim) over |= 1u << j;
         }
         if ((joint || pos) && i >= 1 && i <= n - 2)
         {
            const double v = (xp - xm) * c1;
            const double a = ((xp - x0) - (x0 - xm)) * c2;
            if (joint)
            {
               if (fJV)
               {
                  const double u = fabs(v) * rvr;
                  best[BATOTP_AUDIT_JNT_VEL].offer(u, i, r);
                  if (u <= 1.7976931348623157e308 && u > C.lim) over |= 1u << j;
               }
               if (fJA)
               {
                  const double u = fabs(a) * rar;
                  best[BATOTP_AUDIT_JNT_ACC].offer(u, i, r);
                  if (u <= 1.7976931348623157e308 && u > C.lim) over |= 1u << j;
               }
            }
            else
            {
               // (vx*vx + vy*vy) + vz*vz, one term per position row
               sv[j] = cr == 0 ? v * v : sv[j] + v * v;
               sa[j] = cr == 0 ? a * a : sa[j] + a * a;
               if (cr == C.nPos - 1)
               {
                  if (fCV)
                  {
                     const double u = sqrt(sv[j]) * C.rcv;
                     best[BATOTP_AUDIT_CART_VEL].offer(u, i, 0);
                     if (u <= 1.7976931348623157e308 && u > C.lim) over |= 1u << j;
                  }
                  if (fCA)
                  {
                     const double u = sqrt(sa[j]) * C.rca;
                     best[BATOTP_AUDIT_CART_ACC].offer(u, i, 0);
                     if (u <= 1.7976931348623157e308 && u > C.lim) over |= 1u << j;
                  }
               }
            }
         }
      }
   }

   // workgroup reduction: in-wave, then through LDS
   const int lane = t & 63, wave = t >> 6;
   long long nOver = audit_wave_sum((long long)__popc(over));
   long long nNon = audit_wave_sum(nonfinite);
#pragma unroll
   for (int f = 0; f < AUDIT_NF; ++f) best[f].waveReduce();
   if (lane == 0)
   {
#pragma unroll
      for (int f = 0; f < AUDIT_NF; ++f) { redV[wave][f] = best[f].v; redA[wave][f] = best[f].a; redR[wave][f] = best[f].r; }
      redN[wave][0] = nOver; redN[wave][1] = nNon;
   }
   __syncthreads();
   AuditPartial *out = partials + (pd.pOff + bd.blk);
   if (t < AUDIT_NF)
   {
      AuditBest b;
      b.v = redV[0][t]; b.a = redA[0][t]; b.r = redR[0][t];
      for (int w = 1; w < NW; ++w) b.merge(redV[w][t], redA[w][t], redR[w][t]);
      out->val[t] = b.v; out->at[t] = b.a; out->row[t] = b.r;
   }
   if (t == AUDIT_NF)
   {
      long long a = 0, b = 0;
      for (int w = 0; w < NW; ++w) { a += redN[w][0]; b += redN[w][1]; }
      out->nOver = a; out->nNonfinite = b; out->pad = 0;
   }
}

// one wavefront per path
__global__ __launch_bounds__(64) void k_audit_finish(const AuditPath *__restrict__ paths, int nPaths, const AuditPartial *__restrict__ partials,
                                                     batotp_path_audit *__restrict__ out)
{
   const int k = (int)blockIdx.x;
   if (k >= nPaths) return;
   const AuditPath pd = paths[k];
   const int lane = (int)threadIdx.x;
   const int64_t nblk = (pd.n + AUDIT_BP - 1) / AUDIT_BP;
   AuditBest best[AUDIT_NF];
#pragma unroll
   for (int f = 0; f < AUDIT_NF; ++f) { best[f].v = -1.0; best[f].a = -1; best[f].r = -1; }
   long long nOver = 0, nNon = 0;
   for (int64_t b = lane; b < nblk; b += 64)
   {
      const AuditPartial *p = partials + (pd.pOff + b);
#pragma unroll
      for (int f = 0; f < AUDIT_NF; ++f) best[f].merge(p->val[f], p->at[f], p->row[f]);
      nOver += p->nOver; nNon += p->nNonfinite;
   }
   nOver = audit_wave_sum(nOver);
   nNon = audit_wave_sum(nNon);
#pragma unroll
   for (int f = 0; f < AUDIT_NF; ++f) best[f].waveReduce();
   if (lane == 0)
   {
      batotp_path_audit *o = out + k;
#pragma unroll
      for (int f = 0; f < AUDIT_NF; ++f)
      {
         o->fam[f].peak = best[f].v; o->fam[f].at = best[f].a; o->fam[f].row = best[f].r; o->fam[f].reserved = 0;
      }
      o->n_pts = pd.n; o->n_over = nOver; o->n_nonfinite = nNon;
   }
}

} // namespace bk
