// duty.hip.h -- kernels of batotp_hip_output_duty / _stretch_duty (include/batotp_hip_duty.h has the definition they implement).
//
// k_duty          the grid, the lanes and the point of k_tscale (tscale.hip.h): invdyn_point, then the scale candidate and the static
//                 flag exactly as k_tscale forms them, so that a round of the stretch needs one pass over the rows.  On top of that the
//                 lane forms the seven moments of every joint and the positive part of the power -- 7 n_links + 1 values, DUTY_Q = 57
//                 for the largest model -- and the workgroup sums every one of them in the order the header prescribes.
// k_duty_finish   one lane per (path, quantity) adds the block sums in ascending block order; the wavefront takes the power maximum
//                 under its total order.  The scale partials are finished by k_tscale_finish itself.
//
// The sum inside a wavefront.  Reducing 57 values one after another costs 6 exchanges and 6 additions EACH (342 fp64 additions and
// 684 32-bit cross-lane moves per lane).  Here the wavefront transposes while it halves: at the step with distance d a lane keeps the
// half of its values that belongs to its side of the halving (lanes with bit d clear keep the quantities [0, d), the others
// [d, 2 d)), sends the other half to lane ^ d and adds what it receives.  A lane exchanges and adds 32 + 16 + .. + 1 = 63 values in
// all, and at the end lane q owns the wavefront's sum of quantity q.  Every addition is one the header's tree performs: the value
// that lane l holds of a kept quantity after the step d is (position l mod d) + (position l mod d + d) of the values before it, and
// IEEE addition is commutative, so which of the two lanes performs it does not show in the bits.  The selects are on compile-time
// indices: no per-lane array is indexed dynamically.
// No floating-point atomics; nothing depends on the order of arrival: the same bits for any grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "batotp_hip_duty.h"
#include "tscale.hip.h"

namespace bk
{

constexpr int DUTY_BP = BATOTP_DUTY_BLOCK_POINTS;
constexpr int DUTY_THREADS = DUTY_BP; // one lane per point
constexpr int DUTY_Q = 7 * BATOTP_MAX_LINKS + 1; // quantity 7 j + m: moment m of joint j; quantity 7 BATOTP_MAX_LINKS: w
constexpr int DUTY_QS = 64;                      // doubles per block in the partial sums: lane q of the finish reads quantity q
static_assert(DUTY_BP == TSCALE_BP && DUTY_THREADS == 128, "two wavefronts per block: block sum = wave 0 + wave 1");
static_assert(DUTY_Q <= DUTY_QS, "one lane of a wavefront per quantity");
static_assert(sizeof(batotp_path_duty_sums) == 8 * (DUTY_Q + 3) && offsetof(batotp_path_duty_sums, W) == 8 * (DUTY_Q - 1),
              "k_duty_finish writes quantity q to the q-th double of the record");

// "none" is (-Inf, -1); a candidate has a point >= 0 and a power that is not NaN
struct DutyPeak
{
   double p;
   long long at;
   __device__ __forceinline__ void none() { p = -__builtin_inf(); at = -1; }
   __device__ __forceinline__ void merge(double op, long long oa)
   {
      if (oa >= 0 && (at < 0 || op > p || (op == p && oa < at))) { p = op; at = oa; }
   }
   __device__ __forceinline__ void waveReduce()
   {
      for (int d = 32; d >= 1; d >>= 1)
      {
         const double op = __shfl_down(p, d);
         const long long oa = __shfl_down(at, d);
         merge(op, oa);
      }
   }
};

// the header's tree over the 64 lanes of a wavefront for 64 quantities at once; returns, in lane q, the sum of quantity q
__device__ __forceinline__ double duty_wave_sums(double (&v)[DUTY_QS], int lane)
{
#pragma unroll
   for (int d = 32; d >= 1; d >>= 1)
   {
      const bool up = (lane & d) != 0;
#pragma unroll
      for (int q = 0; q < d; ++q)
      {
         const double a = v[q], b = v[q + d];
         const double keep = up ? b : a, send = up ? a : b;
         v[q] = keep + __shfl_xor(send, d);
      }
   }
   return v[0];
}

__global__ __launch_bounds__(DUTY_THREADS) void k_duty(const batotp_serial_model *__restrict__ model, TscaleConst C, const TscalePath *__restrict__ paths,
                                                       const PathBlock *__restrict__ blocks, int nBlocks, const double *__restrict__ src, int nCart,
                                                       const double *__restrict__ trig, double *__restrict__ dst, TscalePartial *__restrict__ partials,
                                                       double *__restrict__ sums, DutyPeak *__restrict__ peaks)
{
   constexpr int NW = DUTY_THREADS / 64;
   __shared__ batotp_serial_model sm;
   __shared__ double redX[NW], redP[NW], redQ[NW][DUTY_QS];
   __shared__ long long redA[NW], redN[NW], redPa[NW];
   __shared__ int redR[NW], redS[NW];
   invdyn_stage_model(model, sm);
   __syncthreads();
   if ((int)blockIdx.x >= nBlocks) return; // the whole workgroup
   const PathBlock bd = blocks[blockIdx.x];
   const TscalePath pd = paths[bd.path];
   const int64_t i = (int64_t)bd.blk * DUTY_BP + (int)threadIdx.x;

   TscaleBest best;
   best.none();
   DutyPeak peak;
   peak.none();
   long long nStatic = 0;
   double v[DUTY_QS];
#pragma unroll
   for (int q = 0; q < DUTY_QS; ++q) v[q] = 0.0; // lanes past the end of the path, joints past the end of the model
   if (i < pd.p.n)
   {
      const int nl = sm.n_links;
      double t2[BATOTP_MAX_LINKS], fvq[BATOTP_MAX_LINKS], t4[BATOTP_MAX_LINKS], qd[BATOTP_MAX_LINKS];
      invdyn_point(sm, pd.p, i, src, nCart, trig, dst, t2, fvq, t4, qd);
      // the scale candidate: k_tscale
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
      // the moments and the power
      double p = 0.0;
#pragma unroll
      for (int j = 0; j < BATOTP_MAX_LINKS; ++j)
         if (j < nl)
         {
            const double A = t2[j], B = fvq[j], G = t4[j];
            const double tau = (A + B) + G;
            v[7 * j + 0] = A * A; v[7 * j + 1] = A * B; v[7 * j + 2] = B * B; v[7 * j + 3] = A * G;
            v[7 * j + 4] = B * G; v[7 * j + 5] = G * G; v[7 * j + 6] = tau * tau;
            const double e = tau * qd[j];
            p = j == 0 ? e : p + e;
         }
      v[DUTY_Q - 1] = p > 0.0 ? p : 0.0;
      if (p == p) { peak.p = p; peak.at = i; }
   }

   // workgroup reduction: in-wave, then through LDS
   const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
   nStatic = tscale_wave_sum(nStatic);
   best.waveReduce();
   peak.waveReduce();
   redQ[wave][lane] = duty_wave_sums(v, lane);
   if (lane == 0)
   {
      redX[wave] = best.x; redA[wave] = best.a; redR[wave] = best.r; redS[wave] = best.sd; redN[wave] = nStatic;
      redP[wave] = peak.p; redPa[wave] = peak.at;
   }
   __syncthreads();
   const int64_t slot = pd.pOff + bd.blk;
   if ((int)threadIdx.x < DUTY_Q) sums[slot * DUTY_QS + (int)threadIdx.x] = redQ[0][threadIdx.x] + redQ[1][threadIdx.x];
   if (threadIdx.x == 0)
   {
      long long ns = redN[0];
      for (int w = 1; w < NW; ++w) { best.merge(redX[w], redA[w], redR[w], redS[w]); ns += redN[w]; peak.merge(redP[w], redPa[w]); }
      TscalePartial *out = partials + slot;
      out->x = best.x; out->at = best.a; out->row = best.r; out->side = best.sd; out->nStatic = ns;
      peaks[slot].p = peak.p; peaks[slot].at = peak.at;
   }
}

// one wavefront per path of the range, one lane per quantity
__global__ __launch_bounds__(64) void k_duty_finish(const TscalePath *__restrict__ paths, int nPaths, const double *__restrict__ sums,
                                                    const DutyPeak *__restrict__ peaks, batotp_path_duty_sums *__restrict__ out)
{
   const int k = (int)blockIdx.x;
   if (k >= nPaths) return;
   const TscalePath pd = paths[k];
   const int lane = (int)threadIdx.x;
   const int64_t nblk = (pd.p.n + DUTY_BP - 1) / DUTY_BP;
   double S = 0.0;
   if (lane < DUTY_Q && nblk > 0)
   {
      const double *p = sums + pd.pOff * DUTY_QS + lane;
      S = p[0];
#pragma unroll 4
      for (int64_t b = 1; b < nblk; ++b) S = S + p[b * DUTY_QS];
   }
   DutyPeak peak;
   peak.none();
   for (int64_t b = lane; b < nblk; b += 64) peak.merge(peaks[pd.pOff + b].p, peaks[pd.pOff + b].at);
   peak.waveReduce();
   if (lane < DUTY_Q) reinterpret_cast<double *>(out + k)[lane] = S;
   if (lane == 0) { out[k].peak_power = peak.p; out[k].power_at = peak.at; out[k].n_pts = pd.p.n; }
}

} // namespace bk
