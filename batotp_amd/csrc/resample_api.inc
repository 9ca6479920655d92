// resample_api.inc -- host side of batotp_hip_resample (included at the end of batotp_hip.hip).
// Orchestrates the kernels of resample.hip.h; the only host work is sizing the next stage from the
// counts the previous stage reports (small device->host copies).
//
// Memory: three grow-only workspaces cached in the context (stage-0 arrays of all paths, scratch of
// one chunk of paths, the resampled knots).  hipMalloc of the tens of GB a large batch needs costs
// far more than the kernels (measured: 11.3 s of hipMalloc against 0.6 s of kernels for 4096 paths of
// 1e5 knots when every buffer was allocated per call), so the memory is kept between calls
// (batotp_hip_ctx_trim releases it).  Consequence for the caller: the knots of a batotp_resampled
// live in the context's workspace and stay valid until the next batotp_hip_resample on the same
// context, batotp_hip_ctx_trim or batotp_hip_ctx_destroy.

struct batotp_resampled
{
   batotp_ctx *ctx = nullptr;
   int32_t B = 0;
   int C = 0;
   std::vector<int64_t> n, off;
   std::vector<double> sres;
   std::vector<uint32_t> status;
   std::vector<double> au; // per path: integ_res, s_weights[3], scale_type as the automatic integration resolution left them
   double *dY = nullptr; // inside ctx->ws[2]
   uint64_t epoch = 0;   // resample call that produced dY
   int64_t total = 0;
   float ms = 0.f;
   int nChunks = 0;
   bool traced = false;
   uint64_t trace[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // batotp_hip_set_resample_trace: checksums of the intermediate stages (one-path calls)
   std::vector<double> traceData[8];             // ... and the arrays themselves of stages 2 and 3 (batotp_hip_resampled_trace_data)
};

// Every kernel of the resampler goes through this: a launch that fails (a bad configuration, the sticky error of an earlier
// call) ends batotp_hip_resample with a status at once instead of surfacing at some later check -- or not at all.
#define RS_LAUNCH(stream, kernel, grid, block, ...)                          \
   do                                                                        \
   {                                                                         \
      hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);       \
      HIP_TRY(hipGetLastError());                                            \
   } while (0)

namespace
{
int arenaReserve(Arena &a, size_t bytes, hipStream_t st, size_t keepBytes = 0)
{
   if (a.cap >= bytes) return BATOTP_OK;
   size_t want = bytes + bytes / 16 + (1u << 20);
   void *np = nullptr;
   hipError_t e = hipMalloc(&np, want);
   if (e != hipSuccess && want != bytes) { want = bytes; e = hipMalloc(&np, want); }
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (resample workspace)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if (a.p)
   {
      if (keepBytes)
      {
         e = hipMemcpyAsync(np, a.p, keepBytes, hipMemcpyDeviceToDevice, st);
         if (e == hipSuccess) e = hipStreamSynchronize(st);
         if (e != hipSuccess) { hipFree(np); return hipFail(e, "workspace growth copy"); }
      }
      hipFree(a.p);
   }
   a.p = np; a.cap = want;
   return BATOTP_OK;
}

// bump sub-allocation inside a workspace (256-byte granules)
struct Bump
{
   char *base = nullptr;
   size_t at = 0;
   template <typename T> T *take(size_t count)
   {
      T *p = reinterpret_cast<T *>(base + at);
      at += (sizeof(T) * (count ? count : 1) + 255) & ~(size_t)255;
      return p;
   }
};
size_t granule(size_t bytes) { return ((bytes ? bytes : 1) + 255) & ~(size_t)255; }

// what a call holds until it returns, on every path out of it: an output it is making, an event, device memory of its own
struct OutputOwner
{
   batotp_output *o = nullptr;
   ~OutputOwner() { batotp_hip_output_destroy(o); }
   batotp_output *release() { batotp_output *r = o; o = nullptr; return r; }
};
struct Event
{
   hipEvent_t e = nullptr;
   ~Event() { if (e) hipEventDestroy(e); }
};
struct DevMem
{
   void *p = nullptr;
   ~DevMem() { if (p) hipFree(p); }
   int alloc(size_t bytes, const char *label) // label: "hipMalloc (...)" of the error text
   {
      hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
      if (e == hipSuccess) return BATOTP_OK;
      p = nullptr;
      hipFail(e, label);
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
};

// diagnostic (batotp_hip_set_resample_trace, one-path calls): the order-independent checksum of `count` doubles at `ptr`, as
// batotp_hip_resampled_checksums forms it, into slot `k` of the call's trace.  Where two evaluations of the same path disagree, the first
// slot that differs names the stage -- and so the kernel -- that produced the difference.
int rsTraceSum(batotp_ctx *ctx, int k, const double *ptr, int64_t count)
{
   if (!ctx->rsTrace) return BATOTP_OK;
   hipStream_t st = ctx->stream;
   if (!ctx->dTrace) HIP_TRY(hipMalloc((void **)&ctx->dTrace, 3 * sizeof(unsigned long long)));
   const int64_t hostArgs[2] = {0, count > 0 ? count : 0};
   HIP_TRY(hipMemcpyAsync(ctx->dTrace, hostArgs, sizeof(hostArgs), hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(ctx->dTrace + 2, 0, sizeof(unsigned long long), st));
   const unsigned bx = (unsigned)std::max<int64_t>(1, std::min<int64_t>(64, (count + 2047) / 2048));
   RS_LAUNCH(st, k_rs_checksum, dim3(bx, 1), dim3(256), (const int64_t *)ctx->dTrace, (const int64_t *)(ctx->dTrace + 1), 1, ptr, ctx->dTrace + 2);
   unsigned long long h = 0;
   HIP_TRY(hipMemcpyAsync(&h, ctx->dTrace + 2, sizeof(h), hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));
   ctx->rsTraceSums[k] = (uint64_t)h;
   // the second derivatives of the taught points and the points interpSpecial emitted are also kept on the host (a few MB for one
   // path): the traced event of round 6 first differed in stage 2, and WHERE two such arrays differ -- one series, one lane's chunk,
   // a cache line -- is what tells a defect of the solve from a fault of the platform (batotp_hip_resampled_trace_data)
   ctx->rsTraceData[k].clear();
   if ((k == 2 || k == 3) && count > 0)
   {
      ctx->rsTraceData[k].resize((size_t)count);
      HIP_TRY(hipMemcpyAsync(ctx->rsTraceData[k].data(), ptr, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
   }
   return BATOTP_OK;
}

int rsSplines(batotp_ctx *ctx, const std::vector<RsPath> &paths, int C, const double *x, double *sol, PathInfo *dPinfo, int *dRedo)
{
   const int B = (int)paths.size();
   std::vector<PathInfo> pi(B);
   for (int p = 0; p < B; ++p)
   {
      memset(&pi[p], 0, sizeof(PathInfo));
      pi[p].koff = paths[p].off;
      pi[p].n = paths[p].status ? 4 : paths[p].n; // failed paths: any in-bounds work, results unused
   }
   HIP_TRY(hipMemcpyAsync(dPinfo, pi.data(), sizeof(PathInfo) * B, hipMemcpyHostToDevice, ctx->stream));
   HIP_TRY(hipStreamSynchronize(ctx->stream)); // pi goes out of scope
   const int threads = B * C;
   // few series: a wavefront per series where the series is long enough (spline_lanes.hip.h), the lane-per-series kernel for the
   // rest; many series: the lane-per-series kernel for all (seriesLanesPay)
   const bool byLanes = seriesLanesPay(threads);
   if (byLanes) RS_LAUNCH(ctx->stream, k_spline_sol_lanes, dim3((unsigned)threads), dim3(64), dPinfo, B, C, x, sol, dRedo);
   const unsigned lanes = seriesBlock(threads);
   RS_LAUNCH(ctx->stream, k_spline_sol, dim3((unsigned)((threads + lanes - 1) / lanes)), dim3(lanes), dPinfo, B, C, C, x, sol, byLanes ? dRedo : nullptr);
   HIP_TRY(hipGetLastError());
   return BATOTP_OK;
}

// the three kernels of an adjust_s pass (see resample.hip.h); dPaths: device array of B entries
int rsArcLengths(hipStream_t st, const RsParams &P, RsPath *dPaths, int B, const double *x, double *ta, double *ca, double *sC, int64_t total, int special)
{
   const int bs = 256;
   const unsigned gridPts = (unsigned)((total + bs - 1) / bs);
   RS_LAUNCH(st, k_rs_seglen, dim3(gridPts), dim3(bs), P, dPaths, B, x, ta, ca, total);
   if (P.autoOn)
      RS_LAUNCH(st, k_rs_scan, dim3((unsigned)((B + 63) / 64)), dim3(64), P, dPaths, B, ta, ca, special);
   else
      RS_LAUNCH(st, k_rs_scan_rows, dim3((unsigned)((B + 1) / 2)), dim3(64), P, dPaths, B, ta, ca, special); // two paths per wavefront
   RS_LAUNCH(st, k_rs_sites, dim3(gridPts), dim3(bs), P, dPaths, B, ta, ca, sC, special, total);
   return BATOTP_OK;
}

// Trig tables made on the host (BATOTP_F_HOST_TRIG): every call is spelled out so that no optimiser decides which libm
// entry point runs -- the reference's optimised build calls sincos() where its source has cos and sin of one angle
// (robot.cpp:130-136, 198-199, and th2 of dynRR, robot.cpp:408-419) and cos() elsewhere; the chain model (this library's own)
// is DEFINED on separate cos() / sin() calls (DESIGN.md 2).  theta packed [nJ][n] per span at off*nJ, trig [rows][n] per span
// at off*rows.  kind: 0 forward kinematics (layout: resample.hip.h), 1 Robot::dynRR (cos th1, cos th2, cos(th1+th2), sin th2),
// 2 chain model (cos q_j rows, then sin q_j rows; unit = degrees -> radians factor or 1).  Threads over the spans.
struct TrigSpan { int64_t off, n; bool skip; };
double __attribute__((noinline)) hostPlainCos(double x) { return ::cos(x); }
double __attribute__((noinline)) hostPlainSin(double x) { return ::sin(x); }
int hostTrigRows(int kind, int robot, int nJ) { return kind == 0 ? fwdkin_trig_rows(robot, nJ) : (kind == 1 ? 4 : 2 * nJ); }
void hostTrigTables(int kind, int robot, int nJ, double unit, const std::vector<TrigSpan> &spans, const double *theta, double *trig)
{
   const int rows = hostTrigRows(kind, robot, nJ);
   auto work = [&](size_t pa, size_t pb) {
      for (size_t p = pa; p < pb; ++p)
      {
         const TrigSpan &q = spans[p];
         if (q.skip) continue;
         const int64_t n = q.n;
         const double *th = theta + q.off * nJ;
         double *tr = trig + q.off * rows;
         for (int64_t i = 0; i < n; ++i)
         {
            if (kind == 2)
               for (int j = 0; j < nJ; ++j)
               {
                  const double qj = unit * th[j * n + i];
                  tr[j * n + i] = hostPlainCos(qj);
                  tr[(nJ + j) * n + i] = hostPlainSin(qj);
               }
            else if (kind == 1)
            {
               const double th1 = KIN_DEG2RAD * th[i], th2 = KIN_DEG2RAD * th[n + i];
               tr[i] = hostPlainCos(th1);
               ::sincos(th2, &tr[3 * n + i], &tr[n + i]);
               tr[2 * n + i] = hostPlainCos(th1 + th2);
            }
            else if (robot == BATOTP_ROBOT_RR)
            {
               const double th1 = KIN_DEG2RAD * th[i], th2 = KIN_DEG2RAD * th[n + i];
               ::sincos(th1, &tr[2 * n + i], &tr[i]);
               ::sincos(th1 + th2, &tr[3 * n + i], &tr[n + i]);
            }
            else
               for (int k = 0; k < 7; ++k) ::sincos(KIN_DEG2RAD * th[k * n + i], &tr[(7 + k) * n + i], &tr[k * n + i]);
         }
      }
   };
   unsigned nThreads = std::thread::hardware_concurrency();
   if (nThreads < 1) nThreads = 1;
   if (nThreads > 64) nThreads = 64;
   if (nThreads > spans.size()) nThreads = (unsigned)spans.size();
   if (nThreads <= 1) { work(0, spans.size()); return; }
   std::vector<std::thread> pool;
   for (unsigned t = 0; t < nThreads; ++t)
      pool.emplace_back(work, spans.size() * t / nThreads, spans.size() * (t + 1) / nThreads);
   for (std::thread &t : pool) t.join();
}

// Robot::fwdKin on a stage (x: [C][n] per path): Cartesian rows from the joint rows.  paths = host copy of dPaths with the
// current point counts.  chain != nullptr: the tool point of that kinematic chain (kin_chain.hip.h) instead of the robot type's
// closed form, its host tables those of the chain model (kind 2).
int rsFwdKin(batotp_ctx *ctx, const RsParams &P, const batotp_kin_chain *chain, bool hostTrig, const std::vector<RsPath> &paths, const RsPath *dPaths, double *x,
             int64_t total)
{
   hipStream_t st = ctx->stream;
   const int B = (int)paths.size(), bs = 256, rows = chain ? 2 * P.nJ : fwdkin_trig_rows(P.robot, P.nJ);
   const unsigned grid = (unsigned)((total + bs - 1) / bs);
   const double *trigDev = nullptr;
   if (hostTrig)
   {
      int rc = arenaReserve(ctx->ws[3], sizeof(double) * (size_t)total * (size_t)(P.nJ + rows) + 512, st);
      if (rc) return rc;
      if ((rc = poisonFill(ctx, ctx->ws[3].p, ctx->ws[3].cap, st))) return rc;
      double *pack = (double *)ctx->ws[3].p, *trig = pack + (size_t)total * P.nJ;
      ctx->kinTheta.resize((size_t)total * P.nJ);
      ctx->kinTrig.resize((size_t)total * rows);
      RS_LAUNCH(st, k_rs_pack_theta, dim3(grid), dim3(bs), P, dPaths, B, x, pack, total);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), pack, sizeof(double) * ctx->kinTheta.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      std::vector<TrigSpan> spans(paths.size());
      for (size_t p = 0; p < paths.size(); ++p) spans[p] = TrigSpan{paths[p].off, paths[p].n, paths[p].status != 0};
      hostTrigTables(chain ? 2 : 0, P.robot, P.nJ, (chain && chain->degrees) ? KIN_DEG2RAD : 1.0, spans, ctx->kinTheta.data(), ctx->kinTrig.data());
      HIP_TRY(hipMemcpyAsync(trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, st));
      trigDev = trig;
   }
   if (chain) RS_LAUNCH(st, k_rs_fwdkin_chain, dim3(grid), dim3(bs), P, *chain, dPaths, B, x, trigDev, total);
   else RS_LAUNCH(st, k_rs_fwdkin, dim3(grid), dim3(bs), P, dPaths, B, x, trigDev, rows, total);
   HIP_TRY(hipGetLastError());
   if (hostTrig) HIP_TRY(hipStreamSynchronize(st)); // the host table may be rewritten by the next call
   return BATOTP_OK;
}

// BA::interpTrajLinear (ba.cpp:2768-2794) for a stage of 2 or 3 points -- a path shorter than four resolution steps: every
// row onto 4 evenly spaced nodes by linear interpolation (findInterpSegs spline.cpp:56-99, interp1linear :108-120).  Rare and
// tiny, so it runs on the host side of the library: vals[c * nOld + k] in, out[c * 4 + i] out.
void stretchToFour(const double *vals, int C, int nOld, double *out)
{
   double gOld[3], gNew[4];
   const double cOld = 1.0 / (double)(nOld - 1), cNew = 1.0 / 3.0;
   for (int k = 0; k < nOld; ++k) gOld[k] = cOld * (double)k;
   for (int k = 0; k < 4; ++k) gNew[k] = cNew * (double)k;
   int cur = 0;
   for (int i = 0; i < 4; ++i)
   {
      while (!(gNew[i] < gOld[cur + 1] || cur == nOld - 2)) ++cur;
      const double tau = (gNew[i] - gOld[cur]) / (gOld[cur + 1] - gOld[cur]);
      for (int c = 0; c < C; ++c)
      {
         const double a = vals[c * nOld + cur], b = vals[c * nOld + cur + 1];
         out[c * 4 + i] = a + (b - a) * tau;
      }
   }
}

int64_t rowsCap(const RsPath &q) { return q.status ? 4 : (int64_t)q.nOut + q.nOut / 8 + 64; }

// scratch bytes of the chunk stages for one path: n0 taught points, cap >= points of the first pass
size_t chunkBytesOfPath(const RsPath &q, int C)
{
   const size_t n0 = (size_t)q.n0, cap = (size_t)rowsCap(q);
   // sol0 | rows | x1, sol1 | ta1, ca1, s1
   return 8 * ((size_t)C * n0 + (size_t)C * cap + 2 * (size_t)C * cap + 3 * cap) + 4 * (sizeof(RsPath) + sizeof(PathInfo)) + 4 * (size_t)C + 16 * 256;
}

// stages 0b..2 for the paths of p0 (offsets local to x0 / s0); the knots are appended to the
// context's knot workspace at *yUsed (doubles); fills n2 / sres / status
int rsChunk(batotp_ctx *ctx, RsParams P, const batotp_resample_params *prm, const batotp_kin_chain *chain, bool cable, bool kin, bool hostTrig,
            std::vector<RsPath> &p0, const double *x0,
            const double *s0, int64_t *yUsed, int64_t *n2, double *sresOut, uint32_t *statusOut, double *autoOut)
{
   hipStream_t st = ctx->stream;
   const int B = (int)p0.size(), C = P.C;
   const int bs = 256;
   int rc;
   const int64_t tot0 = p0[B - 1].off + p0[B - 1].n0;

   int64_t totRows = 0;
   for (int p = 0; p < B; ++p)
   {
      p0[p].cap = (int32_t)rowsCap(p0[p]);
      p0[p].offOut = totRows;
      totRows += p0[p].cap;
   }
   if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;   // (every chunk starts from poisoned scratch)
   Bump w;
   w.base = (char *)ctx->ws[1].p;
   RsPath *dP0 = w.take<RsPath>(B), *dP1 = w.take<RsPath>(B), *dP2 = w.take<RsPath>(B);
   PathInfo *dPinfo = w.take<PathInfo>(B);
   int *dRedo = w.take<int>((size_t)B * C); // series the wavefront-per-series spline solve leaves to the sequential kernel
   double *sol0 = w.take<double>((size_t)tot0 * C);
   double *rows = w.take<double>((size_t)totRows * C);
   HIP_TRY(hipMemcpyAsync(dP0, p0.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
   const bool trace = ctx->rsTrace && B == 1 && !p0[0].status;
   if (trace && ((rc = rsTraceSum(ctx, 0, x0, (int64_t)p0[0].n * C)) || (rc = rsTraceSum(ctx, 1, s0, p0[0].n)))) return rc;   // taught points after stage 0, their sites
   if ((rc = rsSplines(ctx, p0, C, x0, sol0, dPinfo, dRedo))) return rc;
   if (trace && (rc = rsTraceSum(ctx, 2, sol0, (int64_t)p0[0].n * C))) return rc;                                                  // their second derivatives
   RS_LAUNCH(st, k_rs_special, dim3((unsigned)B), dim3(64), P, dP0, B, x0, s0, sol0, rows); // one wavefront per path
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));
   if (trace && !p0[0].status && (rc = rsTraceSum(ctx, 3, rows + p0[0].offOut * C, (int64_t)p0[0].nOut * C))) return rc;            // the points interpSpecial emitted
   for (int p = 0; p < B; ++p)
   {
      // ba.cpp:773-774: a walk that emitted fewer than four points is stretched onto four (point-major rows [i][C])
      RsPath &q = p0[p];
      if (q.status != RS_TOO_SHORT || q.nOut < 2 || q.nOut > 3) continue;
      std::vector<double> got((size_t)q.nOut * C), vals((size_t)q.nOut * C), four((size_t)4 * C), back((size_t)4 * C);
      HIP_TRY(hipMemcpy(got.data(), rows + q.offOut * C, sizeof(double) * got.size(), hipMemcpyDeviceToHost));
      for (int i = 0; i < q.nOut; ++i)
         for (int c = 0; c < C; ++c) vals[(size_t)c * q.nOut + i] = got[(size_t)i * C + c];
      stretchToFour(vals.data(), C, q.nOut, four.data());
      for (int i = 0; i < 4; ++i)
         for (int c = 0; c < C; ++c) back[(size_t)i * C + c] = four[(size_t)c * 4 + i];
      HIP_TRY(hipMemcpy(rows + q.offOut * C, back.data(), sizeof(double) * back.size(), hipMemcpyHostToDevice));
      q.sResNew = q.sResNew * (double)(q.nOut - 1) / 3.0; // traj.sres of the stretched stage
      q.nOut = 4;
      q.status = 0;
   }
   HIP_TRY(hipMemcpyAsync(dP0, p0.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st)); // (k_rs_transpose reads the point counts)

   // ---- stage 1: the points interpSpecial emitted -----------------------------------------------
   std::vector<RsPath> p1(B);
   int64_t tot1 = 0;
   for (int p = 0; p < B; ++p)
   {
      memset(&p1[p], 0, sizeof(RsPath));
      p1[p].off = tot1;
      p1[p].status = p0[p].status;
      p1[p].n = p0[p].status ? 4 : p0[p].nOut;
      p1[p].n0 = p1[p].n;
      p1[p].sres = p0[p].sResNew; // traj.sres = iv.sResNew, ba.cpp:768
      p1[p].sw1 = p0[p].sw1; p1[p].sw2 = p0[p].sw2; p1[p].scaleType = p0[p].scaleType; p1[p].integRes = p0[p].integRes; // members of the BA object
      tot1 += p1[p].n;
   }
   double *x1 = w.take<double>((size_t)tot1 * C), *sol1 = w.take<double>((size_t)tot1 * C);
   double *ta1 = w.take<double>((size_t)tot1), *ca1 = w.take<double>((size_t)tot1), *s1 = w.take<double>((size_t)tot1);
   if (w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "resample: chunk scratch estimate exceeded"); return BATOTP_ERR_STATE; }
   HIP_TRY(hipMemsetAsync(x1, 0, sizeof(double) * (size_t)tot1 * C, st));
   HIP_TRY(hipMemcpyAsync(dP1, p1.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
   RS_LAUNCH(st, k_rs_transpose, dim3((unsigned)((tot1 + bs - 1) / bs)), dim3(bs), C, dP0, dP1, B, rows, x1, tot1);
   if (cable) RS_LAUNCH(st, k_rs_invkin_cspr, dim3((unsigned)((tot1 + bs - 1) / bs)), dim3(bs), P, dP1, B, x1, tot1);
   if (kin && (rc = rsFwdKin(ctx, P, chain, hostTrig, p1, dP1, x1, tot1))) return rc; // ba.cpp:626-628
   P.thetaRes = prm->theta_norm_res2; P.cartRes = prm->cart_norm_res2;
   if ((rc = rsArcLengths(st, P, dP1, B, x1, ta1, ca1, s1, tot1, 0))) return rc;
   HIP_TRY(hipMemcpyAsync(p1.data(), dP1, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));
   if (trace && !p1[0].status && ((rc = rsTraceSum(ctx, 4, x1, (int64_t)p1[0].n * C)) || (rc = rsTraceSum(ctx, 5, s1, p1[0].n)))) return rc;   // stage 1: points, sites
   for (int p = 0; p < B; ++p) // what the sequential checks would have returned: the first one wins
      if (!p1[p].status && p1[p].pad) p1[p].status |= (p1[p].pad & 1) ? RS_SMALL_STEP : RS_SEG_ERROR;

   // ---- stage 2: the uniform knots ----------------------------------------------------------------
   std::vector<RsPath> p2(B);
   int64_t tot2 = 0;
   for (int p = 0; p < B; ++p)
   {
      memset(&p2[p], 0, sizeof(RsPath));
      p2[p].off = tot2;
      p2[p].status = p1[p].status;
      p2[p].n = p1[p].status ? 4 : p1[p].nOut;
      p2[p].n0 = p2[p].n;
      n2[p] = p2[p].n;
      // newRes = oldRes*(nPtsOld-1)/(nPtsNew-1), ba.cpp:799
      sresOut[p] = p1[p].status ? 0.0 : p1[p].sresNew * (p1[p].n - 1) / (p2[p].n - 1);
      statusOut[p] = (uint32_t)p1[p].status;
      autoOut[5 * p + 0] = p1[p].integRes; autoOut[5 * p + 1] = prm->s_weights[0]; autoOut[5 * p + 2] = p1[p].sw1; autoOut[5 * p + 3] = p1[p].sw2;
      autoOut[5 * p + 4] = (double)p1[p].scaleType;
      tot2 += p2[p].n;
   }
   // the knots go to the end of the context's knot workspace (grown, contents kept, if it is too small)
   {
      const void *before = ctx->ws[2].p;
      if ((rc = arenaReserve(ctx->ws[2], sizeof(double) * (size_t)(*yUsed + tot2 * C), st, sizeof(double) * (size_t)*yUsed))) return rc;
      if (ctx->ws[2].p != before && (rc = poisonFill(ctx, (char *)ctx->ws[2].p + sizeof(double) * (size_t)*yUsed, ctx->ws[2].cap - sizeof(double) * (size_t)*yUsed, st))) return rc;
   }
   double *y = (double *)ctx->ws[2].p + *yUsed;
   *yUsed += tot2 * C;
   HIP_TRY(hipMemsetAsync(y, 0, sizeof(double) * (size_t)tot2 * C, st));
   HIP_TRY(hipMemcpyAsync(dP2, p2.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
   if ((rc = rsSplines(ctx, p1, C, x1, sol1, dPinfo, dRedo))) return rc;
   RS_LAUNCH(st, k_rs_regular, dim3((unsigned)((tot2 + bs - 1) / bs)), dim3(bs), P, dP1, dP2, B, s1, x1, sol1, y, tot2);
   if (cable) RS_LAUNCH(st, k_rs_invkin_cspr, dim3((unsigned)((tot2 + bs - 1) / bs)), dim3(bs), P, dP2, B, y, tot2);
   if (kin && (rc = rsFwdKin(ctx, P, chain, hostTrig, p2, dP2, y, tot2))) return rc; // ba.cpp:626-628
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(st));
   if (trace && !p1[0].status && ((rc = rsTraceSum(ctx, 6, sol1, (int64_t)p1[0].n * C)) || (rc = rsTraceSum(ctx, 7, y, tot2 * C)))) return rc;   // stage 1's second derivatives, the knots
   return BATOTP_OK;
}
} // namespace

extern "C" int batotp_hip_resampled_destroy(batotp_resampled *r)
{
   delete r; // the knots belong to the context's workspace
   return BATOTP_OK;
}

// batotp_hip_resample and batotp_hip_resample_chain (kin_api.inc, which has checked the chain): chain == nullptr is the former
static int resampleRun(batotp_ctx *ctx, const batotp_resample_params *prm, const batotp_kin_chain *chain, int32_t n_paths, const int64_t *n_in, const double *x,
                       const double *sres_in, batotp_resampled **out)
{
   if (!ctx || !prm || !n_in || !x || !sres_in || !out || n_paths < 1) return BATOTP_ERR_ARG;
   *out = nullptr;
   // joints and Cartesian rows taught together (path type BOTH; reference ba.cpp:184-192, 245-262: nothing is recomputed, both channel
   // sets are resampled as taught).  Six Cartesian rows are tool poses (the UR5 example): 6 rows come in, 7 go on (quaternions); any
   // other count -- tool positions without orientations -- goes through unchanged
   const bool both = prm->path_type == BATOTP_PATH_BOTH;
   const bool pose = both && prm->n_cart == 6;
   const int nJ = prm->n_joints, nCin = prm->n_cart, nC = nCin + (pose ? 1 : 0), C = nJ + nC, B = n_paths;
   if (nJ < 1 || nJ > BATOTP_MAX_JOINTS || nC < 3 || nC > BATOTP_MAX_CART) return BATOTP_ERR_ARG;
   if (nJ > 8 || nC > 8) { snprintf(g_err, sizeof(g_err), "resample: the walk kernel carries at most 8 joints and 8 Cartesian channels"); return BATOTP_ERR_ARG; }
   // (with a chain the Cartesian rows of the caller are not read either: zero until the chain's tool point replaces them)
   const bool joint = prm->path_type == BATOTP_PATH_JOINT && (prm->robot_type == BATOTP_ROBOT_GENJNT || chain);
   const bool cable = prm->path_type == BATOTP_PATH_CART && prm->robot_type == BATOTP_ROBOT_CSPR3DOF && nJ == 3;
   // JOINT paths of the robots with forward kinematics (KUKA, RR; SURVEY.md 8 f-3), or of any robot with a kinematic chain
   const bool kin = prm->path_type == BATOTP_PATH_JOINT && (chain || fwdkin_trig_rows(prm->robot_type, nJ) != 0);
   const bool hostTrig = (kin || pose) && (prm->flags & BATOTP_F_HOST_TRIG) != 0;
   const bool cartOn = (prm->flags & (BATOTP_F_CART_VEL_ON | BATOTP_F_CART_ACC_ON)) != 0;
   if (!joint && !cable && !kin && !both) { snprintf(g_err, sizeof(g_err), "resample: path/robot kind not supported on the device"); return BATOTP_ERR_ARG; }
   if (prm->scale_type < 0 || prm->scale_type > 2) return BATOTP_ERR_ARG;
   if (prm->s_weights[1] + prm->s_weights[2] < 1e-8) { snprintf(g_err, sizeof(g_err), "resample: s follows the input nodes, nothing to resample"); return BATOTP_ERR_ARG; }
   for (int p = 0; p < B; ++p)
      if (n_in[p] < 4 || n_in[p] > (int64_t)1 << 30) return BATOTP_ERR_ARG;
   int rc = bind(ctx);
   if (rc) return rc;
   hipStream_t st = ctx->stream;
   ++ctx->rsEpoch;
   for (int k = 0; k < 8; ++k) ctx->rsTraceSums[k] = 0;

   RsParams P;
   memset(&P, 0, sizeof(P));
   P.nJ = nJ; P.nC = nC; P.C = C;
   P.pathType = prm->path_type; P.scaleType = prm->scale_type; P.robot = prm->robot_type;
   P.cartEval = (prm->flags & (BATOTP_F_CART_VEL_ON | BATOTP_F_CART_ACC_ON)) ? 1 : 0;
   for (int k = 0; k < 3; ++k) P.sW[k] = prm->s_weights[k];
   for (int k = 0; k < 9; ++k) P.pmat[k] = prm->pmat[k];
   P.autoOn = (prm->flags & BATOTP_RS_AUTO_INTEG_RES) ? 1 : 0;
   P.degrees = prm->degrees;
   for (int j = 0; j < 8; ++j) { P.vmax[j] = prm->jnt_vel_max[j]; P.amax[j] = prm->jnt_acc_max[j]; }
   P.cartVelMax = prm->cart_vel_max; P.cartAccMax = prm->cart_acc_max; P.quadThresh = prm->quad_rad_thresh;
   P.thresh = cable ? prm->cart_thresh : prm->jnt_thresh;

   hipEvent_t ev0 = nullptr, ev1 = nullptr;
   HIP_TRY(hipEventCreate(&ev0));
   HIP_TRY(hipEventCreate(&ev1));
   struct EvGuard { hipEvent_t a, b; ~EvGuard() { hipEventDestroy(a); hipEventDestroy(b); } } evGuard{ev0, ev1};

   // ---- stage 0a, all paths: close points, kinematics, arc lengths -> how many points each path emits
   std::vector<RsPath> p0(B);
   int64_t tot0 = 0;
   for (int p = 0; p < B; ++p)
   {
      memset(&p0[p], 0, sizeof(RsPath));
      p0[p].off = tot0; p0[p].n = (int32_t)n_in[p]; p0[p].n0 = p0[p].n; p0[p].sres = sres_in[p];
      p0[p].sw1 = prm->s_weights[1]; p0[p].sw2 = prm->s_weights[2]; p0[p].scaleType = prm->scale_type;
      tot0 += n_in[p];
   }
   const int decim = prm->input_decim_fact > 1 ? prm->input_decim_fact : 1;
   const bool preFilter = decim > 1 || prm->smooth_window > 1; // input decimation / smoothing, ba.cpp:195-242
   const size_t need0 = granule(8 * (size_t)tot0 * C) * (preFilter ? 2 : 1) + 3 * granule(8 * (size_t)tot0) + granule((size_t)tot0) +
                        2 * granule(sizeof(RsPath) * B) + granule(sizeof(int) * (size_t)B);
   if ((rc = arenaReserve(ctx->ws[0], need0, st))) return rc;
   if ((rc = poisonFill(ctx, ctx->ws[0].p, ctx->ws[0].cap, st))) return rc;
   Bump w0;
   w0.base = (char *)ctx->ws[0].p;
   double *x0 = w0.take<double>((size_t)tot0 * C), *ta0 = w0.take<double>((size_t)tot0), *ca0 = w0.take<double>((size_t)tot0);
   double *s0 = w0.take<double>((size_t)tot0);
   unsigned char *drop = w0.take<unsigned char>((size_t)tot0);
   RsPath *dP0 = w0.take<RsPath>((size_t)B), *dP0b = w0.take<RsPath>((size_t)B);
   int *closeFlag = w0.take<int>((size_t)B);
   double *xs = preFilter ? w0.take<double>((size_t)tot0 * C) : nullptr;
   std::vector<double> xWide;
   if (pose)
   {
      // the caller's rows [nJ + 6][n] per path, widened by the (empty) seventh Cartesian row
      xWide.assign((size_t)tot0 * C, 0.0);
      size_t src = 0, dst = 0;
      for (int p = 0; p < B; ++p)
      {
         const size_t cnt = (size_t)n_in[p] * (size_t)(nJ + nCin);
         std::copy(x + src, x + src + cnt, xWide.begin() + dst);
         src += cnt; dst += (size_t)n_in[p] * C;
      }
      HIP_TRY(hipMemcpyAsync(x0, xWide.data(), sizeof(double) * xWide.size(), hipMemcpyHostToDevice, st));
   }
   else HIP_TRY(hipMemcpyAsync(x0, x, sizeof(double) * (size_t)tot0 * C, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(dP0, p0.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
   HIP_TRY(hipEventRecord(ev0, st));
   const int bs = 256;
   if (joint)
   {
      // JOINT path on a robot without kinematic model: the Cartesian rows are zero (ba.cpp:258-262)
      RS_LAUNCH(st, k_rs_zero_cart, dim3((unsigned)((tot0 + bs - 1) / bs)), dim3(bs), P, dP0, B, x0, tot0);
   }
   HIP_TRY(hipMemsetAsync(closeFlag, 0, sizeof(int) * (size_t)B, st));
   RS_LAUNCH(st, k_rs_close_any, dim3((unsigned)((tot0 + bs - 1) / bs)), dim3(bs), P, dP0, B, x0, closeFlag, tot0);
   RS_LAUNCH(st, k_rs_remclose, dim3((unsigned)((B + 63) / 64)), dim3(64), P, dP0, B, x0, drop, closeFlag);
   {
      // ba.cpp:176-183: one point left = nothing to optimise; two or three are stretched onto four (BA::interpTrajLinear)
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      bool touched = false;
      for (int p = 0; p < B; ++p)
      {
         RsPath &q = p0[p];
         if (q.status != RS_TOO_SHORT || q.n < 2 || q.n > 3) continue;
         std::vector<double> vals((size_t)q.n * C), four((size_t)4 * C);
         HIP_TRY(hipMemcpy(vals.data(), x0 + q.off * C, sizeof(double) * vals.size(), hipMemcpyDeviceToHost)); // rows repacked to stride n
         stretchToFour(vals.data(), C, q.n, four.data());
         HIP_TRY(hipMemcpy(x0 + q.off * C, four.data(), sizeof(double) * four.size(), hipMemcpyHostToDevice));
         q.sres = q.sres * (double)(q.n - 1) / 3.0;
         q.n = 4;
         q.status = 0;
         touched = true;
      }
      if (touched) HIP_TRY(hipMemcpyAsync(dP0, p0.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
   }
   if (pose)
   {
      // BA::aa2qVect (ba.cpp:186-193, 327-369): orientations as hemisphere-aligned quaternions from here on
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st)); // point counts after remClosePts
      HIP_TRY(hipStreamSynchronize(st));
      const unsigned gridPts = (unsigned)((tot0 + bs - 1) / bs);
      const double *trigDev = nullptr;
      if (hostTrig)
      {
         if ((rc = arenaReserve(ctx->ws[3], sizeof(double) * (size_t)tot0 * 3 + 512, st))) return rc;
         if ((rc = poisonFill(ctx, ctx->ws[3].p, ctx->ws[3].cap, st))) return rc;
         double *ang = (double *)ctx->ws[3].p, *trig = ang + tot0;
         RS_LAUNCH(st, k_rs_aa_norm, dim3(gridPts), dim3(bs), P, dP0, B, x0, ang, tot0);
         ctx->kinTheta.resize((size_t)tot0);
         ctx->kinTrig.resize((size_t)tot0 * 2);
         HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), ang, sizeof(double) * (size_t)tot0, hipMemcpyDeviceToHost, st));
         HIP_TRY(hipStreamSynchronize(st));
         for (int p = 0; p < B; ++p)
         {
            // sine and cosine of half the rotation angle: one glibc sincos() per point (util.cpp:547-548 as the reference's
            // optimised build calls it)
            const int64_t off = p0[p].off, n = p0[p].n;
            for (int64_t i = 0; i < n; ++i)
               ::sincos(0.5 * ctx->kinTheta[(size_t)(off + i)], &ctx->kinTrig[(size_t)(off * 2 + i)], &ctx->kinTrig[(size_t)(off * 2 + n + i)]);
         }
         HIP_TRY(hipMemcpyAsync(trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, st));
         trigDev = trig;
      }
      RS_LAUNCH(st, k_rs_aa2q, dim3(gridPts), dim3(bs), P, dP0, B, x0, trigDev, tot0);
      RS_LAUNCH(st, k_rs_qalign, dim3((unsigned)((B + 63) / 64)), dim3(64), P, dP0, B, x0);
      HIP_TRY(hipGetLastError());
      if (hostTrig) HIP_TRY(hipStreamSynchronize(st));
   }
   if (preFilter)
   {
      // smooth + decimate the driving rows (joints of a JOINT path, Cartesian rows of a CART path), then the second
      // smoothing -- which, as in the reference, also takes _inputDecimFact as its window
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      const int c0 = cable ? nJ : 0, cN = cable ? nC : (both ? C : nJ);   // BOTH: joints and poses are both driving rows
      const unsigned gridPts = (unsigned)((tot0 + bs - 1) / bs);
      if (decim > 1)
      {
         RS_LAUNCH(st, k_rs_smooth, dim3(gridPts), dim3(bs), P, dP0, B, x0, xs, c0, cN, decim, tot0);
         std::vector<RsPath> pb(p0);
         for (int p = 0; p < B; ++p)
         {
            if (pb[p].status) continue;
            pb[p].n = (pb[p].n - 1) / decim + 1;
            pb[p].sres = pb[p].sres * decim; // traj.sres *= _inputDecimFact, ba.cpp:218
            if (pb[p].n < 4) pb[p].status |= RS_TOO_SHORT;
         }
         HIP_TRY(hipMemcpyAsync(dP0b, pb.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
         RS_LAUNCH(st, k_rs_decimate, dim3(gridPts), dim3(bs), P, dP0, dP0b, B, xs, x0, decim, tot0);
         HIP_TRY(hipGetLastError());
         HIP_TRY(hipStreamSynchronize(st)); // pb leaves scope; dP0 is rewritten
         p0 = pb;
         HIP_TRY(hipMemcpyAsync(dP0, p0.data(), sizeof(RsPath) * B, hipMemcpyHostToDevice, st));
      }
      if (prm->smooth_window > 1)
      {
         RS_LAUNCH(st, k_rs_smooth, dim3(gridPts), dim3(bs), P, dP0, B, x0, xs, c0, cN, decim, tot0);
         HIP_TRY(hipMemcpyAsync(x0, xs, sizeof(double) * (size_t)tot0 * C, hipMemcpyDeviceToDevice, st));
      }
   }
   if (cable) RS_LAUNCH(st, k_rs_invkin_cspr, dim3((unsigned)((tot0 + bs - 1) / bs)), dim3(bs), P, dP0, B, x0, tot0);
   if (kin && cartOn)
   {
      // ba.cpp:247-256: with a Cartesian constraint on, the tool point of the taught points (otherwise their Cartesian rows
      // stay as loaded until the first pass has run)
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st)); // point counts after remClosePts
      HIP_TRY(hipStreamSynchronize(st));
      if ((rc = rsFwdKin(ctx, P, chain, hostTrig, p0, dP0, x0, tot0))) return rc;
   }
   P.thetaRes = prm->theta_norm_res; P.cartRes = prm->cart_norm_res;
   if ((rc = rsArcLengths(st, P, dP0, B, x0, ta0, ca0, s0, tot0, 1))) return rc;
   HIP_TRY(hipMemcpyAsync(p0.data(), dP0, sizeof(RsPath) * B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));

   // ---- the rest in chunks of paths: the scratch of a chunk is bounded (the temporaries of a path are
   //      ~4x its knots); one workspace serves all chunks
   size_t freeB = 0, totalB = 0;
   HIP_TRY(hipMemGetInfo(&freeB, &totalB));
   double budget = 0.25 * (double)(freeB + ctx->ws[1].cap);
   if (budget > 48.0 * 1073741824.0) budget = 48.0 * 1073741824.0;
   if (ctx->rsBudget > 0) budget = (double)ctx->rsBudget; // batotp_hip_set_workspace_budget: the caller bounds the scratch memory
   std::vector<int> cuts;
   const size_t maxChunk = cutRanges(B, [&](int p) { return chunkBytesOfPath(p0[p], C); }, budget, cuts);
   if ((rc = arenaReserve(ctx->ws[1], maxChunk, st))) return rc;
   // knots: first guess from the planned counts; rsChunk grows the workspace if a chunk does not fit
   {
      double est = 0;
      for (int p = 0; p < B; ++p) est += p0[p].status ? 4 : (double)p0[p].nOut;
      if ((rc = arenaReserve(ctx->ws[2], (size_t)(est * 1.02 * C * 8.0) + 4096, st))) return rc;
      if ((rc = poisonFill(ctx, ctx->ws[2].p, ctx->ws[2].cap, st))) return rc;
   }

   batotp_resampled *r = new (std::nothrow) batotp_resampled;
   if (!r) return BATOTP_ERR_ALLOC;
   r->ctx = ctx; r->B = B; r->C = C;
   r->n.resize(B); r->off.resize(B); r->sres.resize(B); r->status.resize(B); r->au.assign((size_t)B * 5, 0.0);
   int64_t yUsed = 0;
   for (size_t k = 0; k + 1 < cuts.size(); ++k)
   {
      const int pa = cuts[k], pb = cuts[k + 1];
      std::vector<RsPath> pc(p0.begin() + pa, p0.begin() + pb);
      const int64_t base = p0[pa].off;
      for (RsPath &q : pc) q.off -= base;
      rc = rsChunk(ctx, P, prm, chain, cable, kin, hostTrig, pc, x0 + base * C, s0 + base, &yUsed, r->n.data() + pa, r->sres.data() + pa, r->status.data() + pa,
                   r->au.data() + 5 * (size_t)pa);
      if (rc) { delete r; return rc; }
   }
   int64_t tot2 = 0;
   for (int p = 0; p < B; ++p) { r->off[p] = tot2; tot2 += r->n[p]; }
   r->total = tot2;
   r->nChunks = (int)cuts.size() - 1;
   r->traced = ctx->rsTrace && B == 1;
   for (int k = 0; k < 8; ++k) { r->trace[k] = ctx->rsTraceSums[k]; r->traceData[k].swap(ctx->rsTraceData[k]); ctx->rsTraceData[k].clear(); }
   r->dY = (double *)ctx->ws[2].p;
   r->epoch = ctx->rsEpoch;
   hipError_t e = hipEventRecord(ev1, st);
   if (e == hipSuccess) e = hipStreamSynchronize(st);
   if (e == hipSuccess) e = hipEventElapsedTime(&r->ms, ev0, ev1);
   if (e != hipSuccess) { delete r; return hipFail(e, "resample timing"); }
   *out = r;
   return BATOTP_OK;
}

extern "C" int batotp_hip_resample(batotp_ctx *ctx, const batotp_resample_params *prm, int32_t n_paths, const int64_t *n_in, const double *x,
                                   const double *sres_in, batotp_resampled **out)
{
   return resampleRun(ctx, prm, nullptr, n_paths, n_in, x, sres_in, out);
}

static int rsLive(batotp_resampled *r)
{
   if (r->epoch != r->ctx->rsEpoch || r->dY != (double *)r->ctx->ws[2].p)
   {
      snprintf(g_err, sizeof(g_err), "resampled knots are no longer valid (a later batotp_hip_resample / ctx_trim reused the workspace)");
      return BATOTP_ERR_STATE;
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_info(batotp_resampled *r, int64_t *n_knots, double *sres, uint32_t *status)
{
   if (!r) return BATOTP_ERR_ARG;
   for (int p = 0; p < r->B; ++p)
   {
      if (n_knots) n_knots[p] = r->n[p];
      if (sres) sres[p] = r->sres[p];
      if (status) status[p] = r->status[p];
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_auto(batotp_resampled *r, double *integ_res, double *s_weights, int32_t *scale_type)
{
   if (!r) return BATOTP_ERR_ARG;
   for (int p = 0; p < r->B; ++p)
   {
      if (integ_res) integ_res[p] = r->au[5 * (size_t)p];
      if (s_weights) for (int k = 0; k < 3; ++k) s_weights[3 * (size_t)p + k] = r->au[5 * (size_t)p + 1 + k];
      if (scale_type) scale_type[p] = (int32_t)r->au[5 * (size_t)p + 4];
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_knots_device(batotp_resampled *r, const double **y_dev, int64_t *n_doubles)
{
   if (!r || !y_dev) return BATOTP_ERR_ARG;
   int rc = rsLive(r);
   if (rc) return rc;
   *y_dev = r->dY;
   if (n_doubles) *n_doubles = r->total * r->C;
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_download(batotp_resampled *r, int32_t path, double *y)
{
   if (!r || !y || path < 0 || path >= r->B) return BATOTP_ERR_ARG;
   int rc = rsLive(r);
   if (rc) return rc;
   if ((rc = bind(r->ctx))) return rc;
   HIP_TRY(hipMemcpyAsync(y, r->dY + r->off[path] * r->C, sizeof(double) * (size_t)(r->n[path] * r->C), hipMemcpyDeviceToHost, r->ctx->stream));
   HIP_TRY(hipStreamSynchronize(r->ctx->stream));
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_checksums(batotp_resampled *r, uint64_t *sums)
{
   if (!r || !sums) return BATOTP_ERR_ARG;
   int rc = rsLive(r);
   if (rc) return rc;
   if ((rc = bind(r->ctx))) return rc;
   hipStream_t st = r->ctx->stream;
   const int B = r->B;
   struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } } d;
   HIP_TRY(hipMalloc(&d.p, sizeof(int64_t) * 3 * (size_t)B));
   int64_t *dOff = (int64_t *)d.p, *dN = dOff + B;
   unsigned long long *dOut = (unsigned long long *)(dN + B);
   std::vector<int64_t> nLive(r->n);
   for (int p = 0; p < B; ++p)
      if (r->status[p]) nLive[p] = 0;     // a failed path has no knots: its checksum is 0
   HIP_TRY(hipMemcpyAsync(dOff, r->off.data(), sizeof(int64_t) * (size_t)B, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(dN, nLive.data(), sizeof(int64_t) * (size_t)B, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemsetAsync(dOut, 0, sizeof(unsigned long long) * (size_t)B, st));
   int64_t nMax = 1;
   for (int p = 0; p < B; ++p) nMax = std::max<int64_t>(nMax, nLive[p] * r->C);
   const unsigned bx = (unsigned)std::min<int64_t>(64, (nMax + 256 * 8 - 1) / (256 * 8));
   for (int p0 = 0; p0 < B; p0 += 65535)   // (gridDim.y limit)
   {
      const int m = std::min(B - p0, 65535);
      RS_LAUNCH(st, k_rs_checksum, dim3(std::max(bx, 1u), (unsigned)m), dim3(256), dOff + p0, dN + p0, r->C, r->dY, dOut + p0);
   }
   static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "64-bit sums");
   HIP_TRY(hipMemcpyAsync(sums, dOut, sizeof(uint64_t) * (size_t)B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_trace(batotp_resampled *r, uint64_t *sums)
{
   if (!r || !sums) return BATOTP_ERR_ARG;
   if (!r->traced) return BATOTP_ERR_STATE;
   for (int k = 0; k < 8; ++k) sums[k] = r->trace[k];
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_trace_data(batotp_resampled *r, int32_t stage, double *out, int64_t cap, int64_t *count)
{
   if (!r || stage < 0 || stage > 7 || !count) return BATOTP_ERR_ARG;
   if (!r->traced) return BATOTP_ERR_STATE;
   *count = (int64_t)r->traceData[stage].size();
   if (out)
   {
      if (cap < *count) return BATOTP_ERR_ARG;
      std::copy(r->traceData[stage].begin(), r->traceData[stage].end(), out);
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_resampled_ms(batotp_resampled *r, float *ms)
{
   if (!r || !ms) return BATOTP_ERR_ARG;
   *ms = r->ms;
   return BATOTP_OK;
}
