// output_api.inc -- host side of batotp_hip_output (included at the end of batotp_hip.hip).
// All sizes of the stage follow from the results of the forward sweep (points and time step of each curve), so
// the host lays out every buffer before the first kernel; the paths of a call are processed in chunks whose
// scratch fits the context's cached workspace.

struct batotp_output
{
   batotp_ctx *ctx = nullptr;
   int32_t K = 0;
   int nJ = 0;                  // rows per point: theta + cart + trq
   int nTheta = 0, nCart = 0, nTrq = 0;
   std::vector<int64_t> n, off; // points per path, first point of the path in dTheta (points, not doubles)
   std::vector<double> sres;
   double *dTheta = nullptr;    // path after path, [nJ][n] each (nJ = rows per point)
   int64_t total = 0;
   float ms = 0.f;
};

extern "C" int batotp_hip_output_destroy(batotp_output *o)
{
   if (!o) return BATOTP_OK;
   if (o->ctx) hipSetDevice(o->ctx->device);
   if (o->dTheta) hipFree(o->dTheta);
   delete o;
   return BATOTP_OK;
}

// k_out_segmax is ONE WAVEFRONT PER PATH (output.hip.h): the stage and the known-answer entry below launch it through this function, so
// that a test of the entry point is a test of the grid the stage uses (round 5 shipped the wavefront kernel on the old lane-per-path grid:
// only the first ceil(K / 64) paths of a chunk got their running maximum, and no test saw it because every test curve was monotone)
static void launchOutSegmax(hipStream_t st, const OutPath *dPaths, int K, int *segK)
{
   hipLaunchKernelGGL(k_out_segmax, dim3((unsigned)K), dim3(64), 0, st, dPaths, K, segK);
}

// known-answer test of that step (reference batotp/spline.cpp:56-99, findInterpSegs: the cursor never moves back): seg holds the raw
// segment indices of n_paths paths back to back (n1[k] sites each) and comes back as their running maxima
extern "C" int batotp_hip_out_segmax_kat(batotp_ctx *ctx, int32_t n_paths, const int32_t *n1, int32_t *seg)
{
   if (!ctx || n_paths < 1 || !n1 || !seg) return BATOTP_ERR_ARG;
   int rc = bind(ctx);
   if (rc) return rc;
   std::vector<OutPath> pc((size_t)n_paths);
   int64_t total = 0;
   for (int k = 0; k < n_paths; ++k)
   {
      if (n1[k] < 0) return BATOTP_ERR_ARG;
      memset(&pc[k], 0, sizeof(OutPath));
      pc[k].off1 = total; pc[k].n1 = n1[k]; pc[k].p = k;
      total += n1[k];
   }
   if (total < 1 || total > (int64_t)1 << 30) return BATOTP_ERR_ARG;
   struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } } dP, dS;
   hipStream_t st = ctx->stream;
   HIP_TRY(hipMalloc(&dP.p, sizeof(OutPath) * (size_t)n_paths));
   HIP_TRY(hipMalloc(&dS.p, sizeof(int) * (size_t)total));
   HIP_TRY(hipMemcpyAsync(dP.p, pc.data(), sizeof(OutPath) * (size_t)n_paths, hipMemcpyHostToDevice, st));
   HIP_TRY(hipMemcpyAsync(dS.p, seg, sizeof(int) * (size_t)total, hipMemcpyHostToDevice, st));
   launchOutSegmax(st, (const OutPath *)dP.p, n_paths, (int *)dS.p);
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipMemcpyAsync(seg, dS.p, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));
   return BATOTP_OK;
}

extern "C" int batotp_hip_output(batotp_batch *b, const batotp_output_params *prm, int32_t path0, int32_t n_paths, batotp_output **out)
{
   if (!b || !prm || !out || path0 < 0 || n_paths < 1 || path0 + n_paths > b->B) return BATOTP_ERR_ARG;
   *out = nullptr;
   const bool cable = prm->path_type == BATOTP_PATH_CART && b->prob.robot_type == BATOTP_ROBOT_CSPR3DOF && prm->n_joints == 3 &&
                      b->prob.n_cart == 3 && (b->prob.flags & BATOTP_F_TRQ_ON) && (b->prob.flags & BATOTP_F_PARALLEL);
   const bool jointPath = prm->path_type == BATOTP_PATH_JOINT || prm->path_type == 0;
   // JOINT path of a robot with forward kinematics (KUKA, RR; SURVEY.md 8 f-3): three Cartesian rows from the joint rows
   const int trigRows = fwdkin_trig_rows(b->prob.robot_type, prm->n_joints);
   const bool kin = jointPath && trigRows != 0 && b->prob.n_cart >= 3;
   // torque recomputation of a serial robot (ba.cpp:1791-1827): the two-link arm's closed form or the batch's chain model
   const bool serialTrq = jointPath && (b->prob.flags & BATOTP_F_TRQ_ON) && !(b->prob.flags & BATOTP_F_PARALLEL) &&
                          (b->hasSerial || b->prob.robot_type == BATOTP_ROBOT_RR);
   const bool jointMode = jointPath && (!(b->prob.flags & BATOTP_F_TRQ_ON) || serialTrq);
   // joints and Cartesian rows taught together (path type BOTH): the Cartesian rows are evaluated like the joints (ba.cpp:1726-1736);
   // seven of them are position + quaternion (what aa2qVect left) and are turned back into axis-angle at the very end (ba.cpp:1920-1927)
   const bool both = prm->path_type == BATOTP_PATH_BOTH && b->prob.n_cart >= 3 && b->prob.n_cart <= BATOTP_MAX_CART && !(b->prob.flags & BATOTP_F_TRQ_ON);
   const bool pose = both && b->prob.n_cart == 7;
   if ((!cable && !jointMode && !both) || prm->n_joints != b->P.nJ || !(prm->out_res > 0) || !(prm->integ_res > 0 || prm->integ_res == BATOTP_OUT_STEP_PER_PATH) || !(prm->out_smooth_fact >= 1) ||
       (kin && b->prob.robot_type == BATOTP_ROBOT_RR && (b->prob.flags & BATOTP_F_NO_SAMPLES)))
   {
      snprintf(g_err, sizeof(g_err), "output stage: configuration not supported on the device");
      return BATOTP_ERR_ARG;
   }
   // the integration step is a property of the path (batotp_hip_set_path_integ_res).  BATOTP_OUT_STEP_PER_PATH samples every path of
   // the range with its own; a positive integ_res is a statement about the whole range and is refused where a path disagrees
   const bool perPath = prm->integ_res == BATOTP_OUT_STEP_PER_PATH;
   for (int k = 0; k < n_paths && !perPath; ++k)
   {
      const double h = b->pinfo[path0 + k].integ_res;
      if (h != prm->integ_res)
      {
         snprintf(g_err, sizeof(g_err), "output stage: path %d integrates with step %.17g, the parameters say %.17g", path0 + k, h, prm->integ_res);
         return BATOTP_ERR_ARG;
      }
   }
   const bool hostTrig = (b->prob.flags & BATOTP_F_HOST_TRIG) != 0;
   if (!b->revDone) return BATOTP_ERR_STATE;
   int rc = bind(b->ctx);
   if (rc) return rc;
   batotp_ctx *ctx = b->ctx;
   hipStream_t st = ctx->stream;
   const int K = n_paths, nJ = b->P.nJ;
   const int nCartRows = cable ? 3 : (both ? (int)b->prob.n_cart : (kin ? 3 : 0)), nTrqRows = cable ? 3 : (serialTrq ? nJ : 0);
   const int R = nJ + nCartRows + nTrqRows; // rows per point the stage works with: joints (+ Cartesian + torques)
   const int Rout = pose ? R - 1 : R;       // rows per point of the result (poses leave as position + axis-angle)

   // ba.cpp:1668-1675: never sample finer than the integration step; smooth + re-interpolate afterwards.  All of it follows from
   // the step, so it is a property of the path; `route` (re-interpolated or not, smoothed or not) decides which stages a path
   // passes and which buffers they need.  A NaN step compares false: such a path has no forward curve and takes no route at all.
   struct OutStep { double h, outRes, smoothFact; bool reinterp, smoothing; int route; };
   const double outResUser = prm->out_res;
   auto stepOf = [&](double h) {
      OutStep s{h, prm->out_res, prm->out_smooth_fact, false, false, 0};
      if (s.outRes < h)
      {
         s.reinterp = true;
         s.outRes = h;
         s.smoothFact *= std::max(outResUser / s.outRes, 1.);
      }
      s.smoothing = s.smoothFact > 1.5;
      s.route = (s.reinterp ? 2 : 0) | (s.smoothing ? 1 : 0);
      return s;
   };
   std::vector<OutStep> step(K);
   for (int k = 0; k < K; ++k) step[k] = stepOf(perPath ? b->pinfo[path0 + k].integ_res : prm->integ_res);

   std::vector<batotp_path_result> res(b->B);
   HIP_TRY(hipMemcpyAsync(res.data(), b->dRes, sizeof(batotp_path_result) * b->B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));

   batotp_output *o = new (std::nothrow) batotp_output;
   if (!o) return BATOTP_ERR_ALLOC;
   o->ctx = ctx; o->K = K; o->nJ = Rout; o->nTheta = nJ; o->nCart = pose ? 6 : nCartRows; o->nTrq = nTrqRows;
   o->n.assign(K, 0); o->off.assign(K, 0); o->sres.assign(K, 0.0);
   std::vector<OutPath> all(K);
   int64_t totF = 0;
   unsigned routesLive = 0; // routes taken by the paths of the range that have a trajectory
   for (int k = 0; k < K; ++k)
   {
      OutPath &q = all[k];
      const OutStep &S = step[k];
      const double outRes = S.outRes, smoothFact = S.smoothFact;
      const bool reinterp = S.reinterp, smoothing = S.smoothing;
      memset(&q, 0, sizeof(q));
      const batotp_path_result &r = res[path0 + k];
      const uint32_t stt = r.status_rev | r.status_fwd;
      q.p = path0 + k;
      q.offF = totF;
      o->off[k] = totF;
      if (r.n_fwd < 4 || !(S.h > 0) || (stt & (BATOTP_ST_MAX_INTEG_TIME | BATOTP_ST_CAPACITY | BATOTP_ST_NONFINITE))) continue;
      q.nFwd = (int32_t)r.n_fwd;
      q.tStep = (r.status_fwd & BATOTP_ST_SHORT) ? r.t_total / 3. : S.h;
      const double tLast = q.tStep * (double)(q.nFwd - 1);
      int nOut = (int)(smoothFact * std::ceil(tLast / outRes + 1.)); // ba.cpp:1683
      nOut = std::max(nOut, 4);
      q.n1 = nOut;
      q.n2 = smoothing ? std::max((int)((nOut - 1) / smoothFact) + 1, 4) : nOut; // ba.cpp:1841
      q.nF = reinterp ? std::max((int)(std::ceil(tLast / outResUser)), 4) : q.n2;  // ba.cpp:1876
      o->n[k] = q.nF;
      o->sres[k] = reinterp ? outResUser : outRes;
      q.window = smoothing ? (int)smoothFact : 0;
      const double tfact = outRes / smoothFact; // traj.sres/_outSmoothFact, ba.cpp:1754
      q.vfactT = 1.0 / tfact;
      q.afactT = q.vfactT * q.vfactT;
      routesLive |= 1u << S.route;
      totF += q.nF;
   }
   // more than one route in the range: the chunks that mix them stage their results (see the chunk loop)
   const bool mixedCall = (routesLive & (routesLive - 1)) != 0;
   o->total = totF;
   hipError_t e = hipMalloc((void **)&o->dTheta, sizeof(double) * (size_t)std::max<int64_t>(totF * Rout, 1));
   if (e != hipSuccess)
   {
      delete o;
      hipFail(e, "hipMalloc (output trajectories)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, o->dTheta, sizeof(double) * (size_t)std::max<int64_t>(totF * Rout, 1), st))) { batotp_hip_output_destroy(o); return rc; }

   OutParams P;
   memset(&P, 0, sizeof(P));
   P.nJ = nJ; P.R = R; P.compact = b->compact ? 1 : 0; P.kmC = b->kmC;
   P.C = b->P.C; P.Cin = b->P.Cin; P.svd = (b->prob.flags & BATOTP_F_SVD) ? 1 : 0;
   for (int k = 0; k < 9; ++k) P.pmat[k] = b->prob.pmat[k];

   // scratch of one path: s(t) second derivatives | sOut, segment | th1 (unless final) | th2 (if a middle stage) | sol2
   auto scratchOf = [&](const OutPath &q, const OutStep &S) -> size_t {
      const bool smoothing = S.smoothing, reinterp = S.reinterp;
      size_t by = 8 * (size_t)q.nFwd + 12 * (size_t)q.n1 + 8 * 256 + sizeof(OutPath) + 2 * sizeof(int64_t) * (1 + R) + 2 * sizeof(int) * (1 + R);
      if (smoothing || reinterp) by += 8 * (size_t)R * q.n1;
      if (smoothing && reinterp) by += 8 * (size_t)R * q.n2;
      if (reinterp) by += 8 * (size_t)R * q.n2;
      if (cable || serialTrq) by += 2 * 8 * (size_t)R * q.n1; // samples before the torque step and their second derivatives
      if (pose) by += 8 * (size_t)(R + 3) * q.nF + 1024;      // final rows before the pose conversion, (norm, q0) pairs, atan2 table
      else if (mixedCall) by += 8 * (size_t)R * q.nF;         // staged final rows of a chunk that mixes routes
      return by;
   };
   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   std::vector<int> cuts(1, 0);
   size_t maxChunk = 0;
   {
      size_t bytes = 0;
      for (int k = 0; k < K; ++k)
      {
         const size_t need = scratchOf(all[k], step[k]);
         if (k > cuts.back() && (double)(bytes + need) > budget) { cuts.push_back(k); bytes = 0; }
         bytes += need;
         maxChunk = std::max(maxChunk, bytes);
      }
      cuts.push_back(K);
   }
#define OUT_TRY(call)                                                              \
   do                                                                              \
   {                                                                               \
      hipError_t e_ = (call);                                                      \
      if (e_ != hipSuccess) { batotp_hip_output_destroy(o); return hipFail(e_, #call); } \
   } while (0)
   if ((rc = arenaReserve(ctx->ws[1], maxChunk + 4096, st))) { batotp_hip_output_destroy(o); return rc; }
   hipEvent_t ev0 = nullptr, ev1 = nullptr;
   OUT_TRY(hipEventCreate(&ev0));
   OUT_TRY(hipEventCreate(&ev1));
   struct EvGuard { hipEvent_t a, b; ~EvGuard() { hipEventDestroy(a); hipEventDestroy(b); } } evGuard{ev0, ev1};
   OUT_TRY(hipEventRecord(ev0, st));
   const int bs = 256;
   // natural-spline second derivatives of `series` series (descriptors in dYOff / dSOff / dCnt): a wavefront per series where the
   // series is long enough (spline_lanes.hip.h) and there are few of them (seriesLanesPay), the lane-per-series kernel for the rest
   auto solveSeries = [&](int series, const int64_t *dYOff, const int64_t *dSOff, const int *dCnt, int *dRedo, const double *y, int ys, double *sol) {
      const bool byLanes = seriesLanesPay(series);
      if (byLanes) hipLaunchKernelGGL(k_spline_series_lanes, dim3((unsigned)series), dim3(64), 0, st, series, dYOff, dSOff, dCnt, y, ys, sol, dRedo);
      const unsigned lanes = seriesBlock(series);
      hipLaunchKernelGGL(k_spline_series, dim3((unsigned)((series + lanes - 1) / lanes)), dim3(lanes), 0, st, series, dYOff, dSOff, dCnt, y, ys, sol,
                         byLanes ? dRedo : nullptr);
   };

   for (size_t ci = 0; ci + 1 < cuts.size(); ++ci)
   {
      const int ka = cuts[ci], kb = cuts[ci + 1];
      const int64_t baseF = all[ka].offF;
      // The paths of a chunk run route by route through one launch sequence each: at most four, whatever the number of paths and
      // however their routes alternate.  Within a sequence every offset is dense over its own paths (out_find_path searches them);
      // offD is the path's place in the result, which stays in path order.  Where a chunk holds one route only (always, with a
      // positive integ_res) the two coincide and the last stage writes the result itself, as it always did; a chunk that mixes
      // routes stages the final rows of each sequence and k_out_place moves them.
      unsigned routesChunk = 0;
      for (int k = ka; k < kb; ++k) if (all[k].nFwd) routesChunk |= 1u << step[k].route;
      const bool staged = (routesChunk & (routesChunk - 1)) != 0;
      for (int route = 0; route < 4; ++route)
      {
         const bool reinterp = (route & 2) != 0, smoothing = (route & 1) != 0;
         std::vector<OutPath> pc;
         for (int k = ka; k < kb; ++k) if (step[k].route == route) pc.push_back(all[k]);
         const int Kc = (int)pc.size();
         int64_t t1 = 0, t2 = 0, tS = 0, tF = 0;
         for (OutPath &q : pc)
         {
            q.off1 = t1; q.off2 = t2; q.offS = tS; q.offD = q.offF - baseF; q.offF = tF;
            t1 += q.n1; t2 += q.n2; tS += q.nFwd; tF += q.nF;
         }
         if (t1 == 0) continue; // no path of the chunk takes this route, or every one that would failed in the sweep
         if (!smoothing) for (OutPath &q : pc) q.off2 = q.off1;

         if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) { batotp_hip_output_destroy(o); return rc; }   // (every chunk starts from poisoned scratch)
         Bump w;
         w.base = (char *)ctx->ws[1].p;
         OutPath *dPaths = w.take<OutPath>(Kc);
         int64_t *dYOff = w.take<int64_t>((size_t)Kc * R), *dSOff = w.take<int64_t>((size_t)Kc * R);
         int *dCnt = w.take<int>((size_t)Kc * R);
         int *dRedo = w.take<int>((size_t)Kc * R); // series the wavefront-per-series solve leaves to the sequential kernel
         double *solS = w.take<double>((size_t)tS);
         double *sOut = w.take<double>((size_t)t1);
         int *segK = w.take<int>((size_t)t1);
         double *resultOut = o->dTheta + baseF * Rout;
         double *result = (pose || staged) ? w.take<double>((size_t)tF * R) : resultOut;   // poses: the conversion follows the last stage
         double *th0 = (cable || serialTrq) ? w.take<double>((size_t)t1 * R) : nullptr;  // samples before the torque step ...
         double *sol1 = (cable || serialTrq) ? w.take<double>((size_t)t1 * R) : nullptr; // ... and the second derivatives of their splines
         double *th1 = (smoothing || reinterp) ? w.take<double>((size_t)t1 * R) : result;
         double *th2 = !smoothing ? th1 : (reinterp ? w.take<double>((size_t)t2 * R) : result);
         double *sol2 = reinterp ? w.take<double>((size_t)t2 * R) : nullptr;
         if (w.at > ctx->ws[1].cap) { batotp_hip_output_destroy(o); snprintf(g_err, sizeof(g_err), "output stage: scratch estimate exceeded"); return BATOTP_ERR_STATE; }

         // series descriptors: s(t) of every path, then (re-interpolation) every channel of every path
         std::vector<int64_t> yOff((size_t)Kc * R), sOff(yOff.size());
         std::vector<int> cnt(yOff.size());
         for (int k = 0; k < Kc; ++k)
         {
            yOff[k] = (int64_t)pc[k].p * b->cap * 2; // s of point i of the forward curve = element 2*i of its slot
            sOff[k] = pc[k].offS;
            cnt[k] = pc[k].nFwd;
         }
         OUT_TRY(hipMemcpyAsync(dPaths, pc.data(), sizeof(OutPath) * Kc, hipMemcpyHostToDevice, st));
         OUT_TRY(hipMemcpyAsync(dYOff, yOff.data(), sizeof(int64_t) * Kc, hipMemcpyHostToDevice, st));
         OUT_TRY(hipMemcpyAsync(dSOff, sOff.data(), sizeof(int64_t) * Kc, hipMemcpyHostToDevice, st));
         OUT_TRY(hipMemcpyAsync(dCnt, cnt.data(), sizeof(int) * Kc, hipMemcpyHostToDevice, st));
         solveSeries(Kc, dYOff, dSOff, dCnt, dRedo, reinterpret_cast<const double *>(b->dFwd), 2, solS);
         hipLaunchKernelGGL(k_out_s, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, dPaths, Kc, b->dFwd, b->cap, solS, b->dPinfo, b->dSC, sOut,
                            segK, t1);
         launchOutSegmax(st, dPaths, Kc, segK);
         if (!cable)
         {
            double *thA = serialTrq ? th0 : th1; // joint (and Cartesian) rows before the torque step
            hipLaunchKernelGGL(k_out_eval, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM,
                               sOut, segK, thA, 0, nJ, 0, t1);
            if (both)   // the Cartesian rows from their splines, like the joints (ba.cpp:1726-1736)
               hipLaunchKernelGGL(k_out_eval, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM,
                                  sOut, segK, thA, nJ, nCartRows, nJ, t1);
            if (kin || serialTrq)
            {
               // scratch of the kinematics / dynamics at the output points (own workspace): packed joint rows, trig table, and for
               // the torque step a sample array [Cin][3][n1], a dynamics array [4][nJ][n1] and the PathInfo rows k_dynamics reads
               const int rowsDyn = serialTrq ? (b->hasSerial ? 2 * nJ : 4) : 0;
               const int rowsT = std::max(kin ? trigRows : 0, rowsDyn);
               const size_t needKin = 8 * (size_t)t1 * (size_t)(nJ + rowsT + (serialTrq ? 3 * b->P.Cin + 4 * nJ : 0)) + sizeof(PathInfo) * (size_t)Kc + 4096;
               if ((rc = arenaReserve(ctx->ws[3], needKin, st))) { batotp_hip_output_destroy(o); return rc; }
               if ((rc = poisonFill(ctx, ctx->ws[3].p, ctx->ws[3].cap, st))) { batotp_hip_output_destroy(o); return rc; }
               Bump wk;
               wk.base = (char *)ctx->ws[3].p;
               double *pack = wk.take<double>((size_t)t1 * nJ), *trig = wk.take<double>((size_t)t1 * rowsT);
               double *sampT = serialTrq ? wk.take<double>((size_t)t1 * 3 * b->P.Cin) : nullptr;
               double *dynT = serialTrq ? wk.take<double>((size_t)t1 * 4 * nJ) : nullptr;
               PathInfo *dFake = wk.take<PathInfo>((size_t)Kc);
               std::vector<TrigSpan> spans(Kc);
               for (int k = 0; k < Kc; ++k) spans[k] = TrigSpan{pc[k].off1, pc[k].n1, pc[k].n1 == 0};
               const unsigned grid1 = (unsigned)((t1 + bs - 1) / bs);
               // (the tables are trigonometric functions of the joint rows alone: neither tableFor nor hostTrigTables reads a step)
               auto tableFor = [&](int kind, double unit) -> int {
                  // joint rows (already packed on the device) -> host -> trig table -> device
                  const int rows = hostTrigRows(kind, b->prob.robot_type, nJ);
                  ctx->kinTheta.resize((size_t)t1 * nJ);
                  ctx->kinTrig.resize((size_t)t1 * rows);
                  HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), pack, sizeof(double) * ctx->kinTheta.size(), hipMemcpyDeviceToHost, st));
                  HIP_TRY(hipStreamSynchronize(st));
                  hostTrigTables(kind, b->prob.robot_type, nJ, unit, spans, ctx->kinTheta.data(), ctx->kinTrig.data());
                  HIP_TRY(hipMemcpyAsync(trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, st));
                  HIP_TRY(hipStreamSynchronize(st)); // the host table is reused
                  return BATOTP_OK;
               };
               if (kin)
               {
                  // Robot::fwdKin at the output points, ba.cpp:1722-1725
                  if (hostTrig)
                  {
                     hipLaunchKernelGGL(k_out_pack_theta, dim3(grid1), dim3(bs), 0, st, P, dPaths, Kc, thA, pack, t1);
                     if ((rc = tableFor(0, 1.0))) { batotp_hip_output_destroy(o); return rc; }
                  }
                  hipLaunchKernelGGL(k_out_fwdkin, dim3(grid1), dim3(bs), 0, st, P, b->prob.robot_type, dPaths, Kc, thA,
                                     hostTrig ? trig : (const double *)nullptr, trigRows, b->dPinfo, b->dSamp, t1);
               }
               if (serialTrq)
               {
                  // ba.cpp:1791-1827: clamped splines through the joint samples, value / derivatives at the end of the previous
                  // segment, Robot::dynSerial there (the batch's own kernels on a sample array of the output points), a2 + a3 + a4
                  OUT_TRY(hipGetLastError());
                  OUT_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
                  std::vector<PathInfo> fake(Kc);
                  for (int k = 0; k < Kc; ++k)
                  {
                     memset(&fake[k], 0, sizeof(PathInfo));
                     fake[k].koff = pc[k].off1; fake[k].n = pc[k].n1;
                     for (int c = 0; c < nJ; ++c)
                     {
                        const size_t at = (size_t)k * nJ + c;
                        yOff[at] = pc[k].off1 * R + (int64_t)c * pc[k].n1;
                        sOff[at] = yOff[at];
                        cnt[at] = pc[k].n1;
                     }
                  }
                  OUT_TRY(hipMemcpyAsync(dFake, fake.data(), sizeof(PathInfo) * (size_t)Kc, hipMemcpyHostToDevice, st));
                  OUT_TRY(hipMemcpyAsync(dYOff, yOff.data(), sizeof(int64_t) * (size_t)Kc * nJ, hipMemcpyHostToDevice, st));
                  OUT_TRY(hipMemcpyAsync(dSOff, sOff.data(), sizeof(int64_t) * (size_t)Kc * nJ, hipMemcpyHostToDevice, st));
                  OUT_TRY(hipMemcpyAsync(dCnt, cnt.data(), sizeof(int) * (size_t)Kc * nJ, hipMemcpyHostToDevice, st));
                  hipLaunchKernelGGL(k_spline_series_clamped, dim3((unsigned)((Kc * nJ + seriesBlock(Kc * nJ) - 1) / seriesBlock(Kc * nJ))), dim3(seriesBlock(Kc * nJ)), 0, st, Kc * nJ, dYOff, dSOff, dCnt, th0, sol1);
                  OUT_TRY(hipMemsetAsync(sampT, 0, sizeof(double) * (size_t)t1 * 3 * b->P.Cin, st));
                  hipLaunchKernelGGL(k_out_serial_eval, dim3(grid1), dim3(bs), 0, st, P, dPaths, Kc, th0, sol1, th1, sampT, pack, nCartRows, t1);
                  OUT_TRY(hipGetLastError());
                  OUT_TRY(hipStreamSynchronize(st)); // `fake` leaves scope below; the trig tables follow
                  const double *trigDyn = nullptr;
                  if (hostTrig)
                  {
                     const double unit = (b->hasSerial && b->hModel.degrees) ? KIN_DEG2RAD : 1.0;
                     if ((rc = tableFor(b->hasSerial ? 2 : 1, unit))) { batotp_hip_output_destroy(o); return rc; }
                     trigDyn = trig;
                  }
                  if (b->hasSerial)
                     hipLaunchKernelGGL(k_dyn_serial, dim3((unsigned)((t1 + KDS_BLOCK - 1) / KDS_BLOCK)), dim3(KDS_BLOCK), 0, st, b->dModel, b->P.Cin, dFake, Kc,
                                        sampT, trigDyn, dynT, t1);
                  else
                     hipLaunchKernelGGL(k_dynamics, dim3(grid1), dim3(bs), 0, st, b->P, b->dP, dFake, Kc, sampT, trigDyn, dynT, t1);
                  hipLaunchKernelGGL(k_out_trq_sum, dim3(grid1), dim3(bs), 0, st, P, dPaths, Kc, dynT, th1, nJ + nCartRows, t1);
               }
            }
         }
         else
         {
            // CART path: Cartesian rows from the path splines, cable lengths from them, then the torque step
            hipLaunchKernelGGL(k_out_eval, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM,
                               sOut, segK, th0, nJ, 3, 3, t1);
            hipLaunchKernelGGL(k_out_invkin, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, th0, t1);
            OUT_TRY(hipGetLastError());
            OUT_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
            for (int k = 0; k < Kc; ++k)
               for (int c = 0; c < 6; ++c)
               {
                  const size_t at = (size_t)k * 6 + c;
                  yOff[at] = pc[k].off1 * R + (int64_t)c * pc[k].n1;
                  sOff[at] = yOff[at];
                  cnt[at] = pc[k].n1;
               }
            OUT_TRY(hipMemcpyAsync(dYOff, yOff.data(), sizeof(int64_t) * (size_t)Kc * 6, hipMemcpyHostToDevice, st));
            OUT_TRY(hipMemcpyAsync(dSOff, sOff.data(), sizeof(int64_t) * (size_t)Kc * 6, hipMemcpyHostToDevice, st));
            OUT_TRY(hipMemcpyAsync(dCnt, cnt.data(), sizeof(int) * (size_t)Kc * 6, hipMemcpyHostToDevice, st));
            solveSeries(Kc * 6, dYOff, dSOff, dCnt, dRedo, th0, 1, sol1);
            hipLaunchKernelGGL(k_out_trq, dim3((unsigned)((t1 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, th0, sol1, th1, t1);
         }
         if (smoothing)
            hipLaunchKernelGGL(k_out_down, dim3((unsigned)((t2 + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, th1, th2, t2);
         OUT_TRY(hipGetLastError());
         if (reinterp)
         {
            OUT_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
            for (int k = 0; k < Kc; ++k)
               for (int c = 0; c < R; ++c)
               {
                  const size_t at = (size_t)k * R + c;
                  yOff[at] = pc[k].off2 * R + (int64_t)c * pc[k].n2;
                  sOff[at] = yOff[at];
                  cnt[at] = pc[k].n2;
               }
            OUT_TRY(hipMemcpyAsync(dYOff, yOff.data(), sizeof(int64_t) * yOff.size(), hipMemcpyHostToDevice, st));
            OUT_TRY(hipMemcpyAsync(dSOff, sOff.data(), sizeof(int64_t) * sOff.size(), hipMemcpyHostToDevice, st));
            OUT_TRY(hipMemcpyAsync(dCnt, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice, st));
            const int series = Kc * R;
            solveSeries(series, dYOff, dSOff, dCnt, dRedo, th2, 1, sol2);
            hipLaunchKernelGGL(k_out_user, dim3((unsigned)((tF + bs - 1) / bs)), dim3(bs), 0, st, P, dPaths, Kc, th2, sol2, result, tF);
            OUT_TRY(hipGetLastError());
         }
         if (pose)
         {
            // BA::q2aaVect (ba.cpp:1920-1927): quaternion rows -> axis-angle rows, the result loses the seventh Cartesian row
            const unsigned gridF = (unsigned)((tF + bs - 1) / bs);
            const double *atDev = nullptr;
            if (hostTrig)
            {
               double *packQ = w.take<double>((size_t)tF * 2), *atTab = w.take<double>((size_t)tF);
               if (w.at > ctx->ws[1].cap) { batotp_hip_output_destroy(o); snprintf(g_err, sizeof(g_err), "output stage: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
               hipLaunchKernelGGL(k_out_q_norm, dim3(gridF), dim3(bs), 0, st, nJ, R, dPaths, Kc, result, packQ, tF);
               ctx->kinTheta.resize((size_t)tF * 2);
               ctx->kinTrig.resize((size_t)tF);
               OUT_TRY(hipMemcpyAsync(ctx->kinTheta.data(), packQ, sizeof(double) * (size_t)tF * 2, hipMemcpyDeviceToHost, st));
               OUT_TRY(hipStreamSynchronize(st));
               for (int k = 0; k < Kc; ++k)
               {
                  const int64_t off = pc[k].offF, n = pc[k].nF;
                  for (int64_t i = 0; i < n; ++i)   // util.cpp:573: one atan2() per point, host libm
                     ctx->kinTrig[(size_t)(off + i)] = ::atan2(ctx->kinTheta[(size_t)(off * 2 + i)], ctx->kinTheta[(size_t)(off * 2 + n + i)]);
               }
               OUT_TRY(hipMemcpyAsync(atTab, ctx->kinTrig.data(), sizeof(double) * (size_t)tF, hipMemcpyHostToDevice, st));
               atDev = atTab;
            }
            hipLaunchKernelGGL(k_out_q2aa, dim3(gridF), dim3(bs), 0, st, nJ, R, dPaths, Kc, result, atDev, resultOut, tF);
            OUT_TRY(hipGetLastError());
         }
         else if (staged)
         {
            hipLaunchKernelGGL(k_out_place, dim3((unsigned)((tF + bs - 1) / bs)), dim3(bs), 0, st, R, dPaths, Kc, result, resultOut, tF);
            OUT_TRY(hipGetLastError());
         }
         OUT_TRY(hipStreamSynchronize(st)); // the host vectors go out of scope, the scratch is reused by the next route or chunk
      }
   }
   OUT_TRY(hipEventRecord(ev1, st));
   OUT_TRY(hipStreamSynchronize(st));
   OUT_TRY(hipEventElapsedTime(&o->ms, ev0, ev1));
#undef OUT_TRY
   *out = o;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_info(batotp_output *o, int64_t *n_pts, double *sres)
{
   if (!o) return BATOTP_ERR_ARG;
   for (int k = 0; k < o->K; ++k)
   {
      if (n_pts) n_pts[k] = o->n[k];
      if (sres) sres[k] = o->sres[k];
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_channels(batotp_output *o, int32_t *n_theta, int32_t *n_cart, int32_t *n_trq)
{
   if (!o) return BATOTP_ERR_ARG;
   if (n_theta) *n_theta = o->nTheta;
   if (n_cart) *n_cart = o->nCart;
   if (n_trq) *n_trq = o->nTrq;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_download(batotp_output *o, int32_t k, double *theta)
{
   if (!o || !theta || k < 0 || k >= o->K) return BATOTP_ERR_ARG;
   if (o->n[k] == 0) return BATOTP_OK;
   int rc = bind(o->ctx);
   if (rc) return rc;
   HIP_TRY(hipMemcpyAsync(theta, o->dTheta + o->off[k] * o->nJ, sizeof(double) * (size_t)(o->n[k] * o->nJ), hipMemcpyDeviceToHost, o->ctx->stream));
   HIP_TRY(hipStreamSynchronize(o->ctx->stream));
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_download_all(batotp_output *o, double *rows)
{
   if (!o || !rows) return BATOTP_ERR_ARG;
   if (o->total == 0) return BATOTP_OK;
   int rc = bind(o->ctx);
   if (rc) return rc;
   HIP_TRY(hipMemcpyAsync(rows, o->dTheta, sizeof(double) * (size_t)(o->total * o->nJ), hipMemcpyDeviceToHost, o->ctx->stream));
   HIP_TRY(hipStreamSynchronize(o->ctx->stream));
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_device(batotp_output *o, const double **theta_dev, int64_t *n_doubles)
{
   if (!o || !theta_dev) return BATOTP_ERR_ARG;
   *theta_dev = o->dTheta;
   if (n_doubles) *n_doubles = o->total * o->nJ;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_ms(batotp_output *o, float *ms)
{
   if (!o || !ms) return BATOTP_ERR_ARG;
   *ms = o->ms;
   return BATOTP_OK;
}
