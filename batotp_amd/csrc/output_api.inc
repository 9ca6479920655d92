// output_api.inc -- host side of batotp_hip_output (included at the end of batotp_hip.hip).
// All sizes of the stage follow from the results of the forward sweep (points and time step of each curve), so
// the host lays out every buffer before the first kernel (output_plan.h); the paths of a call are processed in
// chunks whose scratch fits the context's cached workspace.

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
   float auditMs = 0.f;         // kernels of the last audit of these rows (audit_api.inc)
   bool audited = false;
   bool fromTorques = false;    // made by batotp_hip_output_torques (invdyn_api.inc) ...
   float trqMs = 0.f;           // ... kernels of that call
   int trqRanges = 0;           // ... and the ranges of paths it was cut into
   bool fromStretch = false;    // made by batotp_hip_output_stretch_to / _by / _audit (stretch_api.inc) ...
   float stretchMs = 0.f;       // ... stretch kernels of that call, all rounds and ranges
   int stretchRanges = 0;       // ... and how many launches that was
   bool fromTscale = false;     // made by batotp_hip_output_torque_scale / _stretch_torques (tscale_api.inc) ...
   float tscaleMs = 0.f;        // ... kernels of tscale.hip.h in that call, all rounds and ranges
   int tscaleRanges = 0;        // ... and how many launches of k_tscale that was
   bool fromDuty = false;       // made by batotp_hip_output_duty / _stretch_duty (duty_api.inc) ...
   float dutyMs = 0.f;          // ... kernels of duty.hip.h in that call, all rounds and ranges
   int dutyRanges = 0;          // ... and how many launches of k_duty that was
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

// ---- batotp_hip_output: what the call is (OutCall), one route of one chunk on the device (OutRoute), the steps of its launch
// sequence in the order they run, and the entry point.  Every hipStreamSynchronize below guards host memory that is about to be
// rewritten or to go out of scope; the comment beside it says which.

// what every step knows about the call: the batch and which branches of the reference's stage its problem takes
struct OutCall
{
   batotp_batch *b;
   batotp_ctx *ctx;
   hipStream_t st;
   bool cable, kin, chainKin, serialTrq, both, pose, hostTrig;   // chainKin: kin by the batch's kinematic chain, not a closed form
   int trigRows, nJ, nCartRows, nTrqRows;
   int R;    // rows per point the stage works with: joints (+ Cartesian + torques)
   int Rout; // rows per point of the result (poses leave as position + axis-angle)
   OutParams P;
};

// the paths of one route of one chunk with their offsets (RouteLayout), the buffers carved for them from the context's workspace
// and the host side of the series descriptors
struct OutRoute
{
   RouteLayout L;
   int Kc;
   bool reinterp, smoothing;
   Bump w;
   OutPath *dPaths;
   int64_t *dYOff, *dSOff;
   int *dCnt, *dRedo;   // dRedo: series the wavefront-per-series solve leaves to the sequential kernel
   double *solS, *sOut;
   int *segK;
   double *resultOut, *result, *th0, *sol1, *th1, *th2, *sol2;
   std::vector<int64_t> yOff, sOff;
   std::vector<int> cnt;
};

// scratch of the kinematics / dynamics at the output points, carved from a workspace of its own
struct OutKin
{
   double *pack, *trig, *sampT, *dynT;
   PathInfo *dFake;
   std::vector<TrigSpan> spans;
};

constexpr int OUT_BS = 256;
static inline dim3 grid256(int64_t n) { return dim3((unsigned)((n + OUT_BS - 1) / OUT_BS)); }

// the refusals of a call, and what it is once it is accepted; binds the context
static int outputCall(batotp_batch *b, const batotp_output_params *prm, int32_t path0, int32_t n_paths, OutCall &c)
{
   const bool cable = prm->path_type == BATOTP_PATH_CART && b->prob.robot_type == BATOTP_ROBOT_CSPR3DOF && prm->n_joints == 3 &&
                      b->prob.n_cart == 3 && (b->prob.flags & BATOTP_F_TRQ_ON) && (b->prob.flags & BATOTP_F_PARALLEL);
   const bool jointPath = prm->path_type == BATOTP_PATH_JOINT || prm->path_type == 0;
   // JOINT path of a robot with forward kinematics (KUKA, RR; SURVEY.md 8 f-3): three Cartesian rows from the joint rows
   // ... or of any robot whose batch has a kinematic chain (batotp_hip_set_kin_chain): the chain's tool point, tables of kind 2
   const bool chainKin = jointPath && b->hasKinChain;
   const int trigRows = chainKin ? 2 * prm->n_joints : fwdkin_trig_rows(b->prob.robot_type, prm->n_joints);
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
       (kin && !chainKin && b->prob.robot_type == BATOTP_ROBOT_RR && (b->prob.flags & BATOTP_F_NO_SAMPLES)))
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
   if (!b->revDone) return BATOTP_ERR_STATE;
   int rc = bind(b->ctx);
   if (rc) return rc;
   const int nJ = b->P.nJ;
   c.b = b; c.ctx = b->ctx; c.st = b->ctx->stream;
   c.cable = cable; c.kin = kin; c.chainKin = kin && chainKin; c.serialTrq = serialTrq; c.both = both; c.pose = pose;
   c.hostTrig = (b->prob.flags & BATOTP_F_HOST_TRIG) != 0;
   c.trigRows = trigRows; c.nJ = nJ;
   c.nCartRows = cable ? 3 : (both ? (int)b->prob.n_cart : (kin ? 3 : 0));
   c.nTrqRows = cable ? 3 : (serialTrq ? nJ : 0);
   c.R = nJ + c.nCartRows + c.nTrqRows;
   c.Rout = pose ? c.R - 1 : c.R;
   OutParams &P = c.P;
   memset(&P, 0, sizeof(P));
   P.nJ = nJ; P.R = c.R; P.compact = b->compact ? 1 : 0; P.kmC = b->kmC;
   P.C = b->P.C; P.Cin = b->P.Cin; P.svd = (b->prob.flags & BATOTP_F_SVD) ? 1 : 0;
   for (int k = 0; k < 9; ++k) P.pmat[k] = b->prob.pmat[k];
   return BATOTP_OK;
}

// the buffers of a route (r.L is set) from the output workspace; resultOut: the chunk's place in the result of the call
static int carveRoute(const OutCall &c, int route, double *resultOut, OutRoute &r)
{
   const int R = c.R, Kc = r.Kc = (int)r.L.pc.size();
   const int64_t t1 = r.L.t1, t2 = r.L.t2;
   const bool reinterp = r.reinterp = (route & 2) != 0, smoothing = r.smoothing = (route & 1) != 0, torque = c.cable || c.serialTrq;
   Bump &w = r.w;
   w.base = (char *)c.ctx->ws[1].p;
   r.dPaths = w.take<OutPath>(Kc);
   r.dYOff = w.take<int64_t>((size_t)Kc * R); r.dSOff = w.take<int64_t>((size_t)Kc * R);
   r.dCnt = w.take<int>((size_t)Kc * R);
   r.dRedo = w.take<int>((size_t)Kc * R);
   r.solS = w.take<double>((size_t)r.L.tS);
   r.sOut = w.take<double>((size_t)t1);
   r.segK = w.take<int>((size_t)t1);
   r.resultOut = resultOut;
   r.result = (c.pose || r.L.staged) ? w.take<double>((size_t)r.L.tF * R) : resultOut; // poses: the conversion follows the last stage
   r.th0 = torque ? w.take<double>((size_t)t1 * R) : nullptr;  // samples before the torque step ...
   r.sol1 = torque ? w.take<double>((size_t)t1 * R) : nullptr; // ... and the second derivatives of their splines
   r.th1 = (smoothing || reinterp) ? w.take<double>((size_t)t1 * R) : r.result;
   r.th2 = !smoothing ? r.th1 : (reinterp ? w.take<double>((size_t)t2 * R) : r.result);
   r.sol2 = reinterp ? w.take<double>((size_t)t2 * R) : nullptr;
   if (w.at > c.ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "output stage: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
   r.yOff.resize((size_t)Kc * R); r.sOff.resize(r.yOff.size()); r.cnt.resize(r.yOff.size());
   return BATOTP_OK;
}

// The first `series` descriptors of r.yOff / sOff / cnt to the device.  The copies read the host vectors when the stream reaches
// them: whoever fills the vectors again synchronises first.
static int uploadSeries(const OutCall &c, const OutRoute &r, int series)
{
   HIP_TRY(hipMemcpyAsync(r.dYOff, r.yOff.data(), sizeof(int64_t) * (size_t)series, hipMemcpyHostToDevice, c.st));
   HIP_TRY(hipMemcpyAsync(r.dSOff, r.sOff.data(), sizeof(int64_t) * (size_t)series, hipMemcpyHostToDevice, c.st));
   HIP_TRY(hipMemcpyAsync(r.dCnt, r.cnt.data(), sizeof(int) * (size_t)series, hipMemcpyHostToDevice, c.st));
   return BATOTP_OK;
}

// ... of the first `rows` channels of every path, solved in place: a path's points are an [R][n] block of the stage-1 arrays
// (down == false) or of the down-sampled ones
static int uploadChannelSeries(const OutCall &c, OutRoute &r, int rows, bool down)
{
   for (int k = 0; k < r.Kc; ++k)
   {
      const OutPath &q = r.L.pc[k];
      const int64_t off = down ? q.off2 : q.off1;
      const int n = down ? q.n2 : q.n1;
      for (int ch = 0; ch < rows; ++ch)
      {
         const size_t at = (size_t)k * rows + ch;
         r.yOff[at] = off * c.R + (int64_t)ch * n;
         r.sOff[at] = r.yOff[at];
         r.cnt[at] = n;
      }
   }
   return uploadSeries(c, r, r.Kc * rows);
}

// natural-spline second derivatives of `series` series (the descriptors on the device): a wavefront per series where the series
// is long enough (spline_lanes.hip.h) and there are few of them (seriesLanesPay), the lane-per-series kernel for the rest
static void solveSeries(const OutCall &c, const OutRoute &r, int series, const double *y, int ys, double *sol)
{
   const bool byLanes = seriesLanesPay(series);
   if (byLanes) hipLaunchKernelGGL(k_spline_series_lanes, dim3((unsigned)series), dim3(64), 0, c.st, series, r.dYOff, r.dSOff, r.dCnt, y, ys, sol, r.dRedo);
   const unsigned lanes = seriesBlock(series);
   hipLaunchKernelGGL(k_spline_series, dim3((unsigned)((series + lanes - 1) / lanes)), dim3(lanes), 0, c.st, series, r.dYOff, r.dSOff, r.dCnt, y, ys, sol,
                      byLanes ? r.dRedo : nullptr);
}

// s at the output times of every path and the segment of the path spline each falls into (ba.cpp:1683-1707)
static int sampleS(const OutCall &c, OutRoute &r)
{
   batotp_batch *b = c.b;
   for (int k = 0; k < r.Kc; ++k)
   {
      const OutPath &q = r.L.pc[k];
      r.yOff[k] = (int64_t)q.p * b->cap * 2; // s of point i of the forward curve = element 2*i of its slot
      r.sOff[k] = q.offS;
      r.cnt[k] = q.nFwd;
   }
   HIP_TRY(hipMemcpyAsync(r.dPaths, r.L.pc.data(), sizeof(OutPath) * r.Kc, hipMemcpyHostToDevice, c.st));
   int rc = uploadSeries(c, r, r.Kc);
   if (rc) return rc;
   solveSeries(c, r, r.Kc, reinterpret_cast<const double *>(b->dFwd), 2, r.solS);
   hipLaunchKernelGGL(k_out_s, grid256(r.L.t1), dim3(OUT_BS), 0, c.st, r.dPaths, r.Kc, b->dFwd, b->cap, r.solS, b->dPinfo, b->dSC, r.sOut, r.segK, r.L.t1);
   launchOutSegmax(c.st, r.dPaths, r.Kc, r.segK);
   return BATOTP_OK;
}

// joint rows (already packed on the device) -> host -> trig table -> device
// (the tables are trigonometric functions of the joint rows alone: neither this nor hostTrigTables reads a step)
static int tableFor(const OutCall &c, const OutRoute &r, const OutKin &kn, int kind, double unit)
{
   batotp_ctx *ctx = c.ctx;
   const int rows = hostTrigRows(kind, c.b->prob.robot_type, c.nJ);
   ctx->kinTheta.resize((size_t)r.L.t1 * c.nJ);
   ctx->kinTrig.resize((size_t)r.L.t1 * rows);
   HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), kn.pack, sizeof(double) * ctx->kinTheta.size(), hipMemcpyDeviceToHost, c.st));
   HIP_TRY(hipStreamSynchronize(c.st));
   hostTrigTables(kind, c.b->prob.robot_type, c.nJ, unit, kn.spans, ctx->kinTheta.data(), ctx->kinTrig.data());
   HIP_TRY(hipMemcpyAsync(kn.trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, c.st));
   HIP_TRY(hipStreamSynchronize(c.st)); // the host table is reused
   return BATOTP_OK;
}

// ba.cpp:1791-1827: clamped splines through the joint samples, value / derivatives at the end of the previous segment,
// Robot::dynSerial there (the batch's own kernels on a sample array of the output points), a2 + a3 + a4
static int serialTorque(const OutCall &c, OutRoute &r, const OutKin &kn)
{
   batotp_batch *b = c.b;
   hipStream_t st = c.st;
   const int Kc = r.Kc, nJ = c.nJ;
   const int64_t t1 = r.L.t1;
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
   std::vector<PathInfo> fake(Kc);
   for (int k = 0; k < Kc; ++k)
   {
      memset(&fake[k], 0, sizeof(PathInfo));
      fake[k].koff = r.L.pc[k].off1; fake[k].n = r.L.pc[k].n1;
   }
   HIP_TRY(hipMemcpyAsync(kn.dFake, fake.data(), sizeof(PathInfo) * (size_t)Kc, hipMemcpyHostToDevice, st));
   int rc = uploadChannelSeries(c, r, nJ, false);
   if (rc) return rc;
   hipLaunchKernelGGL(k_spline_series_clamped, dim3((unsigned)((Kc * nJ + seriesBlock(Kc * nJ) - 1) / seriesBlock(Kc * nJ))), dim3(seriesBlock(Kc * nJ)), 0, st, Kc * nJ, r.dYOff, r.dSOff, r.dCnt, r.th0, r.sol1);
   HIP_TRY(hipMemsetAsync(kn.sampT, 0, sizeof(double) * (size_t)t1 * 3 * b->P.Cin, st));
   hipLaunchKernelGGL(k_out_serial_eval, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, Kc, r.th0, r.sol1, r.th1, kn.sampT, kn.pack, c.nCartRows, t1);
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(st)); // `fake` leaves scope below; the trig tables follow
   const double *trigDyn = nullptr;
   if (c.hostTrig)
   {
      const double unit = (b->hasSerial && b->hModel.degrees) ? KIN_DEG2RAD : 1.0;
      if ((rc = tableFor(c, r, kn, b->hasSerial ? 2 : 1, unit))) return rc;
      trigDyn = kn.trig;
   }
   if (b->hasSerial)
      hipLaunchKernelGGL(k_dyn_serial, dim3((unsigned)((t1 + KDS_BLOCK - 1) / KDS_BLOCK)), dim3(KDS_BLOCK), 0, st, b->dModel, b->P.Cin, kn.dFake, Kc,
                         kn.sampT, trigDyn, kn.dynT, t1);
   else
      hipLaunchKernelGGL(k_dynamics, grid256(t1), dim3(OUT_BS), 0, st, b->P, b->dP, kn.dFake, Kc, kn.sampT, trigDyn, kn.dynT, t1);
   hipLaunchKernelGGL(k_out_trq_sum, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, Kc, kn.dynT, r.th1, nJ + c.nCartRows, t1);
   return BATOTP_OK;
}

// JOINT and BOTH paths: the rows from the path splines, then the forward kinematics and the torques of a serial robot
static int evalJoints(const OutCall &c, OutRoute &r)
{
   batotp_batch *b = c.b;
   batotp_ctx *ctx = c.ctx;
   hipStream_t st = c.st;
   const int Kc = r.Kc, nJ = c.nJ;
   const int64_t t1 = r.L.t1;
   double *thA = c.serialTrq ? r.th0 : r.th1; // joint (and Cartesian) rows before the torque step
   hipLaunchKernelGGL(k_out_eval, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM, r.sOut, r.segK, thA, 0, nJ, 0, t1);
   if (c.both)   // the Cartesian rows from their splines, like the joints (ba.cpp:1726-1736)
      hipLaunchKernelGGL(k_out_eval, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM, r.sOut, r.segK, thA, nJ, c.nCartRows, nJ, t1);
   if (!c.kin && !c.serialTrq) return BATOTP_OK;
   // scratch of the kinematics / dynamics at the output points (own workspace): packed joint rows, trig table, and for
   // the torque step a sample array [Cin][3][n1], a dynamics array [4][nJ][n1] and the PathInfo rows k_dynamics reads
   const int rowsDyn = c.serialTrq ? (b->hasSerial ? 2 * nJ : 4) : 0;
   const int rowsT = std::max(c.kin ? c.trigRows : 0, rowsDyn);
   const size_t needKin = 8 * (size_t)t1 * (size_t)(nJ + rowsT + (c.serialTrq ? 3 * b->P.Cin + 4 * nJ : 0)) + sizeof(PathInfo) * (size_t)Kc + 4096;
   int rc;
   if ((rc = arenaReserve(ctx->ws[3], needKin, st))) return rc;
   if ((rc = poisonFill(ctx, ctx->ws[3].p, ctx->ws[3].cap, st))) return rc;
   Bump wk;
   wk.base = (char *)ctx->ws[3].p;
   OutKin kn;
   kn.pack = wk.take<double>((size_t)t1 * nJ); kn.trig = wk.take<double>((size_t)t1 * rowsT);
   kn.sampT = c.serialTrq ? wk.take<double>((size_t)t1 * 3 * b->P.Cin) : nullptr;
   kn.dynT = c.serialTrq ? wk.take<double>((size_t)t1 * 4 * nJ) : nullptr;
   kn.dFake = wk.take<PathInfo>((size_t)Kc);
   kn.spans.resize(Kc);
   for (int k = 0; k < Kc; ++k) kn.spans[k] = TrigSpan{r.L.pc[k].off1, r.L.pc[k].n1, r.L.pc[k].n1 == 0};
   if (c.kin)
   {
      // Robot::fwdKin at the output points, ba.cpp:1722-1725
      if (c.hostTrig)
      {
         hipLaunchKernelGGL(k_out_pack_theta, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, Kc, thA, kn.pack, t1);
         if ((rc = tableFor(c, r, kn, c.chainKin ? 2 : 0, (c.chainKin && b->kinChain.degrees) ? KIN_DEG2RAD : 1.0))) return rc;
      }
      if (c.chainKin)
         hipLaunchKernelGGL(k_out_fwdkin_chain, grid256(t1), dim3(OUT_BS), 0, st, c.P, b->kinChain, r.dPaths, Kc, thA,
                            c.hostTrig ? kn.trig : (const double *)nullptr, t1);
      else
         hipLaunchKernelGGL(k_out_fwdkin, grid256(t1), dim3(OUT_BS), 0, st, c.P, b->prob.robot_type, r.dPaths, Kc, thA,
                            c.hostTrig ? kn.trig : (const double *)nullptr, c.trigRows, b->dPinfo, b->dSamp, t1);
   }
   return c.serialTrq ? serialTorque(c, r, kn) : BATOTP_OK;
}

// CART path of the cable robot: Cartesian rows from the path splines, cable lengths from them, then the torque step
static int evalCable(const OutCall &c, OutRoute &r)
{
   batotp_batch *b = c.b;
   hipStream_t st = c.st;
   const int64_t t1 = r.L.t1;
   hipLaunchKernelGGL(k_out_eval, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, r.Kc, b->dPinfo, b->dSC, b->dCoef, b->dKM, r.sOut, r.segK, r.th0, c.nJ, 3, 3, t1);
   hipLaunchKernelGGL(k_out_invkin, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, r.Kc, r.th0, t1);
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
   int rc = uploadChannelSeries(c, r, 6, false);
   if (rc) return rc;
   solveSeries(c, r, r.Kc * 6, r.th0, 1, r.sol1);
   hipLaunchKernelGGL(k_out_trq, grid256(t1), dim3(OUT_BS), 0, st, c.P, r.dPaths, r.Kc, r.th0, r.sol1, r.th1, t1);
   return BATOTP_OK;
}

// BA::q2aaVect (ba.cpp:1920-1927): quaternion rows -> axis-angle rows, the result loses the seventh Cartesian row
static int poseToAxisAngle(const OutCall &c, OutRoute &r)
{
   batotp_ctx *ctx = c.ctx;
   hipStream_t st = c.st;
   const int64_t tF = r.L.tF;
   const double *atDev = nullptr;
   if (c.hostTrig)
   {
      double *packQ = r.w.take<double>((size_t)tF * 2), *atTab = r.w.take<double>((size_t)tF);
      if (r.w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "output stage: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
      hipLaunchKernelGGL(k_out_q_norm, grid256(tF), dim3(OUT_BS), 0, st, c.nJ, c.R, r.dPaths, r.Kc, r.result, packQ, tF);
      ctx->kinTheta.resize((size_t)tF * 2);
      ctx->kinTrig.resize((size_t)tF);
      HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), packQ, sizeof(double) * (size_t)tF * 2, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (const OutPath &q : r.L.pc)
      {
         const int64_t off = q.offF, n = q.nF;
         for (int64_t i = 0; i < n; ++i)   // util.cpp:573: one atan2() per point, host libm
            ctx->kinTrig[(size_t)(off + i)] = ::atan2(ctx->kinTheta[(size_t)(off * 2 + i)], ctx->kinTheta[(size_t)(off * 2 + n + i)]);
      }
      HIP_TRY(hipMemcpyAsync(atTab, ctx->kinTrig.data(), sizeof(double) * (size_t)tF, hipMemcpyHostToDevice, st));
      atDev = atTab;
   }
   hipLaunchKernelGGL(k_out_q2aa, grid256(tF), dim3(OUT_BS), 0, st, c.nJ, c.R, r.dPaths, r.Kc, r.result, atDev, r.resultOut, tF);
   HIP_TRY(hipGetLastError());
   return BATOTP_OK;
}

// smoothing + down-sampling, re-interpolation at the user's resolution, and the rows into their place in the result
static int finishRoute(const OutCall &c, OutRoute &r)
{
   hipStream_t st = c.st;
   const int64_t tF = r.L.tF;
   if (r.smoothing) hipLaunchKernelGGL(k_out_down, grid256(r.L.t2), dim3(OUT_BS), 0, st, c.P, r.dPaths, r.Kc, r.th1, r.th2, r.L.t2);
   HIP_TRY(hipGetLastError());
   if (r.reinterp)
   {
      HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten
      int rc = uploadChannelSeries(c, r, c.R, true);
      if (rc) return rc;
      solveSeries(c, r, r.Kc * c.R, r.th2, 1, r.sol2);
      hipLaunchKernelGGL(k_out_user, grid256(tF), dim3(OUT_BS), 0, st, c.P, r.dPaths, r.Kc, r.th2, r.sol2, r.result, tF);
      HIP_TRY(hipGetLastError());
   }
   if (c.pose) return poseToAxisAngle(c, r);
   if (r.L.staged)
   {
      hipLaunchKernelGGL(k_out_place, grid256(tF), dim3(OUT_BS), 0, st, c.R, r.dPaths, r.Kc, r.result, r.resultOut, tF);
      HIP_TRY(hipGetLastError());
   }
   return BATOTP_OK;
}

extern "C" int batotp_hip_output(batotp_batch *b, const batotp_output_params *prm, int32_t path0, int32_t n_paths, batotp_output **out)
{
   if (!b || !prm || !out || path0 < 0 || n_paths < 1 || path0 + n_paths > b->B) return BATOTP_ERR_ARG;
   *out = nullptr;
   OutCall c;
   int rc = outputCall(b, prm, path0, n_paths, c);
   if (rc) return rc;
   batotp_ctx *ctx = c.ctx;
   hipStream_t st = c.st;
   const int K = n_paths;

   std::vector<batotp_path_result> res(b->B);
   HIP_TRY(hipMemcpyAsync(res.data(), b->dRes, sizeof(batotp_path_result) * b->B, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st));

   std::vector<double> h(K);
   for (int k = 0; k < K; ++k) h[k] = prm->integ_res == BATOTP_OUT_STEP_PER_PATH ? b->pinfo[path0 + k].integ_res : prm->integ_res;
   OutPlan pl;
   planOutput(res.data() + path0, h.data(), K, path0, prm->out_res, prm->out_smooth_fact, pl);

   OutputOwner own;
   batotp_output *o = own.o = new (std::nothrow) batotp_output;
   if (!o) return BATOTP_ERR_ALLOC;
   o->ctx = ctx; o->K = K; o->nJ = c.Rout; o->nTheta = c.nJ; o->nCart = c.pose ? 6 : c.nCartRows; o->nTrq = c.nTrqRows;
   o->n = pl.n; o->off = pl.off; o->sres = pl.sres;
   o->total = pl.totF;
   const size_t resultBytes = sizeof(double) * (size_t)std::max<int64_t>(pl.totF * c.Rout, 1);
   hipError_t e = hipMalloc((void **)&o->dTheta, resultBytes);
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (output trajectories)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, o->dTheta, resultBytes, st))) return rc;

   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   cutChunks(pl, OutRows{c.R, c.cable || c.serialTrq, c.pose}, budget);
   if ((rc = arenaReserve(ctx->ws[1], pl.maxChunk + 4096, st))) return rc;
   Event ev0, ev1;
   HIP_TRY(hipEventCreate(&ev0.e));
   HIP_TRY(hipEventCreate(&ev1.e));
   HIP_TRY(hipEventRecord(ev0.e, st));

   for (size_t ci = 0; ci + 1 < pl.cuts.size(); ++ci)
      for (int route = 0; route < 4; ++route)
      {
         const int ka = pl.cuts[ci], kb = pl.cuts[ci + 1];
         OutRoute r;
         r.L = routeLayout(pl, ka, kb, route);
         if (r.L.t1 == 0) continue; // no path of the chunk takes this route, or every one that would failed in the sweep
         if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc; // (every route starts from poisoned scratch)
         if ((rc = carveRoute(c, route, o->dTheta + pl.all[ka].offF * c.Rout, r))) return rc;
         if ((rc = sampleS(c, r))) return rc;
         if ((rc = c.cable ? evalCable(c, r) : evalJoints(c, r))) return rc;
         if ((rc = finishRoute(c, r))) return rc;
         HIP_TRY(hipStreamSynchronize(st)); // the host vectors go out of scope, the scratch is reused by the next route or chunk
      }
   HIP_TRY(hipEventRecord(ev1.e, st));
   HIP_TRY(hipStreamSynchronize(st));
   HIP_TRY(hipEventElapsedTime(&o->ms, ev0.e, ev1.e));
   *out = o;
   own.o = nullptr;
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
