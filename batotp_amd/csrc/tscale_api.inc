// tscale_api.inc -- host side of include/batotp_hip_tscale.h (included at the end of batotp_hip.hip, after the stretch's): the refusals
// of a call, the bounds, the ranges of paths whose tables fit the workspace budget (as invdyn_api.inc cuts them) with the host trig
// tables per range, and the rounds -- those of batotp_hip_output_stretch_audit (stretch_api.inc) with the torque family on top.  A
// range's tables and partials are indexed from the range's first point, the rows from the output's: nothing depends on the cut.

// everything a call refuses before anything is launched or allocated; the bounds and the problem the results are audited against
static int tscaleCheck(const batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model, uint32_t flags, double target,
                       const char *what, TscaleConst &C, batotp_problem &probTrq)
{
   if (flags & ~(uint32_t)BATOTP_F_HOST_TRIG)
   {
      snprintf(g_err, sizeof(g_err), "%s: flags 0x%x: only BATOTP_F_HOST_TRIG is understood", what, (unsigned)flags);
      return BATOTP_ERR_ARG;
   }
   if (!(target > 0.0 && target <= 1.0))
   {
      snprintf(g_err, sizeof(g_err), "%s: target is in (0, 1]", what);
      return BATOTP_ERR_ARG;
   }
   int rc = stretchSourceCheck(o, what);
   if (rc) return rc;
   if ((rc = invdynModelCheck(model, o->nTheta))) return rc;
   if (prob->flags & BATOTP_F_PARALLEL)
   {
      snprintf(g_err, sizeof(g_err), "%s: the problem is a parallel mechanism: the torque rows of a chain model are not its actuator forces", what);
      return BATOTP_ERR_ARG;
   }
   {
      AuditConst A; // everything the audit refuses
      if ((rc = auditConst(o, prob, 0.0, A))) return rc;
   }
   memset(&C, 0, sizeof(C));
   for (int j = 0; j < model->n_links; ++j)
   {
      const double mid = (prob->jnt_trq_max[j] + prob->jnt_trq_min[j]) * 0.5;
      const double half = (prob->jnt_trq_max[j] - prob->jnt_trq_min[j]) * 0.5;
      if (!(std::isfinite(mid) && std::isfinite(half) && half > 0.0))
      {
         snprintf(g_err, sizeof(g_err), "%s: the torque range of joint %d is not finite and positive", what, j);
         return BATOTP_ERR_ARG;
      }
      C.hi[j] = mid + target * half;
      C.lo[j] = mid - target * half;
   }
   probTrq = *prob;
   probTrq.flags |= BATOTP_F_TRQ_ON;
   return BATOTP_OK;
}

// scratch bytes of a path in a range: descriptors, partials and, with host tables, packed joint rows [nl][n] and tables [2 nl][n]
static size_t tscalePathBytes(int64_t n, int nl, bool hostTrig)
{
   const size_t nb = (size_t)((n + TSCALE_BP - 1) / TSCALE_BP);
   return sizeof(TscalePath) + (sizeof(TscaleBlock) + sizeof(TscalePartial)) * nb + (hostTrig ? sizeof(double) * (size_t)n * 3 * (size_t)nl : 0);
}

// o (checked) with torque rows: a new output in *out, the records of its K paths in dScale (device); ms and launches are ADDED to
// the two counters
static int tscaleRun(batotp_output *o, const batotp_serial_model *model, uint32_t flags, const TscaleConst &C, batotp_output **out,
                     batotp_path_tscale *dScale, float &msSum, int &launches)
{
   int rc = bind(o->ctx);
   if (rc) return rc;
   batotp_ctx *ctx = o->ctx;
   hipStream_t st = ctx->stream;
   const bool hostTrig = (flags & BATOTP_F_HOST_TRIG) != 0;
   const int K = o->K, nl = model->n_links, nCart = o->nCart, Rin = o->nTheta + o->nCart, Rout = Rin + nl;

   struct Owner { batotp_output *o; ~Owner() { batotp_hip_output_destroy(o); } } own{new (std::nothrow) batotp_output};
   batotp_output *r = own.o;
   if (!r) return BATOTP_ERR_ALLOC;
   r->ctx = ctx; r->K = K; r->nJ = Rout; r->nTheta = o->nTheta; r->nCart = nCart; r->nTrq = nl;
   r->n = o->n; r->off = o->off; r->sres = o->sres; r->total = o->total;
   r->fromTscale = true;
   const size_t resultBytes = sizeof(double) * (size_t)std::max<int64_t>(o->total * Rout, 1);
   hipError_t e = hipMalloc((void **)&r->dTheta, resultBytes);
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (output with torque rows)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, r->dTheta, resultBytes, st))) return rc;

   // ranges of consecutive paths whose scratch fits the budget, at least one path each (as invdyn_api.inc)
   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   std::vector<int> cuts(1, 0);
   size_t bytes = 0, maxRange = 0;
   for (int k = 0; k < K; ++k)
   {
      const size_t need = tscalePathBytes(o->n[k], nl, hostTrig);
      if (k > cuts.back() && (double)(bytes + need) > budget) { cuts.push_back(k); bytes = 0; }
      bytes += need;
      maxRange = std::max(maxRange, bytes);
   }
   cuts.push_back(K);
   if ((rc = arenaReserve(ctx->ws[1], maxRange + granule(sizeof(batotp_serial_model)) + 10 * 256 + 4096, st))) return rc;

   struct Event { hipEvent_t e = nullptr; ~Event() { if (e) hipEventDestroy(e); } } ev[4];
   for (Event &v : ev) HIP_TRY(hipEventCreate(&v.e));
   std::vector<TscalePath> paths;
   std::vector<TscaleBlock> blocks;
   std::vector<TrigSpan> spans;
   for (size_t ci = 0; ci + 1 < cuts.size(); ++ci)
   {
      const int ka = cuts[ci], kb = cuts[ci + 1], Kc = kb - ka;
      if (Kc == 0) continue; // an output without paths
      paths.assign((size_t)Kc, TscalePath());
      blocks.clear();
      spans.clear();
      int64_t pts = 0;
      for (int k = ka; k < kb; ++k)
      {
         const double h = o->sres[k];
         TscalePath &p = paths[k - ka];
         p.off = o->off[k]; p.n = o->n[k]; p.tOff = pts; p.pOff = (int64_t)blocks.size();
         p.c1 = 1.0 / (2.0 * h); p.c2 = 1.0 / (h * h);
         const int64_t nb = (o->n[k] + TSCALE_BP - 1) / TSCALE_BP;
         if (nb > 0x7fffffff) { snprintf(g_err, sizeof(g_err), "output_torque_scale: too many blocks"); return BATOTP_ERR_ARG; }
         for (int64_t b = 0; b < nb; ++b) blocks.push_back(TscaleBlock{k - ka, (int32_t)b});
         spans.push_back(TrigSpan{pts, o->n[k], o->n[k] == 0});
         pts += o->n[k];
      }
      const size_t nBlocks = blocks.size();
      if (nBlocks > 0x7fffffff) { snprintf(g_err, sizeof(g_err), "output_torque_scale: too many blocks"); return BATOTP_ERR_ARG; }
      if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;
      Bump w;
      w.base = (char *)ctx->ws[1].p;
      batotp_serial_model *dModel = w.take<batotp_serial_model>(1);
      TscalePath *dPaths = w.take<TscalePath>((size_t)Kc);
      TscaleBlock *dBlocks = w.take<TscaleBlock>(std::max<size_t>(nBlocks, 1));
      TscalePartial *dPartials = w.take<TscalePartial>(std::max<size_t>(nBlocks, 1));
      // an output without Cartesian rows is the packed array already: the range's paths are contiguous in it
      double *pack = (hostTrig && nCart > 0 && pts > 0) ? w.take<double>((size_t)pts * nl) : nullptr;
      double *trig = (hostTrig && pts > 0) ? w.take<double>((size_t)pts * 2 * nl) : nullptr;
      if (w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "output_torque_scale: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
      HIP_TRY(hipMemcpyAsync(dPaths, paths.data(), sizeof(TscalePath) * (size_t)Kc, hipMemcpyHostToDevice, st));
      float msPack = 0.f, msKernel = 0.f;
      if (nBlocks > 0)
      {
         HIP_TRY(hipMemcpyAsync(dModel, model, sizeof(*model), hipMemcpyHostToDevice, st));
         HIP_TRY(hipMemcpyAsync(dBlocks, blocks.data(), sizeof(TscaleBlock) * nBlocks, hipMemcpyHostToDevice, st));
         if (hostTrig)
         {
            const double *packed = o->dTheta + o->off[ka] * Rin;
            if (pack)
            {
               HIP_TRY(hipEventRecord(ev[0].e, st));
               hipLaunchKernelGGL(k_tscale_pack, dim3((unsigned)nBlocks), dim3(TSCALE_THREADS), 0, st, dPaths, dBlocks, (int)nBlocks, o->dTheta, nl, nCart, pack);
               HIP_TRY(hipGetLastError());
               HIP_TRY(hipEventRecord(ev[1].e, st));
               packed = pack;
            }
            ctx->kinTheta.resize((size_t)pts * nl);
            ctx->kinTrig.resize((size_t)pts * 2 * nl);
            HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), packed, sizeof(double) * ctx->kinTheta.size(), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (pack) HIP_TRY(hipEventElapsedTime(&msPack, ev[0].e, ev[1].e));
            hostTrigTables(2, 0, nl, model->degrees ? KIN_DEG2RAD : 1.0, spans, ctx->kinTheta.data(), ctx->kinTrig.data());
            HIP_TRY(hipMemcpyAsync(trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, st));
         }
      }
      HIP_TRY(hipEventRecord(ev[2].e, st));
      if (nBlocks > 0)
         hipLaunchKernelGGL(k_tscale, dim3((unsigned)nBlocks), dim3(TSCALE_THREADS), 0, st, dModel, C, dPaths, dBlocks, (int)nBlocks, o->dTheta, nCart, trig, r->dTheta,
                            dPartials);
      hipLaunchKernelGGL(k_tscale_finish, dim3((unsigned)Kc), dim3(64), 0, st, dPaths, Kc, dPartials, dScale + ka); // a path without points: "none"
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev[3].e, st));
      HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors and the host tables are rewritten by the next range
      HIP_TRY(hipEventElapsedTime(&msKernel, ev[2].e, ev[3].e));
      msSum += msPack + msKernel;
      if (nBlocks > 0) ++launches;
   }
   *out = r;
   own.o = nullptr;
   return BATOTP_OK;
}

// device memory of a call's records, freed when the call returns
struct TscaleRecs
{
   void *p = nullptr;
   ~TscaleRecs() { if (p) hipFree(p); }
   int alloc(size_t bytes)
   {
      hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 1));
      if (e == hipSuccess) return BATOTP_OK;
      p = nullptr;
      hipFail(e, "hipMalloc (records of the torque scale)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
};

extern "C" int batotp_hip_output_torque_scale(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model, uint32_t flags, double target,
                                              batotp_output **out, batotp_path_tscale *scale)
{
   if (out) *out = nullptr;
   if (!o || !prob || !model || !out || (!scale && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_torque_scale: NULL argument");
      return BATOTP_ERR_ARG;
   }
   TscaleConst C;
   batotp_problem probTrq;
   int rc = tscaleCheck(o, prob, model, flags, target, "output_torque_scale", C, probTrq);
   if (rc) return rc;
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   TscaleRecs dRecs;
   if ((rc = dRecs.alloc(sizeof(batotp_path_tscale) * (size_t)K))) return rc;
   float ms = 0.f;
   int launches = 0;
   batotp_output *r = nullptr;
   if ((rc = tscaleRun(o, model, flags, C, &r, (batotp_path_tscale *)dRecs.p, ms, launches))) return rc;
   if (K > 0)
   {
      hipStream_t st = o->ctx->stream;
      hipError_t e = hipMemcpyAsync(scale, dRecs.p, sizeof(batotp_path_tscale) * (size_t)K, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) { batotp_hip_output_destroy(r); HIP_TRY(e); }
   }
   r->tscaleMs = ms; r->tscaleRanges = launches;
   *out = r;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_torques(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model, uint32_t flags, double target,
                                                 int32_t max_rounds, double max_factor, batotp_output **out, batotp_path_stretch *report,
                                                 batotp_path_tscale *scale)
{
   if (out) *out = nullptr;
   if (!o || !prob || !model || !out || (!report && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_torques: NULL argument");
      return BATOTP_ERR_ARG;
   }
   if (!(target > 0.0 && target <= 1.0) || max_rounds < 1 || max_rounds > 16 || !(std::isfinite(max_factor) && max_factor >= 1.0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_torques: target is in (0, 1], max_rounds in 1..16, max_factor finite and >= 1");
      return BATOTP_ERR_ARG;
   }
   TscaleConst C;
   batotp_problem probTrq;
   int rc = tscaleCheck(o, prob, model, flags, target, "output_stretch_torques", C, probTrq);
   if (rc) return rc;
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   hipStream_t st = o->ctx->stream;

   // one buffer, one copy per round: the audit records, then the scale records
   TscaleRecs dRecs;
   const size_t auditBytes = sizeof(batotp_path_audit) * (size_t)K, scaleBytes = sizeof(batotp_path_tscale) * (size_t)K;
   if ((rc = dRecs.alloc(auditBytes + scaleBytes))) return rc;
   batotp_path_tscale *dScale = (batotp_path_tscale *)((char *)dRecs.p + auditBytes);
   std::vector<char> host(auditBytes + scaleBytes);
   const batotp_path_audit *recs = (const batotp_path_audit *)host.data();
   const batotp_path_tscale *srec = (const batotp_path_tscale *)(host.data() + auditBytes);

   std::vector<int64_t> n2(o->n);
   std::vector<int32_t> rounds((size_t)K, 0), status((size_t)K, BATOTP_STRETCH_PASSES);
   std::vector<char> capped((size_t)K, 0);
   struct Current { batotp_output *o = nullptr; ~Current() { batotp_hip_output_destroy(o); } } cur, trq; // the stretched rows so far (never o itself); with torques
   float ms = 0.f, msStretch = 0.f;
   int launches = 0, launchesStretch = 0;
   const int velFam[2] = {BATOTP_AUDIT_JNT_VEL, BATOTP_AUDIT_CART_VEL}, accFam[2] = {BATOTP_AUDIT_JNT_ACC, BATOTP_AUDIT_CART_ACC};
   for (;;)
   {
      batotp_hip_output_destroy(trq.o);
      trq.o = nullptr;
      if ((rc = tscaleRun(cur.o ? cur.o : o, model, flags, C, &trq.o, dScale, ms, launches))) return rc;
      if (K > 0)
      {
         if ((rc = auditRun(trq.o, &probTrq, 0.0, dRecs.p, nullptr))) return rc;
         HIP_TRY(hipMemcpyAsync(host.data(), dRecs.p, auditBytes + scaleBytes, hipMemcpyDeviceToHost, st));
         HIP_TRY(hipStreamSynchronize(st));
      }
      bool again = false;
      for (int k = 0; k < K; ++k)
      {
         const batotp_path_audit &a = recs[k];
         const batotp_path_tscale &t = srec[k];
         double need = 1.0;
         bool pass = true;
         for (int f : velFam)
            if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, a.fam[f].peak / target); }
         for (int f : accFam)
            if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, sqrt(a.fam[f].peak / target)); }
         const bool kinPass = pass, trqPass = a.fam[BATOTP_AUDIT_TRQ].peak <= target; // -1: not audited, or nothing to evaluate
         if (!trqPass)
         {
            pass = false;
            if (t.n_static == 0 && t.s < 1.0) need = std::max(need, 1.0 / t.s);
         }
         if (pass) { status[k] = BATOTP_STRETCH_PASSES; continue; }
         if (!trqPass && t.n_static > 0 && kinPass) { status[k] = BATOTP_STRETCH_STATIC; continue; }
         if (capped[k]) { status[k] = BATOTP_STRETCH_CAPPED; continue; }
         if (rounds[k] >= max_rounds) { status[k] = BATOTP_STRETCH_ROUNDS; continue; }
         const int64_t m = n2[k] - 1;
         double intervals = std::max(ceil((double)m * need), (double)(m + 1));
         const double bound = std::min(floor((double)(o->n[k] - 1) * max_factor), (double)(BATOTP_STRETCH_MAX_POINTS - 1));
         if (intervals > bound) { intervals = bound; capped[k] = 1; status[k] = BATOTP_STRETCH_CAPPED; }
         const int64_t nNew = (int64_t)intervals + 1;
         if (nNew == n2[k]) continue; // capped where it stands
         n2[k] = nNew;
         ++rounds[k];
         again = true;
      }
      if (!again) break;
      batotp_output *next = nullptr;
      if ((rc = stretchRun(o, n2.data(), &next, msStretch, launchesStretch))) return rc;
      batotp_hip_output_destroy(cur.o);
      cur.o = next;
   }
   for (int k = 0; k < K; ++k)
   {
      batotp_path_stretch &s = report[k];
      s.n_in = o->n[k]; s.n_out = n2[k];
      s.factor = o->n[k] < 2 ? 1.0 : (double)(n2[k] - 1) / (double)(o->n[k] - 1);
      s.rounds = rounds[k]; s.status = status[k];
      if (scale) scale[k] = srec[k];
   }
   trq.o->tscaleMs = ms; trq.o->tscaleRanges = launches;
   *out = trq.o;
   trq.o = nullptr;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_tscale_ms(batotp_output *out, float *ms)
{
   if (!out || !ms) return BATOTP_ERR_ARG;
   if (!out->fromTscale) return BATOTP_ERR_STATE;
   *ms = out->tscaleMs;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_tscale_ranges(batotp_output *out, int32_t *n)
{
   if (!out || !n) return BATOTP_ERR_ARG;
   if (!out->fromTscale) return BATOTP_ERR_STATE;
   *n = out->tscaleRanges;
   return BATOTP_OK;
}
