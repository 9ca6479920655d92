// tscale_api.inc -- host side of include/batotp_hip_tscale.h (included at the end of batotp_hip.hip, after the stretch's): the refusals
// of a call, the bounds, what rangeRun (range_run.inc) needs to know of a torque scale -- the descriptors and partials of a range on
// top of TorqueScratch, and the two launches -- and what a round of StretchRounds (stretch_api.inc) evaluates here: the torque scale,
// then the audit of its result, into one buffer.

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
   return sizeof(TscalePath) + (sizeof(PathBlock) + sizeof(TscalePartial)) * (size_t)blocksOf(n, TSCALE_BP) +
          (hostTrig ? sizeof(double) * (size_t)n * 3 * (size_t)nl : 0);
}

// o (checked) with torque rows: a new output in *out, the records of its K paths in dScale (device); ms and launches are ADDED to
// the two counters.  A path without points must get the "none" record, so a range without blocks still runs k_tscale_finish.
static int tscaleRun(batotp_output *o, const batotp_serial_model *model, uint32_t flags, const TscaleConst &C, batotp_output **out,
                     batotp_path_tscale *dScale, float &msSum, int &launches)
{
   const bool hostTrig = (flags & BATOTP_F_HOST_TRIG) != 0;
   const int nl = model->n_links, nCart = o->nCart, Rout = o->nTheta + nCart + nl;
   TorqueScratch ts{model, hostTrig};
   TscalePartial *dPartials = nullptr;
   RangeJob<TscalePath> job{"output_torque_scale", "hipMalloc (output with torque rows)", &batotp_output::fromTscale, o->n.data(), Rout, nl, TSCALE_BP,
                            granule(sizeof(batotp_serial_model)) + 10 * 256 + 4096, true};
   job.pathBytes = [=](int64_t n) { return tscalePathBytes(n, nl, hostTrig); };
   job.fill = [=](const OutRange &rg, int k, int64_t firstBlock, TscalePath &p) { invdynPathFill(o, k, rg.pts, p.p); p.pOff = firstBlock; };
   job.take = [&](OutRange &rg) { ts.take(rg); dPartials = rg.w.take<TscalePartial>(rg.nBlocks); };
   job.prepare = [&](OutRange &rg, float &ms) { return ts.prepare(rg, (int)sizeof(TscalePath), ms); };
   job.launch = [&](OutRange &rg) {
      const TscalePath *dPaths = (const TscalePath *)rg.dPaths;
      const int Kc = rg.kb - rg.ka;
      if (rg.nBlocks > 0)
         hipLaunchKernelGGL(k_tscale, dim3((unsigned)rg.nBlocks), dim3(TSCALE_THREADS), 0, rg.ctx->stream, ts.dModel, C, dPaths, rg.dBlocks, (int)rg.nBlocks,
                            (const double *)o->dTheta, nCart, (const double *)ts.trig, rg.r->dTheta, dPartials);
      hipLaunchKernelGGL(k_tscale_finish, dim3((unsigned)Kc), dim3(64), 0, rg.ctx->stream, dPaths, Kc, (const TscalePartial *)dPartials, dScale + rg.ka);
   };
   return rangeRun(o, job, out, msSum, launches);
}

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
   DevMem dRecs;
   if ((rc = dRecs.alloc(sizeof(batotp_path_tscale) * (size_t)K, "hipMalloc (records of the torque scale)"))) return rc;
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
   DevMem dRecs;
   const size_t auditBytes = sizeof(batotp_path_audit) * (size_t)K, scaleBytes = sizeof(batotp_path_tscale) * (size_t)K;
   if ((rc = dRecs.alloc(auditBytes + scaleBytes, "hipMalloc (records of the torque scale)"))) return rc;
   batotp_path_tscale *dScale = (batotp_path_tscale *)((char *)dRecs.p + auditBytes);
   std::vector<char> host(auditBytes + scaleBytes);
   const batotp_path_tscale *hScale = (const batotp_path_tscale *)(host.data() + auditBytes);

   OutputOwner trq; // the rows of the round with their torques
   float ms = 0.f;
   int launches = 0;
   StretchRounds R;
   rc = R.run(o, target, max_rounds, max_factor, [&](batotp_output *rows, const batotp_path_audit *&recs, const batotp_path_tscale *&srec) {
      recs = (const batotp_path_audit *)host.data();
      srec = hScale;
      batotp_hip_output_destroy(trq.release());
      int rc = tscaleRun(rows, model, flags, C, &trq.o, dScale, ms, launches);
      if (rc || K == 0) return rc;
      if ((rc = auditRun(trq.o, &probTrq, 0.0, dRecs.p, nullptr))) return rc;
      HIP_TRY(hipMemcpyAsync(host.data(), dRecs.p, auditBytes + scaleBytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      return (int)BATOTP_OK;
   });
   if (rc) return rc;
   R.report(o, report);
   if (scale)
      for (int k = 0; k < K; ++k) scale[k] = hScale[k];
   trq.o->tscaleMs = ms; trq.o->tscaleRanges = launches;
   *out = trq.release();
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
