// duty_api.inc -- host side of include/batotp_hip_duty.h (included at the end of batotp_hip.hip, after the torque scale's): the
// refusals of a call, what rangeRun (range_run.inc) needs to know of a duty pass -- the partials of a range on top of those of the
// torque scale, and the three launches -- and what a round of StretchRounds (stretch_api.inc) evaluates here: torque rows, scale
// records and duty sums in one pass, then the audit of the result.  The host rule is duty_rounds.h.

// everything a call refuses of its ratings; the reciprocals and limits the host rule reads
static int dutyCheck(const batotp_serial_model *model, const double *rated, double target, const char *what, DutyRating &R)
{
   if (!(target > 0.0 && target <= 1.0))
   {
      snprintf(g_err, sizeof(g_err), "%s: target is in (0, 1]", what);
      return BATOTP_ERR_ARG;
   }
   for (int j = 0; j < model->n_links; ++j)
      if (!(std::isfinite(rated[j]) && rated[j] > 0.0))
      {
         snprintf(g_err, sizeof(g_err), "%s: the rated torque of joint %d is not finite and positive", what, j);
         return BATOTP_ERR_ARG;
      }
   dutyRating(model->n_links, rated, target, R);
   return BATOTP_OK;
}

static size_t dutyPathBytes(int64_t n, int nl, bool hostTrig)
{
   return tscalePathBytes(n, nl, hostTrig) + (sizeof(double) * DUTY_QS + sizeof(DutyPeak)) * (size_t)blocksOf(n, DUTY_BP);
}

// o (checked) with torque rows: a new output in *out, the scale records of its K paths in dScale and their sums in dSums (device);
// ms and launches are ADDED to the two counters.  A path without points must get its records, so a range without blocks still
// runs the two finish kernels.
static int dutyRun(batotp_output *o, const batotp_serial_model *model, uint32_t flags, const TscaleConst &C, batotp_output **out,
                   batotp_path_tscale *dScale, batotp_path_duty_sums *dSums, float &msSum, int &launches)
{
   const bool hostTrig = (flags & BATOTP_F_HOST_TRIG) != 0;
   const int nl = model->n_links, nCart = o->nCart, Rout = o->nTheta + nCart + nl;
   TorqueScratch ts{model, hostTrig};
   TscalePartial *dPartials = nullptr;
   double *dBlockSums = nullptr;
   DutyPeak *dPeaks = nullptr;
   RangeJob<TscalePath> job{"output_duty", "hipMalloc (output with torque rows)", &batotp_output::fromDuty, o->n.data(), Rout, nl, DUTY_BP,
                            granule(sizeof(batotp_serial_model)) + 12 * 256 + 4096, true};
   job.pathBytes = [=](int64_t n) { return dutyPathBytes(n, nl, hostTrig); };
   job.fill = [=](const OutRange &rg, int k, int64_t firstBlock, TscalePath &p) { invdynPathFill(o, k, rg.pts, p.p); p.pOff = firstBlock; };
   job.take = [&](OutRange &rg) {
      ts.take(rg);
      dPartials = rg.w.take<TscalePartial>(rg.nBlocks);
      dBlockSums = rg.w.take<double>(rg.nBlocks * DUTY_QS);
      dPeaks = rg.w.take<DutyPeak>(rg.nBlocks);
   };
   job.prepare = [&](OutRange &rg, float &ms) { return ts.prepare(rg, (int)sizeof(TscalePath), ms); };
   job.launch = [&](OutRange &rg) {
      const TscalePath *dPaths = (const TscalePath *)rg.dPaths;
      const int Kc = rg.kb - rg.ka;
      if (rg.nBlocks > 0)
         hipLaunchKernelGGL(k_duty, dim3((unsigned)rg.nBlocks), dim3(DUTY_THREADS), 0, rg.ctx->stream, ts.dModel, C, dPaths, rg.dBlocks, (int)rg.nBlocks,
                            (const double *)o->dTheta, nCart, (const double *)ts.trig, rg.r->dTheta, dPartials, dBlockSums, dPeaks);
      hipLaunchKernelGGL(k_tscale_finish, dim3((unsigned)Kc), dim3(64), 0, rg.ctx->stream, dPaths, Kc, (const TscalePartial *)dPartials, dScale + rg.ka);
      hipLaunchKernelGGL(k_duty_finish, dim3((unsigned)Kc), dim3(64), 0, rg.ctx->stream, dPaths, Kc, (const double *)dBlockSums, (const DutyPeak *)dPeaks,
                         dSums + rg.ka);
   };
   return rangeRun(o, job, out, msSum, launches);
}

// bounds of the scale candidate for a call that has no torque range: none binds, no point is static
static void dutyOpenBounds(TscaleConst &C)
{
   for (int j = 0; j < BATOTP_MAX_LINKS; ++j) { C.hi[j] = std::numeric_limits<double>::infinity(); C.lo[j] = -std::numeric_limits<double>::infinity(); }
}

extern "C" int batotp_hip_output_duty(batotp_output *o, const batotp_serial_model *model, uint32_t flags, const double *rated, double target,
                                      batotp_output **out, batotp_path_duty *duty, batotp_path_duty_sums *sums)
{
   if (out) *out = nullptr;
   if (!o || !model || !rated || !out || (!duty && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_duty: NULL argument");
      return BATOTP_ERR_ARG;
   }
   if (flags & ~(uint32_t)BATOTP_F_HOST_TRIG)
   {
      snprintf(g_err, sizeof(g_err), "output_duty: flags 0x%x: only BATOTP_F_HOST_TRIG is understood", (unsigned)flags);
      return BATOTP_ERR_ARG;
   }
   int rc = stretchSourceCheck(o, "output_duty");
   if (rc) return rc;
   if ((rc = invdynModelCheck(model, o->nTheta))) return rc;
   DutyRating R;
   if ((rc = dutyCheck(model, rated, target, "output_duty", R))) return rc;
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   DevMem dRecs;
   const size_t scaleBytes = sizeof(batotp_path_tscale) * (size_t)K, sumBytes = sizeof(batotp_path_duty_sums) * (size_t)K;
   if ((rc = dRecs.alloc(sumBytes + scaleBytes, "hipMalloc (records of the duty pass)"))) return rc;
   TscaleConst C;
   dutyOpenBounds(C);
   float ms = 0.f;
   int launches = 0;
   OutputOwner r;
   if ((rc = dutyRun(o, model, flags, C, &r.o, (batotp_path_tscale *)((char *)dRecs.p + sumBytes), (batotp_path_duty_sums *)dRecs.p, ms, launches))) return rc;
   if (K > 0)
   {
      std::vector<batotp_path_duty_sums> own;
      if (!sums) { own.resize((size_t)K); sums = own.data(); }
      hipStream_t st = o->ctx->stream;
      HIP_TRY(hipMemcpyAsync(sums, dRecs.p, sumBytes, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int k = 0; k < K; ++k) dutyRecord(sums[k], R, o->sres[k], duty[k]);
   }
   r.o->dutyMs = ms; r.o->dutyRanges = launches;
   *out = r.release();
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_duty(batotp_output *o, const batotp_problem *prob, const batotp_serial_model *model, uint32_t flags,
                                              const double *rated, double target, int32_t max_rounds, double max_factor, batotp_output **out,
                                              batotp_path_stretch *report, batotp_path_tscale *scale, batotp_path_duty *duty)
{
   if (out) *out = nullptr;
   if (!o || !prob || !model || !rated || !out || (!report && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_duty: NULL argument");
      return BATOTP_ERR_ARG;
   }
   if (!(target > 0.0 && target <= 1.0) || max_rounds < 1 || max_rounds > 16 || !(std::isfinite(max_factor) && max_factor >= 1.0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_duty: target is in (0, 1], max_rounds in 1..16, max_factor finite and >= 1");
      return BATOTP_ERR_ARG;
   }
   TscaleConst C;
   batotp_problem probTrq;
   int rc = tscaleCheck(o, prob, model, flags, target, "output_stretch_duty", C, probTrq);
   if (rc) return rc;
   DutyRating R;
   if ((rc = dutyCheck(model, rated, target, "output_stretch_duty", R))) return rc;
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   hipStream_t st = o->ctx->stream;

   // one buffer, one copy per round: the audit records, the scale records, the sums
   DevMem dRecs;
   const size_t auditBytes = sizeof(batotp_path_audit) * (size_t)K, scaleBytes = sizeof(batotp_path_tscale) * (size_t)K,
                sumBytes = sizeof(batotp_path_duty_sums) * (size_t)K;
   if ((rc = dRecs.alloc(auditBytes + scaleBytes + sumBytes, "hipMalloc (records of the duty pass)"))) return rc;
   batotp_path_tscale *dScale = (batotp_path_tscale *)((char *)dRecs.p + auditBytes);
   batotp_path_duty_sums *dSums = (batotp_path_duty_sums *)((char *)dRecs.p + auditBytes + scaleBytes);
   std::vector<char> host(auditBytes + scaleBytes + sumBytes);
   const batotp_path_tscale *hScale = (const batotp_path_tscale *)(host.data() + auditBytes);
   const batotp_path_duty_sums *hSums = (const batotp_path_duty_sums *)(host.data() + auditBytes + scaleBytes);
   std::vector<batotp_path_duty> hDuty((size_t)K);

   OutputOwner trq; // the rows of the round with their torques
   float ms = 0.f;
   int launches = 0;
   StretchRounds Rn;
   Rn.duty = hDuty.data();
   rc = Rn.run(o, target, max_rounds, max_factor, [&](batotp_output *rows, const batotp_path_audit *&recs, const batotp_path_tscale *&srec) {
      recs = (const batotp_path_audit *)host.data();
      srec = hScale;
      batotp_hip_output_destroy(trq.release());
      int rc = dutyRun(rows, model, flags, C, &trq.o, dScale, dSums, ms, launches);
      if (rc || K == 0) return rc;
      if ((rc = auditRun(trq.o, &probTrq, 0.0, dRecs.p, nullptr))) return rc;
      HIP_TRY(hipMemcpyAsync(host.data(), dRecs.p, host.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int k = 0; k < K; ++k) dutyRecord(hSums[k], R, o->sres[k], hDuty[k]);
      return (int)BATOTP_OK;
   });
   if (rc) return rc;
   Rn.report(o, report);
   for (int k = 0; k < K; ++k)
   {
      if (scale) scale[k] = hScale[k];
      if (duty) duty[k] = hDuty[k];
   }
   trq.o->dutyMs = ms; trq.o->dutyRanges = launches;
   *out = trq.release();
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_duty_ms(batotp_output *out, float *ms)
{
   if (!out || !ms) return BATOTP_ERR_ARG;
   if (!out->fromDuty) return BATOTP_ERR_STATE;
   *ms = out->dutyMs;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_duty_ranges(batotp_output *out, int32_t *n)
{
   if (!out || !n) return BATOTP_ERR_ARG;
   if (!out->fromDuty) return BATOTP_ERR_STATE;
   *n = out->dutyRanges;
   return BATOTP_OK;
}
