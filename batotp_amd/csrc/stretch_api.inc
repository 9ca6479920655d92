// stretch_api.inc -- host side of include/batotp_hip_stretch.h (included at the end of batotp_hip.hip): the refusals of a call, what
// rangeRun (range_run.inc) needs to know of a stretch -- the descriptors over the NEW points and the launch -- and the rounds of the
// audit mode, which the torque mode (tscale_api.inc) runs as well; what a round decides for a path is stretch_rounds.h.

// BATOTP_ERR_ARG with a message for an output no stretch takes
static int stretchSourceCheck(const batotp_output *o, const char *what)
{
   if (o->nTrq != 0)
   {
      snprintf(g_err, sizeof(g_err), "%s: the output has %d torque rows: stretch first, then call batotp_hip_output_torques", what, o->nTrq);
      return BATOTP_ERR_ARG;
   }
   return BATOTP_OK;
}

static int stretchCountsCheck(const batotp_output *o, const int64_t *n2, const char *what)
{
   for (int k = 0; k < o->K; ++k)
   {
      const int64_t n = o->n[k];
      if (n2[k] < n || n2[k] > BATOTP_STRETCH_MAX_POINTS || (n < 2 && n2[k] != n))
      {
         snprintf(g_err, sizeof(g_err), "%s: path %d has %lld points and cannot be brought to %lld", what, k, (long long)n, (long long)n2[k]);
         return BATOTP_ERR_ARG;
      }
   }
   return BATOTP_OK;
}

// o (checked) with n2[k] points for path k: a new output in *out; ms and launches are ADDED to the two counters
static int stretchRun(batotp_output *o, const int64_t *n2, batotp_output **out, float &msSum, int &launches)
{
   const int R = o->nJ;
   RangeJob<StretchPath> job{"output_stretch", "hipMalloc (stretched output)", &batotp_output::fromStretch, n2, R, 0, STRETCH_BP, 8 * 256 + 4096, false};
   job.pathBytes = [](int64_t n) { return sizeof(StretchPath) + sizeof(PathBlock) * (size_t)blocksOf(n, STRETCH_BP); };
   job.fill = [=](const OutRange &rg, int k, int64_t, StretchPath &p) {
      p.offIn = o->off[k]; p.nIn = o->n[k]; p.offOut = rg.r->off[k]; p.nOut = n2[k];
      p.rk = (n2[k] > 1) ? (double)(o->n[k] - 1) / (double)(n2[k] - 1) : 0.0;
   };
   job.launch = [=](OutRange &rg) {
      hipLaunchKernelGGL(k_stretch, dim3((unsigned)rg.nBlocks), dim3(STRETCH_THREADS), 0, rg.ctx->stream, (const StretchPath *)rg.dPaths, rg.dBlocks, (int)rg.nBlocks,
                         (const double *)o->dTheta, R, rg.r->dTheta);
   };
   return rangeRun(o, job, out, msSum, launches);
}

// The rounds of the two audit-driven stretches.  evaluate(rows, recs, srec) runs a round's evaluation of `rows` (o, or o stretched
// to the counts so far) and points recs at the audit records of its K paths on the host and srec at their scale records, or leaves
// srec alone where the torque family takes no part.
struct StretchRounds
{
   std::vector<int64_t> n2;
   std::vector<StretchState> state;
   OutputOwner cur;   // o stretched to n2 (never o itself); nullptr while nothing was stretched
   float ms = 0.f;    // of the stretches
   int launches = 0;
   const batotp_path_duty *duty = nullptr; // the duty records of the round's K paths, where the RMS family takes part (duty_api.inc)

   template <class Evaluate> int run(batotp_output *o, double target, int32_t max_rounds, double max_factor, Evaluate evaluate)
   {
      const int K = o->K;
      n2 = o->n;
      state.assign((size_t)K, StretchState());
      for (;;)
      {
         const batotp_path_audit *recs = nullptr;
         const batotp_path_tscale *srec = nullptr;
         int rc = evaluate(cur.o ? cur.o : o, recs, srec);
         if (rc) return rc;
         bool again = false;
         for (int k = 0; k < K; ++k)
            if (stretchDecide(recs[k], srec ? srec + k : nullptr, target, max_rounds, max_factor, o->n[k], n2[k], state[k], duty ? duty + k : nullptr))
               again = true;
         if (!again) return BATOTP_OK;
         batotp_output *next = nullptr;
         if ((rc = stretchRun(o, n2.data(), &next, ms, launches))) return rc;
         batotp_hip_output_destroy(cur.o);
         cur.o = next;
      }
   }

   void report(const batotp_output *o, batotp_path_stretch *rep) const
   {
      for (int k = 0; k < o->K; ++k) stretchReport(o->n[k], n2[k], state[k], rep[k]);
   }
};

extern "C" int batotp_hip_output_stretch_to(batotp_output *o, const int64_t *n_out, batotp_output **out)
{
   if (out) *out = nullptr;
   if (!o || !out || (!n_out && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_to: NULL argument");
      return BATOTP_ERR_ARG;
   }
   int rc = stretchSourceCheck(o, "output_stretch_to");
   if (rc) return rc;
   if ((rc = stretchCountsCheck(o, n_out, "output_stretch_to"))) return rc;
   float ms = 0.f;
   int launches = 0;
   batotp_output *r = nullptr;
   if ((rc = stretchRun(o, n_out, &r, ms, launches))) return rc;
   r->stretchMs = ms; r->stretchRanges = launches;
   *out = r;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_by(batotp_output *o, const double *factor, batotp_output **out)
{
   if (out) *out = nullptr;
   if (!o || !out || (!factor && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_by: NULL argument");
      return BATOTP_ERR_ARG;
   }
   int rc = stretchSourceCheck(o, "output_stretch_by");
   if (rc) return rc;
   std::vector<int64_t> n2((size_t)o->K);
   for (int k = 0; k < o->K; ++k)
   {
      const int64_t n = o->n[k];
      if (!(std::isfinite(factor[k]) && factor[k] >= 1.0))
      {
         snprintf(g_err, sizeof(g_err), "output_stretch_by: the factor of path %d is not finite and >= 1", k);
         return BATOTP_ERR_ARG;
      }
      if (n < 2) { n2[k] = n; continue; }
      const double iv = ceil((double)(n - 1) * factor[k]);
      if (!(iv <= (double)(BATOTP_STRETCH_MAX_POINTS - 1)))
      {
         snprintf(g_err, sizeof(g_err), "output_stretch_by: the factor of path %d gives more than 2^40 points", k);
         return BATOTP_ERR_ARG;
      }
      n2[k] = (int64_t)iv + 1;
   }
   if ((rc = stretchCountsCheck(o, n2.data(), "output_stretch_by"))) return rc;
   float ms = 0.f;
   int launches = 0;
   batotp_output *r = nullptr;
   if ((rc = stretchRun(o, n2.data(), &r, ms, launches))) return rc;
   r->stretchMs = ms; r->stretchRanges = launches;
   *out = r;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_audit(batotp_output *o, const batotp_problem *prob, double target, int32_t max_rounds, double max_factor,
                                               batotp_output **out, batotp_path_stretch *report)
{
   if (out) *out = nullptr;
   if (!o || !prob || !out || (!report && o->K > 0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_audit: NULL argument");
      return BATOTP_ERR_ARG;
   }
   if (!(target > 0.0 && target <= 1.0) || max_rounds < 1 || max_rounds > 16 || !(std::isfinite(max_factor) && max_factor >= 1.0))
   {
      snprintf(g_err, sizeof(g_err), "output_stretch_audit: target is in (0, 1], max_rounds in 1..16, max_factor finite and >= 1");
      return BATOTP_ERR_ARG;
   }
   int rc = stretchSourceCheck(o, "output_stretch_audit");
   if (rc) return rc;
   {
      AuditConst C; // everything the audit refuses, before anything is launched or allocated
      if ((rc = auditConst(o, prob, 0.0, C))) return rc;
   }
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   hipStream_t st = o->ctx->stream;

   DevMem dRecs;
   if ((rc = dRecs.alloc(sizeof(batotp_path_audit) * (size_t)K, "hipMalloc (audit records of the stretch)"))) return rc;
   std::vector<batotp_path_audit> host((size_t)K);
   StretchRounds R;
   rc = R.run(o, target, max_rounds, max_factor, [&](batotp_output *rows, const batotp_path_audit *&recs, const batotp_path_tscale *&) {
      recs = host.data();
      if (K == 0) return (int)BATOTP_OK;
      int rc = auditRun(rows, prob, 0.0, dRecs.p, nullptr);
      if (rc) return rc;
      HIP_TRY(hipMemcpyAsync(host.data(), dRecs.p, sizeof(batotp_path_audit) * (size_t)K, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      return (int)BATOTP_OK;
   });
   if (rc) return rc;
   if (!R.cur.o && (rc = stretchRun(o, R.n2.data(), &R.cur.o, R.ms, R.launches))) return rc; // nothing to stretch: the rows of o, copied
   R.report(o, report);
   R.cur.o->stretchMs = R.ms; R.cur.o->stretchRanges = R.launches;
   *out = R.cur.release();
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_ms(batotp_output *out, float *ms)
{
   if (!out || !ms) return BATOTP_ERR_ARG;
   if (!out->fromStretch) return BATOTP_ERR_STATE;
   *ms = out->stretchMs;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_stretch_ranges(batotp_output *out, int32_t *n_ranges)
{
   if (!out || !n_ranges) return BATOTP_ERR_ARG;
   if (!out->fromStretch) return BATOTP_ERR_STATE;
   *n_ranges = out->stretchRanges;
   return BATOTP_OK;
}
