// stretch_api.inc -- host side of include/batotp_hip_stretch.h (included at the end of batotp_hip.hip): the refusals of a call, the
// ranges of paths whose descriptor tables fit the workspace budget (as invdyn_api.inc cuts them), per range the tables over the NEW
// points and the launch, and the rounds of the audit mode.  The rows of the source and of the result are indexed from the output's
// first point, so nothing a lane computes depends on where the ranges are cut.

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
   int rc = bind(o->ctx);
   if (rc) return rc;
   batotp_ctx *ctx = o->ctx;
   hipStream_t st = ctx->stream;
   const int K = o->K, R = o->nJ;

   struct Owner { batotp_output *o; ~Owner() { batotp_hip_output_destroy(o); } } own{new (std::nothrow) batotp_output};
   batotp_output *r = own.o;
   if (!r) return BATOTP_ERR_ALLOC;
   r->ctx = ctx; r->K = K; r->nJ = R; r->nTheta = o->nTheta; r->nCart = o->nCart; r->nTrq = 0;
   r->n.assign(n2, n2 + K); r->sres = o->sres; r->off.resize((size_t)K);
   int64_t total = 0;
   for (int k = 0; k < K; ++k) { r->off[k] = total; total += n2[k]; }
   r->total = total;
   r->fromStretch = true;
   const size_t resultBytes = sizeof(double) * (size_t)std::max<int64_t>(total * R, 1);
   hipError_t e = hipMalloc((void **)&r->dTheta, resultBytes);
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (stretched output)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, r->dTheta, resultBytes, st))) return rc;
   if (total == 0) { *out = r; own.o = nullptr; return BATOTP_OK; }

   // ranges of consecutive paths whose tables fit the budget, at least one path each (as cutChunks, output_plan.h)
   const auto pathBytes = [](int64_t n) { return sizeof(StretchPath) + sizeof(StretchBlock) * (size_t)((n + STRETCH_BP - 1) / STRETCH_BP); };
   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   std::vector<int> cuts(1, 0);
   size_t bytes = 0, maxRange = 0;
   for (int k = 0; k < K; ++k)
   {
      const size_t need = pathBytes(n2[k]);
      if (k > cuts.back() && (double)(bytes + need) > budget) { cuts.push_back(k); bytes = 0; }
      bytes += need;
      maxRange = std::max(maxRange, bytes);
   }
   cuts.push_back(K);
   if ((rc = arenaReserve(ctx->ws[1], maxRange + 8 * 256 + 4096, st))) return rc;

   struct Event { hipEvent_t e = nullptr; ~Event() { if (e) hipEventDestroy(e); } } ev[2];
   for (Event &v : ev) HIP_TRY(hipEventCreate(&v.e));
   std::vector<StretchPath> paths;
   std::vector<StretchBlock> blocks;
   for (size_t ci = 0; ci + 1 < cuts.size(); ++ci)
   {
      const int ka = cuts[ci], kb = cuts[ci + 1], Kc = kb - ka;
      paths.assign((size_t)Kc, StretchPath());
      blocks.clear();
      for (int k = ka; k < kb; ++k)
      {
         StretchPath &p = paths[k - ka];
         p.offIn = o->off[k]; p.nIn = o->n[k]; p.offOut = r->off[k]; p.nOut = n2[k];
         p.rk = (n2[k] > 1) ? (double)(o->n[k] - 1) / (double)(n2[k] - 1) : 0.0;
         const int64_t nb = (n2[k] + STRETCH_BP - 1) / STRETCH_BP;
         if (nb > 0x7fffffff) { snprintf(g_err, sizeof(g_err), "output_stretch: too many blocks"); return BATOTP_ERR_ARG; }
         for (int64_t b = 0; b < nb; ++b) blocks.push_back(StretchBlock{k - ka, (int32_t)b});
      }
      const size_t nBlocks = blocks.size();
      if (nBlocks == 0) continue; // a range of empty paths
      if (nBlocks > 0x7fffffff) { snprintf(g_err, sizeof(g_err), "output_stretch: too many blocks"); return BATOTP_ERR_ARG; }
      if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;
      Bump w;
      w.base = (char *)ctx->ws[1].p;
      StretchPath *dPaths = w.take<StretchPath>((size_t)Kc);
      StretchBlock *dBlocks = w.take<StretchBlock>(nBlocks);
      if (w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "output_stretch: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
      HIP_TRY(hipMemcpyAsync(dPaths, paths.data(), sizeof(StretchPath) * (size_t)Kc, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dBlocks, blocks.data(), sizeof(StretchBlock) * nBlocks, hipMemcpyHostToDevice, st));
      HIP_TRY(hipEventRecord(ev[0].e, st));
      hipLaunchKernelGGL(k_stretch, dim3((unsigned)nBlocks), dim3(STRETCH_THREADS), 0, st, dPaths, dBlocks, (int)nBlocks, o->dTheta, R, r->dTheta);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev[1].e, st));
      HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors are rewritten by the next range
      float ms = 0.f;
      HIP_TRY(hipEventElapsedTime(&ms, ev[0].e, ev[1].e));
      msSum += ms;
      ++launches;
   }
   *out = r;
   own.o = nullptr;
   return BATOTP_OK;
}

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

   struct DevRecs { void *p = nullptr; ~DevRecs() { if (p) hipFree(p); } } dRecs;
   hipError_t e = hipMalloc(&dRecs.p, sizeof(batotp_path_audit) * (size_t)std::max(K, 1));
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (audit records of the stretch)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   std::vector<batotp_path_audit> recs((size_t)K);
   std::vector<int64_t> n2(o->n);
   std::vector<int32_t> rounds((size_t)K, 0), status((size_t)K, BATOTP_STRETCH_PASSES);
   std::vector<char> capped((size_t)K, 0);
   struct Current { batotp_output *o = nullptr; ~Current() { batotp_hip_output_destroy(o); } } cur; // the stretched result so far (never o itself)
   float ms = 0.f;
   int launches = 0;
   const int velFam[2] = {BATOTP_AUDIT_JNT_VEL, BATOTP_AUDIT_CART_VEL}, accFam[2] = {BATOTP_AUDIT_JNT_ACC, BATOTP_AUDIT_CART_ACC};
   for (;;)
   {
      if (K > 0)
      {
         if ((rc = auditRun(cur.o ? cur.o : o, prob, 0.0, dRecs.p, nullptr))) return rc;
         HIP_TRY(hipMemcpyAsync(recs.data(), dRecs.p, sizeof(batotp_path_audit) * (size_t)K, hipMemcpyDeviceToHost, st));
         HIP_TRY(hipStreamSynchronize(st));
      }
      bool again = false;
      for (int k = 0; k < K; ++k)
      {
         const batotp_path_audit &a = recs[k];
         double need = 1.0;
         bool pass = true;
         for (int f : velFam)
            if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, a.fam[f].peak / target); }
         for (int f : accFam)
            if (!(a.fam[f].peak <= target)) { pass = false; need = std::max(need, sqrt(a.fam[f].peak / target)); }
         if (pass) { status[k] = BATOTP_STRETCH_PASSES; continue; }
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
      if ((rc = stretchRun(o, n2.data(), &next, ms, launches))) return rc;
      batotp_hip_output_destroy(cur.o);
      cur.o = next;
   }
   if (!cur.o && (rc = stretchRun(o, n2.data(), &cur.o, ms, launches))) return rc; // nothing to stretch: the rows of o, copied
   for (int k = 0; k < K; ++k)
   {
      batotp_path_stretch &s = report[k];
      s.n_in = o->n[k]; s.n_out = n2[k];
      s.factor = o->n[k] < 2 ? 1.0 : (double)(n2[k] - 1) / (double)(o->n[k] - 1);
      s.rounds = rounds[k]; s.status = status[k];
   }
   cur.o->stretchMs = ms; cur.o->stretchRanges = launches;
   *out = cur.o;
   cur.o = nullptr;
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
