// audit_api.inc -- host side of batotp_hip_output_audit (include/batotp_hip_audit.h; included at the end of batotp_hip.hip).
// Everything the kernels need follows from the output object (points, offsets and time step of every path) and the problem's
// limits, so the host forms the constant block and the tables of path and block descriptors before the first kernel, as the
// output stage plans its chunks.

// the constant block of a call; BATOTP_ERR_ARG (with a message) for what the header lists
static int auditConst(const batotp_output *o, const batotp_problem *prob, double tol, AuditConst &C)
{
   memset(&C, 0, sizeof(C));
   if (!(tol >= 0.0) || !std::isfinite(tol))
   {
      snprintf(g_err, sizeof(g_err), "audit: tol must be finite and >= 0");
      return BATOTP_ERR_ARG;
   }
   if (prob->n_joints != o->nTheta)
   {
      snprintf(g_err, sizeof(g_err), "audit: the problem has %d joints, the output %d joint rows", (int)prob->n_joints, o->nTheta);
      return BATOTP_ERR_ARG;
   }
   const int trqRows = (prob->flags & BATOTP_F_PARALLEL) ? prob->n_cart : prob->n_joints;
   if (o->nTrq > trqRows || o->nTrq > BATOTP_MAX_JOINTS || o->nTheta > BATOTP_MAX_JOINTS)
   {
      snprintf(g_err, sizeof(g_err), "audit: the output has %d torque rows, the problem %d", o->nTrq, trqRows);
      return BATOTP_ERR_ARG;
   }
   C.nTheta = o->nTheta; C.nCart = o->nCart; C.nTrq = o->nTrq; C.nPos = std::min(3, o->nCart);
   C.lim = 1.0 + tol;
   const auto good = [](double x) { return std::isfinite(x) && x > 0.0; };
   unsigned fams = 0;
   if (o->nTheta > 0) fams |= 1u << BATOTP_AUDIT_JNT_VEL; // the reference keeps joint-velocity limits always on
   if (o->nTheta > 0 && (prob->flags & BATOTP_F_JNT_ACC_ON)) fams |= 1u << BATOTP_AUDIT_JNT_ACC;
   if (o->nCart > 0 && (prob->flags & BATOTP_F_CART_VEL_ON)) fams |= 1u << BATOTP_AUDIT_CART_VEL;
   if (o->nCart > 0 && (prob->flags & BATOTP_F_CART_ACC_ON)) fams |= 1u << BATOTP_AUDIT_CART_ACC;
   if (o->nTrq > 0 && (prob->flags & BATOTP_F_TRQ_ON)) fams |= 1u << BATOTP_AUDIT_TRQ;
   C.fams = fams;
   bool ok = true;
   for (int j = 0; j < o->nTheta; ++j)
   {
      if (fams & (1u << BATOTP_AUDIT_JNT_VEL)) { ok = ok && good(prob->jnt_vel_max[j]); C.rv[j] = 1.0 / prob->jnt_vel_max[j]; }
      if (fams & (1u << BATOTP_AUDIT_JNT_ACC)) { ok = ok && good(prob->jnt_acc_max[j]); C.ra[j] = 1.0 / prob->jnt_acc_max[j]; }
   }
   if (fams & (1u << BATOTP_AUDIT_CART_VEL)) { ok = ok && good(prob->cart_vel_max); C.rcv = 1.0 / prob->cart_vel_max; }
   if (fams & (1u << BATOTP_AUDIT_CART_ACC)) { ok = ok && good(prob->cart_acc_max); C.rca = 1.0 / prob->cart_acc_max; }
   if (fams & (1u << BATOTP_AUDIT_TRQ))
      for (int r = 0; r < o->nTrq; ++r)
      {
         const double half = (prob->jnt_trq_max[r] - prob->jnt_trq_min[r]) * 0.5;
         ok = ok && good(half);
         C.mid[r] = (prob->jnt_trq_max[r] + prob->jnt_trq_min[r]) * 0.5;
         C.rt[r] = 1.0 / half;
      }
   if (!ok)
   {
      snprintf(g_err, sizeof(g_err), "audit: a limit of an audited family is not finite and positive");
      return BATOTP_ERR_ARG;
   }
   return BATOTP_OK;
}

// The two kernels of an audit -- k_audit_blocks on the table of block descriptors, k_audit_finish with a wavefront per path.  Every
// audit goes through this function, the ones of outputs made by batotp_hip_output_from_rows (the known-answer route of the tests)
// included: a test of that entry point is a test of the grids the product uses.
static void launchAudit(hipStream_t st, const AuditConst &C, const AuditPath *dPaths, int K, const PathBlock *dBlocks, int64_t nBlocks,
                        const double *rows, AuditPartial *dPartials, batotp_path_audit *dOut)
{
   if (nBlocks > 0)
      hipLaunchKernelGGL(k_audit_blocks, dim3((unsigned)nBlocks), dim3(AUDIT_THREADS), 0, st, C, dPaths, dBlocks, (int)nBlocks, rows, dPartials);
   hipLaunchKernelGGL(k_audit_finish, dim3((unsigned)K), dim3(64), 0, st, dPaths, K, dPartials, dOut);
}

// outDev: device memory for K rows, or nullptr = rows in the workspace, copied to outHost
static int auditRun(batotp_output *o, const batotp_problem *prob, double tol, void *outDev, batotp_path_audit *outHost)
{
   AuditConst C;
   int rc = auditConst(o, prob, tol, C);
   if (rc) return rc;
   if ((rc = bind(o->ctx))) return rc;
   const int K = o->K;
   if (K == 0) { o->auditMs = 0.f; o->audited = true; return BATOTP_OK; }
   batotp_ctx *ctx = o->ctx;
   hipStream_t st = ctx->stream;

   std::vector<AuditPath> paths((size_t)K);
   std::vector<PathBlock> blocks;
   std::vector<int64_t> first;
   if (!pathBlocks(o->n.data(), 0, K, AUDIT_BP, blocks, first)) { snprintf(g_err, sizeof(g_err), "audit: too many blocks"); return BATOTP_ERR_ARG; }
   const int64_t nBlocks = (int64_t)blocks.size();
   for (int k = 0; k < K; ++k)
   {
      const double h = o->sres[k];
      AuditPath &p = paths[k];
      p.off = o->off[k]; p.n = o->n[k]; p.pOff = first[k];
      p.c1 = 1.0 / (2.0 * h); p.c2 = 1.0 / (h * h);
   }

   const size_t need = granule(sizeof(AuditPath) * (size_t)K) + granule(sizeof(PathBlock) * (size_t)nBlocks) +
                       granule(sizeof(AuditPartial) * (size_t)nBlocks) + granule(sizeof(batotp_path_audit) * (size_t)K) + 4096;
   if ((rc = arenaReserve(ctx->ws[1], need, st))) return rc;
   if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;
   Bump w;
   w.base = (char *)ctx->ws[1].p;
   AuditPath *dPaths = w.take<AuditPath>((size_t)K);
   PathBlock *dBlocks = w.take<PathBlock>((size_t)nBlocks);
   AuditPartial *dPartials = w.take<AuditPartial>((size_t)nBlocks);
   batotp_path_audit *dOut = outDev ? (batotp_path_audit *)outDev : w.take<batotp_path_audit>((size_t)K);
   if (w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "audit: scratch estimate exceeded"); return BATOTP_ERR_STATE; }

   Event ev0, ev1;
   HIP_TRY(hipEventCreate(&ev0.e));
   HIP_TRY(hipEventCreate(&ev1.e));
   HIP_TRY(hipMemcpyAsync(dPaths, paths.data(), sizeof(AuditPath) * (size_t)K, hipMemcpyHostToDevice, st));
   if (nBlocks) HIP_TRY(hipMemcpyAsync(dBlocks, blocks.data(), sizeof(PathBlock) * (size_t)nBlocks, hipMemcpyHostToDevice, st));
   HIP_TRY(hipEventRecord(ev0.e, st));
   launchAudit(st, C, dPaths, K, dBlocks, nBlocks, o->dTheta, dPartials, dOut);
   HIP_TRY(hipGetLastError());
   HIP_TRY(hipEventRecord(ev1.e, st));
   if (outHost) HIP_TRY(hipMemcpyAsync(outHost, dOut, sizeof(batotp_path_audit) * (size_t)K, hipMemcpyDeviceToHost, st));
   HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors go out of scope
   HIP_TRY(hipEventElapsedTime(&o->auditMs, ev0.e, ev1.e));
   o->audited = true;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_audit(batotp_output *o, const batotp_problem *prob, double tol, batotp_path_audit *out)
{
   if (!o || !prob || !out) return BATOTP_ERR_ARG;
   return auditRun(o, prob, tol, nullptr, out);
}

extern "C" int batotp_hip_output_audit_device(batotp_output *o, const batotp_problem *prob, double tol, void *out_dev)
{
   if (!o || !prob || !out_dev) return BATOTP_ERR_ARG;
   return auditRun(o, prob, tol, out_dev, nullptr);
}

extern "C" int batotp_hip_output_audit_ms(batotp_output *o, float *ms)
{
   if (!o || !ms) return BATOTP_ERR_ARG;
   if (!o->audited) return BATOTP_ERR_STATE;
   *ms = o->auditMs;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_from_rows(batotp_ctx *ctx, int32_t n_paths, const int64_t *n_pts, const double *sres, int32_t n_theta,
                                           int32_t n_cart, int32_t n_trq, const double *rows, batotp_output **out)
{
   if (!ctx || !out || n_paths < 0 || (n_paths > 0 && (!n_pts || !sres)) || n_theta < 0 || n_theta > BATOTP_MAX_JOINTS || n_cart < 0 ||
       n_cart > BATOTP_MAX_CART || n_trq < 0 || n_trq > BATOTP_MAX_JOINTS || n_theta + n_cart + n_trq < 1)
      return BATOTP_ERR_ARG;
   const int R = n_theta + n_cart + n_trq;
   int64_t total = 0;
   for (int k = 0; k < n_paths; ++k)
   {
      if (n_pts[k] < 0 || n_pts[k] > ((int64_t)1 << 40)) return BATOTP_ERR_ARG;
      if (n_pts[k] > 0 && !(std::isfinite(sres[k]) && sres[k] > 0.0))
      {
         snprintf(g_err, sizeof(g_err), "output from rows: the step of path %d is not finite and positive", k);
         return BATOTP_ERR_ARG;
      }
      total += n_pts[k];
   }
   if (total > 0 && !rows) return BATOTP_ERR_ARG;
   *out = nullptr;
   int rc = bind(ctx);
   if (rc) return rc;
   OutputOwner own;
   batotp_output *o = own.o = new (std::nothrow) batotp_output;
   if (!o) return BATOTP_ERR_ALLOC;
   o->ctx = ctx; o->K = n_paths; o->nJ = R; o->nTheta = n_theta; o->nCart = n_cart; o->nTrq = n_trq;
   o->n.assign(n_pts, n_pts + n_paths); o->sres.assign(sres, sres + n_paths); o->off.resize((size_t)n_paths);
   int64_t at = 0;
   for (int k = 0; k < n_paths; ++k) { o->off[k] = at; at += n_pts[k]; }
   o->total = total;
   const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(total * R, 1);
   hipError_t e = hipMalloc((void **)&o->dTheta, bytes);
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (output trajectories)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if (total > 0)
   {
      HIP_TRY(hipMemcpyAsync(o->dTheta, rows, sizeof(double) * (size_t)(total * R), hipMemcpyHostToDevice, ctx->stream));
      HIP_TRY(hipStreamSynchronize(ctx->stream)); // the caller's rows are read until here
   }
   *out = own.release();
   return BATOTP_OK;
}
