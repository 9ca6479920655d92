// kin_api.inc -- host side of include/batotp_hip_kin.h (included at the end of batotp_hip.hip): the checks of a kinematic
// chain, the known-answer entry of its tool point, and the two places a chain is handed to -- the resampler (resampleRun,
// resample_api.inc) and a batch for its output stage (outputCall / evalJoints, output_api.inc).

// BATOTP_ERR_ARG with a message for a chain no kernel may see
static int kinChainCheck(const batotp_kin_chain *ch, const char *who)
{
   if (!ch) return BATOTP_ERR_ARG;
   if (ch->n_links < 1 || ch->n_links > BATOTP_MAX_LINKS)
   {
      snprintf(g_err, sizeof(g_err), "%s: a kinematic chain has 1 to %d links, not %d", who, BATOTP_MAX_LINKS, (int)ch->n_links);
      return BATOTP_ERR_ARG;
   }
   for (int i = 0; i < ch->n_links; ++i)
   {
      const double *a = ch->axis[i], *o = ch->off[i];
      for (int j = 0; j < 3; ++j)
         if (!std::isfinite(a[j]) || !std::isfinite(o[j]))
         {
            snprintf(g_err, sizeof(g_err), "%s: link %d of the kinematic chain has an entry that is not finite", who, i);
            return BATOTP_ERR_ARG;
         }
      const double nn = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
      if (!(fabs(nn - 1.0) <= 1e-12))
      {
         snprintf(g_err, sizeof(g_err), "%s: joint axis %d of the kinematic chain is not a unit vector", who, i);
         return BATOTP_ERR_ARG;
      }
   }
   for (int j = 0; j < 3; ++j)
      if (!std::isfinite(ch->tool[j]))
      {
         snprintf(g_err, sizeof(g_err), "%s: the tool point of the kinematic chain is not finite", who);
         return BATOTP_ERR_ARG;
      }
   return BATOTP_OK;
}

extern "C" int batotp_hip_kin_chain_from_model(const batotp_serial_model *model, const double tool[3], batotp_kin_chain *out)
{
   if (!model || !tool || !out) return BATOTP_ERR_ARG;
   if (model->n_links < 1 || model->n_links > BATOTP_MAX_LINKS)
   {
      snprintf(g_err, sizeof(g_err), "kin_chain_from_model: a model has 1 to %d links, not %d", BATOTP_MAX_LINKS, (int)model->n_links);
      return BATOTP_ERR_ARG;
   }
   batotp_kin_chain c;
   batotp_kin_chain_of_model(model, tool, &c);
   int rc = kinChainCheck(&c, "kin_chain_from_model");
   if (rc) return rc;
   *out = c;
   return BATOTP_OK;
}

extern "C" int batotp_hip_builtin_kin_chain(int32_t robot_type, batotp_kin_chain *out)
{
   if (!out) return BATOTP_ERR_ARG;
   if (batotp_builtin_kin_chain(robot_type, out) != 0)
   {
      snprintf(g_err, sizeof(g_err), "builtin_kin_chain: robot type %d has no built-in kinematic chain", (int)robot_type);
      return BATOTP_ERR_ARG;
   }
   return BATOTP_OK;
}

// The point lists become a stage of the resampler -- [n_links + 3][n] per path, described by RsPath rows -- and go through
// rsFwdKin, the function the resampler's three call sites use: same packing kernel, same host tables, same launch.
extern "C" int batotp_hip_fwdkin_chain(batotp_ctx *ctx, const batotp_kin_chain *chain, uint32_t flags, int32_t n_paths, const int64_t *n_pts,
                                       const double *theta, double *cart_out)
{
   if (!ctx || !chain || !n_pts || !theta || !cart_out || n_paths < 1) return BATOTP_ERR_ARG;
   int rc = kinChainCheck(chain, "fwdkin_chain");
   if (rc) return rc;
   const int nJ = chain->n_links, C = nJ + 3, B = n_paths;
   std::vector<RsPath> paths((size_t)B);
   int64_t total = 0;
   for (int p = 0; p < B; ++p)
   {
      if (n_pts[p] < 0 || n_pts[p] > (int64_t)1 << 30) return BATOTP_ERR_ARG;
      memset(&paths[p], 0, sizeof(RsPath));
      paths[p].off = total; paths[p].n = (int32_t)n_pts[p]; paths[p].n0 = paths[p].n;
      total += n_pts[p];
   }
   if (total < 1 || total > (int64_t)1 << 30) return BATOTP_ERR_ARG;
   if ((rc = bind(ctx))) return rc;
   hipStream_t st = ctx->stream;
   RsParams P;
   memset(&P, 0, sizeof(P));
   P.nJ = nJ; P.nC = 3; P.C = C; P.pathType = BATOTP_PATH_JOINT; P.degrees = chain->degrees;
   struct Dev { void *p = nullptr; ~Dev() { if (p) (void)hipFree(p); } } dX, dP;
   HIP_TRY(hipMalloc(&dX.p, sizeof(double) * (size_t)total * C));
   HIP_TRY(hipMalloc(&dP.p, sizeof(RsPath) * (size_t)B));
   if ((rc = poisonFill(ctx, dX.p, sizeof(double) * (size_t)total * C, st))) return rc;
   double *x = (double *)dX.p;
   // the caller's rows [n_links][n] per path into the joint rows of the stage, the Cartesian rows back from it
   const double *src = theta;
   for (int p = 0; p < B; ++p)
   {
      const size_t cnt = (size_t)n_pts[p] * nJ;
      if (cnt) HIP_TRY(hipMemcpyAsync(x + paths[p].off * C, src, sizeof(double) * cnt, hipMemcpyHostToDevice, st));
      src += cnt;
   }
   HIP_TRY(hipMemcpyAsync(dP.p, paths.data(), sizeof(RsPath) * (size_t)B, hipMemcpyHostToDevice, st));
   if ((rc = rsFwdKin(ctx, P, chain, (flags & BATOTP_F_HOST_TRIG) != 0, paths, (const RsPath *)dP.p, x, total))) return rc;
   double *dst = cart_out;
   for (int p = 0; p < B; ++p)
   {
      const size_t cnt = (size_t)n_pts[p] * 3;
      if (cnt) HIP_TRY(hipMemcpyAsync(dst, x + paths[p].off * C + (int64_t)nJ * n_pts[p], sizeof(double) * cnt, hipMemcpyDeviceToHost, st));
      dst += cnt;
   }
   HIP_TRY(hipStreamSynchronize(st));
   return BATOTP_OK;
}

extern "C" int batotp_hip_resample_chain(batotp_ctx *ctx, const batotp_resample_params *prm, const batotp_kin_chain *chain, int32_t n_paths,
                                         const int64_t *n_in, const double *x, const double *sres_in, batotp_resampled **out)
{
   if (out) *out = nullptr;
   if (!ctx || !prm || !chain || !out) return BATOTP_ERR_ARG;
   int rc = kinChainCheck(chain, "resample_chain");
   if (rc) return rc;
   if (prm->path_type != BATOTP_PATH_JOINT)
   {
      snprintf(g_err, sizeof(g_err), "resample_chain: a kinematic chain serves JOINT paths (path type %d)", (int)prm->path_type);
      return BATOTP_ERR_ARG;
   }
   if (prm->n_cart != 3)
   {
      snprintf(g_err, sizeof(g_err), "resample_chain: the tool point has 3 Cartesian rows, the parameters say %d", (int)prm->n_cart);
      return BATOTP_ERR_ARG;
   }
   if (chain->n_links != prm->n_joints)
   {
      snprintf(g_err, sizeof(g_err), "resample_chain: the chain has %d links, the paths %d joints", (int)chain->n_links, (int)prm->n_joints);
      return BATOTP_ERR_ARG;
   }
   return resampleRun(ctx, prm, chain, n_paths, n_in, x, sres_in, out);
}

extern "C" int batotp_hip_set_kin_chain(batotp_batch *b, const batotp_kin_chain *chain)
{
   if (!b || !chain) return BATOTP_ERR_ARG;
   int rc = kinChainCheck(chain, "set_kin_chain");
   if (rc) return rc;
   if (chain->n_links != b->P.nJ)
   {
      snprintf(g_err, sizeof(g_err), "set_kin_chain: the chain has %d links, the batch %d joints", (int)chain->n_links, (int)b->P.nJ);
      return BATOTP_ERR_ARG;
   }
   if (b->prob.n_cart < 3)
   {
      snprintf(g_err, sizeof(g_err), "set_kin_chain: the batch carries %d Cartesian channels, a tool point needs 3", (int)b->prob.n_cart);
      return BATOTP_ERR_ARG;
   }
   b->kinChain = *chain;
   b->hasKinChain = true;
   return BATOTP_OK;
}
