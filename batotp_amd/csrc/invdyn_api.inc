// invdyn_api.inc -- host side of include/batotp_hip_invdyn.h (included at the end of batotp_hip.hip): the refusals of a call, the
// ranges of paths whose tables fit the workspace budget, and per range the descriptor tables, the host trig tables
// (BATOTP_F_HOST_TRIG: the route of tableFor in output_api.inc -- packed joint rows to the host, hostTrigTables of kind 2 over
// spans, the tables back) and the launch.  A range's tables are indexed from the range's first point, the rows of the source and
// of the result from the output's: nothing a lane computes depends on where the ranges are cut.

// BATOTP_ERR_ARG with a message for a model no kernel may see
static int invdynModelCheck(const batotp_serial_model *m, int nTheta)
{
   if (m->n_links < 1 || m->n_links > BATOTP_MAX_LINKS)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: a model has 1 to %d links, not %d", BATOTP_MAX_LINKS, (int)m->n_links);
      return BATOTP_ERR_ARG;
   }
   if (m->n_links != nTheta)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: the model has %d links, the output %d joint rows", (int)m->n_links, nTheta);
      return BATOTP_ERR_ARG;
   }
   bool ok = std::isfinite(m->gravity[0]) && std::isfinite(m->gravity[1]) && std::isfinite(m->gravity[2]);
   if (!ok)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: the gravity vector of the model is not finite");
      return BATOTP_ERR_ARG;
   }
   for (int i = 0; i < m->n_links; ++i)
   {
      const batotp_serial_link &L = m->link[i];
      ok = std::isfinite(L.mass) && std::isfinite(L.fv);
      for (int j = 0; j < 3; ++j) ok = ok && std::isfinite(L.axis[j]) && std::isfinite(L.off[j]) && std::isfinite(L.com[j]);
      for (int j = 0; j < 6; ++j) ok = ok && std::isfinite(L.inertia[j]);
      if (!ok)
      {
         snprintf(g_err, sizeof(g_err), "output_torques: link %d of the model has an entry that is not finite", i);
         return BATOTP_ERR_ARG;
      }
      const double nn = L.axis[0] * L.axis[0] + L.axis[1] * L.axis[1] + L.axis[2] * L.axis[2];
      if (!(fabs(nn - 1.0) <= 1e-12)) // the rule of kinChainCheck
      {
         snprintf(g_err, sizeof(g_err), "output_torques: joint axis %d of the model is not a unit vector", i);
         return BATOTP_ERR_ARG;
      }
   }
   return BATOTP_OK;
}

// scratch bytes of path k in a range: its descriptors and, with host tables, packed joint rows [nl][n] and tables [2 nl][n]
static size_t invdynPathBytes(int64_t n, int nl, bool hostTrig)
{
   const size_t nb = (size_t)((n + INVDYN_BP - 1) / INVDYN_BP);
   return sizeof(InvdynPath) + sizeof(InvdynBlock) * nb + (hostTrig ? sizeof(double) * (size_t)n * 3 * (size_t)nl : 0);
}

extern "C" int batotp_hip_output_torques(batotp_output *o, const batotp_serial_model *model, uint32_t flags, batotp_output **out)
{
   if (out) *out = nullptr;
   if (!o || !model || !out)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: NULL argument");
      return BATOTP_ERR_ARG;
   }
   if (flags & ~(uint32_t)BATOTP_F_HOST_TRIG)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: flags 0x%x: only BATOTP_F_HOST_TRIG is understood", (unsigned)flags);
      return BATOTP_ERR_ARG;
   }
   if (o->nTrq != 0)
   {
      snprintf(g_err, sizeof(g_err), "output_torques: the output already has %d torque rows", o->nTrq);
      return BATOTP_ERR_ARG;
   }
   int rc = invdynModelCheck(model, o->nTheta);
   if (rc) return rc;
   if ((rc = bind(o->ctx))) return rc;
   batotp_ctx *ctx = o->ctx;
   hipStream_t st = ctx->stream;
   const bool hostTrig = (flags & BATOTP_F_HOST_TRIG) != 0;
   const int K = o->K, nl = model->n_links, nCart = o->nCart, Rin = o->nTheta + o->nCart, Rout = Rin + nl;

   struct Owner { batotp_output *o; ~Owner() { batotp_hip_output_destroy(o); } } own{new (std::nothrow) batotp_output};
   batotp_output *r = own.o;
   if (!r) return BATOTP_ERR_ALLOC;
   r->ctx = ctx; r->K = K; r->nJ = Rout; r->nTheta = o->nTheta; r->nCart = nCart; r->nTrq = nl;
   r->n = o->n; r->off = o->off; r->sres = o->sres; r->total = o->total;
   r->fromTorques = true;
   const size_t resultBytes = sizeof(double) * (size_t)std::max<int64_t>(o->total * Rout, 1);
   hipError_t e = hipMalloc((void **)&r->dTheta, resultBytes);
   if (e != hipSuccess)
   {
      hipFail(e, "hipMalloc (output with torque rows)");
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, r->dTheta, resultBytes, st))) return rc;
   if (o->total == 0) { *out = r; own.o = nullptr; return BATOTP_OK; }

   // ranges of consecutive paths whose scratch fits the budget, at least one path each (as cutChunks, output_plan.h)
   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   std::vector<int> cuts(1, 0);
   size_t bytes = 0, maxRange = 0;
   for (int k = 0; k < K; ++k)
   {
      const size_t need = invdynPathBytes(o->n[k], nl, hostTrig);
      if (k > cuts.back() && (double)(bytes + need) > budget) { cuts.push_back(k); bytes = 0; }
      bytes += need;
      maxRange = std::max(maxRange, bytes);
   }
   cuts.push_back(K);
   if ((rc = arenaReserve(ctx->ws[1], maxRange + granule(sizeof(batotp_serial_model)) + 8 * 256 + 4096, st))) return rc;

   struct Event { hipEvent_t e = nullptr; ~Event() { if (e) hipEventDestroy(e); } } ev[4];
   for (Event &v : ev) HIP_TRY(hipEventCreate(&v.e));
   std::vector<InvdynPath> paths;
   std::vector<InvdynBlock> blocks;
   std::vector<TrigSpan> spans;
   for (size_t ci = 0; ci + 1 < cuts.size(); ++ci)
   {
      const int ka = cuts[ci], kb = cuts[ci + 1], Kc = kb - ka;
      paths.assign((size_t)Kc, InvdynPath());
      blocks.clear();
      spans.clear();
      int64_t pts = 0;
      for (int k = ka; k < kb; ++k)
      {
         const double h = o->sres[k];
         InvdynPath &p = paths[k - ka];
         p.off = o->off[k]; p.n = o->n[k]; p.tOff = pts;
         p.c1 = 1.0 / (2.0 * h); p.c2 = 1.0 / (h * h);
         const int64_t nb = (o->n[k] + INVDYN_BP - 1) / INVDYN_BP;
         for (int64_t b = 0; b < nb; ++b) blocks.push_back(InvdynBlock{k - ka, (int32_t)b});
         spans.push_back(TrigSpan{pts, o->n[k], o->n[k] == 0});
         pts += o->n[k];
      }
      const size_t nBlocks = blocks.size();
      if (nBlocks == 0) continue; // a range of empty paths
      if (nBlocks > 0x7fffffff) { snprintf(g_err, sizeof(g_err), "output_torques: too many blocks"); return BATOTP_ERR_ARG; }
      if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;
      Bump w;
      w.base = (char *)ctx->ws[1].p;
      batotp_serial_model *dModel = w.take<batotp_serial_model>(1);
      InvdynPath *dPaths = w.take<InvdynPath>((size_t)Kc);
      InvdynBlock *dBlocks = w.take<InvdynBlock>(nBlocks);
      // an output without Cartesian rows is the packed array already: the range's paths are contiguous in it
      double *pack = (hostTrig && nCart > 0) ? w.take<double>((size_t)pts * nl) : nullptr;
      double *trig = hostTrig ? w.take<double>((size_t)pts * 2 * nl) : nullptr;
      if (w.at > ctx->ws[1].cap) { snprintf(g_err, sizeof(g_err), "output_torques: scratch estimate exceeded"); return BATOTP_ERR_STATE; }
      HIP_TRY(hipMemcpyAsync(dModel, model, sizeof(*model), hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dPaths, paths.data(), sizeof(InvdynPath) * (size_t)Kc, hipMemcpyHostToDevice, st));
      HIP_TRY(hipMemcpyAsync(dBlocks, blocks.data(), sizeof(InvdynBlock) * nBlocks, hipMemcpyHostToDevice, st));
      float msPack = 0.f, msKernel = 0.f;
      if (hostTrig)
      {
         const double *packed = o->dTheta + o->off[ka] * Rin;
         if (pack)
         {
            HIP_TRY(hipEventRecord(ev[0].e, st));
            hipLaunchKernelGGL(k_invdyn_pack, dim3((unsigned)nBlocks), dim3(INVDYN_THREADS), 0, st, dPaths, dBlocks, (int)nBlocks, o->dTheta, nl, nCart, pack);
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
      HIP_TRY(hipEventRecord(ev[2].e, st));
      hipLaunchKernelGGL(k_invdyn, dim3((unsigned)nBlocks), dim3(INVDYN_THREADS), 0, st, dModel, dPaths, dBlocks, (int)nBlocks, o->dTheta, nCart, trig, r->dTheta);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev[3].e, st));
      HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors and the host tables are rewritten by the next range
      HIP_TRY(hipEventElapsedTime(&msKernel, ev[2].e, ev[3].e));
      r->trqMs += msPack + msKernel;
      ++r->trqRanges;
   }
   *out = r;
   own.o = nullptr;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_torques_ms(batotp_output *out, float *ms)
{
   if (!out || !ms) return BATOTP_ERR_ARG;
   if (!out->fromTorques) return BATOTP_ERR_STATE;
   *ms = out->trqMs;
   return BATOTP_OK;
}

extern "C" int batotp_hip_output_torques_ranges(batotp_output *out, int32_t *n_ranges)
{
   if (!out || !n_ranges) return BATOTP_ERR_ARG;
   if (!out->fromTorques) return BATOTP_ERR_STATE;
   *n_ranges = out->trqRanges;
   return BATOTP_OK;
}
