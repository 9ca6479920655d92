// invdyn_api.inc -- host side of include/batotp_hip_invdyn.h (included at the end of batotp_hip.hip): the refusals of a call and what
// rangeRun (range_run.inc) needs to know of it -- the bytes and the descriptor of a path, the scratch of a range (TorqueScratch: the
// model and, with BATOTP_F_HOST_TRIG, the host trig tables) and the launch.

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
   return sizeof(InvdynPath) + sizeof(PathBlock) * (size_t)blocksOf(n, INVDYN_BP) + (hostTrig ? sizeof(double) * (size_t)n * 3 * (size_t)nl : 0);
}

// what the torque kernels read of path k of o, whose range has tOff points before it
static void invdynPathFill(const batotp_output *o, int k, int64_t tOff, InvdynPath &p)
{
   const double h = o->sres[k];
   p.off = o->off[k]; p.n = o->n[k]; p.tOff = tOff;
   p.c1 = 1.0 / (2.0 * h); p.c2 = 1.0 / (h * h);
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
   const bool hostTrig = (flags & BATOTP_F_HOST_TRIG) != 0;
   const int nl = model->n_links, nCart = o->nCart, Rout = o->nTheta + nCart + nl;
   TorqueScratch ts{model, hostTrig};
   RangeJob<InvdynPath> job{"output_torques", "hipMalloc (output with torque rows)", &batotp_output::fromTorques, o->n.data(), Rout, nl, INVDYN_BP,
                            granule(sizeof(batotp_serial_model)) + 8 * 256 + 4096, false};
   job.pathBytes = [=](int64_t n) { return invdynPathBytes(n, nl, hostTrig); };
   job.fill = [=](const OutRange &rg, int k, int64_t, InvdynPath &p) { invdynPathFill(o, k, rg.pts, p); };
   job.take = [&](OutRange &rg) { ts.take(rg); };
   job.prepare = [&](OutRange &rg, float &ms) { return ts.prepare(rg, (int)sizeof(InvdynPath), ms); };
   job.launch = [&](OutRange &rg) {
      hipLaunchKernelGGL(k_invdyn, dim3((unsigned)rg.nBlocks), dim3(INVDYN_THREADS), 0, rg.ctx->stream, ts.dModel, (const InvdynPath *)rg.dPaths, rg.dBlocks,
                         (int)rg.nBlocks, (const double *)o->dTheta, nCart, (const double *)ts.trig, rg.r->dTheta);
   };
   batotp_output *r = nullptr;
   float ms = 0.f;
   int ranges = 0;
   if ((rc = rangeRun(o, job, &r, ms, ranges))) return rc;
   r->trqMs = ms; r->trqRanges = ranges;
   *out = r;
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
