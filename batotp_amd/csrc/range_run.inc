// range_run.inc -- the driver of every output that is made from an output: torque rows (invdyn_api.inc), the time stretch
// (stretch_api.inc) and the torque scale (tscale_api.inc); included at the end of batotp_hip.hip before the three.  It owns and
// poisons the result, cuts the paths into ranges whose scratch fits the workspace budget (cutRanges, output_plan.h) and, per range,
// builds and uploads the path and block descriptors, lets the caller launch between two events and waits.  A range's descriptors are
// indexed from the range's first point and block, the rows of the source and of the result from the output's: nothing a lane
// computes depends on where the ranges are cut.
#include <functional>

// one range of a call, as the callbacks of its job see it
struct OutRange
{
   batotp_ctx *ctx;
   batotp_output *o, *r;     // source and result of the call
   int ka, kb;               // the paths of the range
   int64_t pts;              // points of the result in it (while the descriptors are filled: before the path that is being filled)
   size_t nBlocks;
   void *dPaths;             // kb - ka descriptors of the job's type
   const PathBlock *dBlocks;
   Bump w;                   // the workspace behind the two tables
};

template <class Path> struct RangeJob
{
   const char *what, *resultLabel; // "output_torques", "hipMalloc (...)": the error texts
   bool batotp_output::*from;      // the flag that names the entry point in the result
   const int64_t *n;               // points per path of the result
   int rows, nTrq;                 // rows of the result, torque rows among them
   int bp;                         // points per block
   size_t slack;                   // bytes of a range besides those of its paths
   bool emptyRanges;               // true: an output without points is served like any other, and so is a range without blocks
   std::function<size_t(int64_t)> pathBytes;                     // scratch of a path with so many points in the result
   std::function<void(const OutRange &, int, int64_t, Path &)> fill; // descriptor of path k, rg.pts and so many blocks of its range before it
   std::function<void(OutRange &)> take;                         // the rest of the range's scratch, from rg.w
   std::function<int(OutRange &, float &)> prepare;              // (a range with blocks) before the timed launch; kernel ms it took
   std::function<void(OutRange &)> launch;
};

// a new output in *out; ms and launches are ADDED to the two counters (launches: the ranges that had blocks)
template <class Path> static int rangeRun(batotp_output *o, const RangeJob<Path> &job, batotp_output **out, float &msSum, int &launches)
{
   int rc = bind(o->ctx);
   if (rc) return rc;
   batotp_ctx *ctx = o->ctx;
   hipStream_t st = ctx->stream;
   const int K = o->K;

   OutputOwner own;
   batotp_output *r = own.o = new (std::nothrow) batotp_output;
   if (!r) return BATOTP_ERR_ALLOC;
   r->ctx = ctx; r->K = K; r->nJ = job.rows; r->nTheta = o->nTheta; r->nCart = o->nCart; r->nTrq = job.nTrq;
   r->n.assign(job.n, job.n + K); r->sres = o->sres; r->off.resize((size_t)K);
   int64_t total = 0;
   for (int k = 0; k < K; ++k) { r->off[k] = total; total += job.n[k]; }
   r->total = total;
   r->*job.from = true;
   const size_t resultBytes = sizeof(double) * (size_t)std::max<int64_t>(total * job.rows, 1);
   hipError_t e = hipMalloc((void **)&r->dTheta, resultBytes);
   if (e != hipSuccess)
   {
      hipFail(e, job.resultLabel);
      (void)hipGetLastError(); // reported; clear the sticky error
      return BATOTP_ERR_ALLOC;
   }
   if ((rc = poisonFill(ctx, r->dTheta, resultBytes, st))) return rc;
   if (total == 0 && !job.emptyRanges) { *out = own.release(); return BATOTP_OK; }

   size_t freeB = 0, totalB = 0;
   hipMemGetInfo(&freeB, &totalB);
   double budget = std::min(0.5 * (double)(freeB + ctx->ws[1].cap), 24.0 * 1073741824.0);
   if (ctx->outBudget > 0) budget = (double)ctx->outBudget; // batotp_hip_set_workspace_budget
   std::vector<int> cuts;
   const size_t maxRange = cutRanges(K, [&](int k) { return job.pathBytes(job.n[k]); }, budget, cuts);
   if ((rc = arenaReserve(ctx->ws[1], maxRange + job.slack, st))) return rc;

   Event ev[2];
   for (Event &v : ev) HIP_TRY(hipEventCreate(&v.e));
   std::vector<Path> paths;
   std::vector<PathBlock> blocks;
   std::vector<int64_t> first;
   for (size_t ci = 0; ci + 1 < cuts.size(); ++ci)
   {
      OutRange rg{ctx, o, r, cuts[ci], cuts[ci + 1], 0, 0, nullptr, nullptr, Bump()};
      const int Kc = rg.kb - rg.ka;
      if (!pathBlocks(job.n, rg.ka, rg.kb, job.bp, blocks, first))
      {
         snprintf(g_err, sizeof(g_err), "%s: too many blocks", job.what);
         return BATOTP_ERR_ARG;
      }
      rg.nBlocks = blocks.size();
      if (Kc == 0 || (rg.nBlocks == 0 && !job.emptyRanges)) continue; // an output without paths; a range of empty paths
      paths.assign((size_t)Kc, Path());
      for (int k = rg.ka; k < rg.kb; ++k)
      {
         job.fill(rg, k, first[k - rg.ka], paths[k - rg.ka]);
         rg.pts += job.n[k];
      }
      if ((rc = poisonFill(ctx, ctx->ws[1].p, ctx->ws[1].cap, st))) return rc;
      rg.w.base = (char *)ctx->ws[1].p;
      Path *dPaths = rg.w.take<Path>((size_t)Kc);
      PathBlock *dBlocks = rg.w.take<PathBlock>(rg.nBlocks);
      rg.dPaths = dPaths; rg.dBlocks = dBlocks;
      if (job.take) job.take(rg);
      if (rg.w.at > ctx->ws[1].cap)
      {
         snprintf(g_err, sizeof(g_err), "%s: scratch estimate exceeded", job.what);
         return BATOTP_ERR_STATE;
      }
      HIP_TRY(hipMemcpyAsync(dPaths, paths.data(), sizeof(Path) * (size_t)Kc, hipMemcpyHostToDevice, st));
      float msBefore = 0.f, msKernel = 0.f;
      if (rg.nBlocks > 0)
      {
         HIP_TRY(hipMemcpyAsync(dBlocks, blocks.data(), sizeof(PathBlock) * rg.nBlocks, hipMemcpyHostToDevice, st));
         if (job.prepare && (rc = job.prepare(rg, msBefore))) return rc;
      }
      HIP_TRY(hipEventRecord(ev[0].e, st));
      job.launch(rg);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipEventRecord(ev[1].e, st));
      HIP_TRY(hipStreamSynchronize(st)); // the descriptor vectors and the host tables are rewritten by the next range
      HIP_TRY(hipEventElapsedTime(&msKernel, ev[0].e, ev[1].e));
      msSum += msBefore + msKernel;
      if (rg.nBlocks > 0) ++launches;
   }
   *out = own.release();
   return BATOTP_OK;
}

// The chain model and the trig tables of a range of torque rows (k_invdyn, k_tscale).  With BATOTP_F_HOST_TRIG the tables come from
// the host, the route of tableFor in output_api.inc: packed joint rows to the host, hostTrigTables of kind 2 over spans, the
// tables back.
struct TorqueScratch
{
   const batotp_serial_model *model;
   bool hostTrig;
   batotp_serial_model *dModel = nullptr;
   double *pack = nullptr, *trig = nullptr;
   Event ev[2];
   std::vector<TrigSpan> spans;

   void take(OutRange &rg)
   {
      const int nl = model->n_links;
      const bool tables = hostTrig && rg.pts > 0;
      dModel = rg.w.take<batotp_serial_model>(1);
      // an output without Cartesian rows is the packed array already: the range's paths are contiguous in it
      pack = (tables && rg.o->nCart > 0) ? rg.w.take<double>((size_t)rg.pts * nl) : nullptr;
      trig = tables ? rg.w.take<double>((size_t)rg.pts * 2 * nl) : nullptr;
   }

   // pathStride: bytes of a descriptor of rg.dPaths, which begins with an InvdynPath
   int prepare(OutRange &rg, int pathStride, float &msPack)
   {
      batotp_ctx *ctx = rg.ctx;
      hipStream_t st = ctx->stream;
      batotp_output *o = rg.o;
      const int nl = model->n_links;
      HIP_TRY(hipMemcpyAsync(dModel, model, sizeof(*model), hipMemcpyHostToDevice, st));
      if (!hostTrig) return BATOTP_OK;
      const double *packed = o->dTheta + o->off[rg.ka] * (o->nTheta + o->nCart);
      if (pack)
      {
         for (Event &v : ev)
            if (!v.e) HIP_TRY(hipEventCreate(&v.e));
         HIP_TRY(hipEventRecord(ev[0].e, st));
         hipLaunchKernelGGL(k_invdyn_pack, dim3((unsigned)rg.nBlocks), dim3(INVDYN_THREADS), 0, st, (const void *)rg.dPaths, pathStride, rg.dBlocks, (int)rg.nBlocks,
                            (const double *)o->dTheta, nl, o->nCart, pack);
         HIP_TRY(hipGetLastError());
         HIP_TRY(hipEventRecord(ev[1].e, st));
         packed = pack;
      }
      spans.clear();
      int64_t pts = 0;
      for (int k = rg.ka; k < rg.kb; ++k) { spans.push_back(TrigSpan{pts, o->n[k], o->n[k] == 0}); pts += o->n[k]; }
      ctx->kinTheta.resize((size_t)pts * nl);
      ctx->kinTrig.resize((size_t)pts * 2 * nl);
      HIP_TRY(hipMemcpyAsync(ctx->kinTheta.data(), packed, sizeof(double) * ctx->kinTheta.size(), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (pack) HIP_TRY(hipEventElapsedTime(&msPack, ev[0].e, ev[1].e));
      hostTrigTables(2, 0, nl, model->degrees ? KIN_DEG2RAD : 1.0, spans, ctx->kinTheta.data(), ctx->kinTrig.data());
      HIP_TRY(hipMemcpyAsync(trig, ctx->kinTrig.data(), sizeof(double) * ctx->kinTrig.size(), hipMemcpyHostToDevice, st));
      return BATOTP_OK;
   }
};
