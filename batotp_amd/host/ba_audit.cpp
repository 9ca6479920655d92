// ba_audit.cpp -- the seam between BA::optimizeBatch and the audit of finished trajectories (include/batotp_hip_audit.h).
// This is the only file of the host library that refers to the audit entry points: the other files reach them through the
// pointer BA::setAuditTolerance leaves in the object, so a program that never asks for an audit links against any
// implementation of include/batotp_hip.h.
#include <vector>

#include "ba.h"
#include "batotp_hip_audit.h"

namespace BATOTP
{

static int auditRange(void *output, const void *problem, double tol, size_t n, BatchAudit *out)
{
   batotp_output *o = static_cast<batotp_output *>(output);
   std::vector<batotp_path_audit> rows(n);
   std::vector<int64_t> nPts(n);
   std::vector<double> sres(n);
   int rc = batotp_hip_output_audit(o, static_cast<const batotp_problem *>(problem), tol, rows.data());
   if (rc == BATOTP_OK) rc = batotp_hip_output_info(o, nPts.data(), sres.data());
   if (rc != BATOTP_OK) return rc;
   for (size_t k = 0; k < n; ++k)
   {
      BatchAudit &a = out[k];
      for (int f = 0; f < BATOTP_AUDIT_FAMILIES; ++f)
      {
         a.peak[f] = rows[k].fam[f].peak;
         a.at[f] = rows[k].fam[f].at;
         a.row[f] = rows[k].fam[f].row;
      }
      a.nPts = rows[k].n_pts; a.nOver = rows[k].n_over; a.nNonfinite = rows[k].n_nonfinite;
      a.sres = sres[k];
      a.audited = true;
   }
   return BATOTP_OK;
}

void BA::setAuditTolerance(double tol)
{
   _auditTol = tol;
   _auditFn = tol >= 0 ? &auditRange : nullptr;
}

} // namespace BATOTP
