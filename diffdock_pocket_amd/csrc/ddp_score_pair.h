// ddp_score_pair.h - the pair arithmetic of the Vinardo-form score, used by score_evaluate (ddp_pose_descent.h) for ddp_pose_score and
// the two minimisers, and by the interaction profile (ddp_profile.hip).  The constants come in ddp_score_form_t (include/ddp_hip.h,
// which states the form): the `form` member of every entry's argument struct.
#ifndef DDP_SCORE_PAIR_H
#define DDP_SCORE_PAIR_H
#include <hip/hip_runtime.h>
#include <math.h>

#include "ddp_hip.h"

// The four unweighted sums (gauss, repulsion, hydrophobic, hbond) and, with GRAD, the gradient of the weighted energy with respect to
// the first atom.
struct ScoreAcc {
  double t[4];
  double gx, gy, gz;
};

// One typed pair at centre offset (dx, dy, dz) = x_first - x_second, rsum = R_first + R_second, flag bytes fi and fj.  d^2 is tested
// against cutoff^2 before the square root and the exponential; the comparison is written so that a NaN distance goes through and
// poisons the sums.  The ramps have their slope on the open interval only; d = 0 adds the energy and no gradient.
template <bool GRAD>
__device__ __forceinline__ void score_pair(const ddp_score_form_t& A, double cut2, double dx, double dy, double dz, double rsum, unsigned fi,
                                           unsigned fj, ScoreAcc& acc) {
  const double d2 = dx * dx + dy * dy + dz * dz;
  if (d2 >= cut2) return;
  const double d = sqrt(d2);
  const double s = d - rsum;
  const double u = (s - A.gauss_offset) / A.gauss_width;
  const double ga = exp(-(u * u));
  acc.t[0] += ga;
  double de = 0.0;                                 // d(weighted energy) / ds
  if (GRAD) de = A.w_gauss * (ga * (-2.0 * u / A.gauss_width));
  if (s < 0.0) {
    acc.t[1] += s * s;
    if (GRAD) de += A.w_repulsion * (2.0 * s);
  }
  if (fi & fj & 1u) {                              // both hydrophobic
    if (s <= A.hydrophobic_good) acc.t[2] += 1.0;
    else if (s < A.hydrophobic_bad) {
      acc.t[2] += (A.hydrophobic_bad - s) / (A.hydrophobic_bad - A.hydrophobic_good);
      if (GRAD) de -= A.w_hydrophobic / (A.hydrophobic_bad - A.hydrophobic_good);
    }
  }
  if ((((fi >> 1) & (fj >> 2)) | ((fi >> 2) & (fj >> 1))) & 1u) {   // donor-acceptor, either direction
    if (s <= A.hbond_good) acc.t[3] += 1.0;
    else if (s < A.hbond_bad) {
      acc.t[3] += (A.hbond_bad - s) / (A.hbond_bad - A.hbond_good);
      if (GRAD) de -= A.w_hbond / (A.hbond_bad - A.hbond_good);
    }
  }
  if (GRAD && d != 0.0) {
    const double k = de / d;
    acc.gx += k * dx; acc.gy += k * dy; acc.gz += k * dz;
  }
}

#endif
