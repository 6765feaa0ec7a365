// t2fit_bspline.h -- the cubic B-spline lattice rules that the bias field (t2fit_n4.hip) and the free-form deformation
// (t2fit_ffd.hip) share: a lattice of side c spans an axis of n voxels with c - 3 cells, and a voxel index touches the
// four nodes k .. k + 3.  The axis tables, the contractions and what is accumulated differ between the two and stay there.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace t2fit {

// the first node kf (a whole number) and the cell offset tau in [0, 1] of voxel index i of an axis of n.  The last index
// is the end of the last cell.  The clamp is never taken -- p is at most s - s / (n - 1), which is below s by far more
// than a rounding for any n a volume has -- so it changes no value; it keeps k + 3 inside the lattice whatever p is.
__device__ inline void bspline_node(int i, int n, int side, double& kf, double& tau) {
  const int s = side - 3;
  kf = 0.0, tau = 0.0;
  if (n > 1) {
    if (i == n - 1) {
      kf = (double)(s - 1), tau = 1.0;
    } else {
      const double p = ((double)i * (double)s) / (double)(n - 1);
      kf = floor(p);
      tau = p - kf;
      kf = kf > (double)(s - 1) ? (double)(s - 1) : kf;
    }
  }
}

__device__ inline void bspline_weights(double tau, double* b) {
  const double t2 = tau * tau, t3 = t2 * tau, om = 1.0 - tau;
  b[0] = ((om * om) * om) / 6.0;
  b[1] = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0;
  b[2] = (((-3.0 * t3 + 3.0 * t2) + 3.0 * tau) + 1.0) / 6.0;
  b[3] = t3 / 6.0;
}

// the weight of lattice node c for a voxel whose first node is k, d = c - k: selected, not indexed, so that a row
// kernel's unrolled loop over c keeps its accumulators in registers; +0.0 outside the voxel's four
__device__ inline double select_tap(int d, double w0, double w1, double w2, double w3) {
  double wc = 0.0;
  wc = d == 0 ? w0 : wc;
  wc = d == 1 ? w1 : wc;
  wc = d == 2 ? w2 : wc;
  wc = d == 3 ? w3 : wc;
  return wc;
}

}  // namespace t2fit
