// Cyclic Jacobi on a symmetric 3x3 in fp64, registers only: the rotation mesh_simplify.hip (the quadric of a cell) and
// cloud_knn.hip (the covariance of a neighbourhood) share.  Both files state their arithmetic as separate roundings.
#pragma once
#include <math.h>

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace adamvs {

constexpr int JACOBI_SWEEPS = 8;        // a 3x3 is diagonal to fp64 after 5; fixed, so that the loop unrolls fully

// One Jacobi rotation of the symmetric 3x3 in the plane (p, q), r the third index; columns p and q of V follow.
__host__ __device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                                       double& v1p, double& v1q, double& v2p, double& v2q) {
  double t = 0.0;
  if (apq != 0.0) {
    const double theta = (aqq - app) / (2.0 * apq);
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));        // theta^2 = inf gives t = 0: the rotation is below fp64
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app = app - t * apq;
  aqq = aqq + t * apq;
  apq = 0.0;
  const double rp = c * arp - s * arq, rq = s * arp + c * arq;
  arp = rp, arq = rq;
  const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
  const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
  const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
  v0p = a0, v0q = b0, v1p = a1, v1q = b1, v2p = a2, v2q = b2;
}

}  // namespace adamvs
