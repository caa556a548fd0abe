// The arithmetic of cloud_register.hip (include/adamvs_hip.h "Cloud registration"): the rigid motion of one point and the 32 terms
// one (query, target) pair adds to the point-to-plane normal equations.  Inline and __host__ __device__: the kernels and their
// host twins run the same functions.
#pragma once
#include <math.h>

#include "common.h"
#include "kernels.h"

// The header states the arithmetic as separate roundings: no fused multiply-add in any file that includes this one.
#pragma clang fp contract(off)

namespace adamvs {

static_assert(ICP_TERMS == 32, "21 + 6 + 5 terms; the workgroup's combine writes one term per lane of half a wave");

struct RigidMotion {      // y = R (x - c) + u,  u = c + t
  double R[9], c[3], u[3];
};

struct IcpFrame {         // the pivot, the length scale of the rotation unknowns, the Huber width (<= 0: off)
  double c[3], L, delta;
};

__host__ __device__ __forceinline__ bool icp_finite3(const double* p) {
  return fabs(p[0]) <= 1.7976931348623157e308 && fabs(p[1]) <= 1.7976931348623157e308 && fabs(p[2]) <= 1.7976931348623157e308;
}

// y_k = ((R_k0 d_0 + R_k1 d_1) + R_k2 d_2) + u_k,  d = x - c
__host__ __device__ __forceinline__ void rigid_point(const RigidMotion& M, const double* x, double* y) {
  const double d0 = x[0] - M.c[0], d1 = x[1] - M.c[1], d2 = x[2] - M.c[2];
#pragma unroll
  for (int k = 0; k < 3; ++k) y[k] = ((M.R[3 * k] * d0 + M.R[3 * k + 1] * d1) + M.R[3 * k + 2] * d2) + M.u[k];
}

// the 32 terms of the pair (y, p with the normal n), in the header's order
__host__ __device__ __forceinline__ void icp_pair_terms(const IcpFrame& F, const double* y, const double* p, const double* n, double* term) {
  const double e0 = y[0] - p[0], e1 = y[1] - p[1], e2 = y[2] - p[2];
  const double r = (e0 * n[0] + e1 * n[1]) + e2 * n[2];
  const double q0 = (y[0] - F.c[0]) / F.L, q1 = (y[1] - F.c[1]) / F.L, q2 = (y[2] - F.c[2]) / F.L;
  double a[6];
  a[0] = q1 * n[2] - q2 * n[1];
  a[1] = q2 * n[0] - q0 * n[2];
  a[2] = q0 * n[1] - q1 * n[0];
  a[3] = n[0], a[4] = n[1], a[5] = n[2];
  const double ar = fabs(r);
  const double w = (!(F.delta > 0.0) || ar <= F.delta) ? 1.0 : F.delta / ar;
  int t = 0;
#pragma unroll
  for (int u = 0; u < 6; ++u) {
    const double wa = w * a[u];
#pragma unroll
    for (int v = u; v < 6; ++v) term[t++] = wa * a[v];
  }
#pragma unroll
  for (int u = 0; u < 6; ++u) term[21 + u] = (w * a[u]) * r;
  term[27] = (w * r) * r;
  term[28] = r * r;
  term[29] = (e0 * e0 + e1 * e1) + e2 * e2;
  term[30] = 1.0;
  term[31] = w;
}

// The terms of query i: those of its pair, or 32 zeros.  PAIR iff 0 <= index[i] < nt, flag[index[i]] == 0 and y_i is finite.
__host__ __device__ __forceinline__ void icp_query_terms(const IcpFrame& F, const double* __restrict__ Y, const int* __restrict__ index, long i,
                                                         const double* __restrict__ P, const double* __restrict__ N,
                                                         const unsigned char* __restrict__ flag, long nt, double* term) {
#pragma unroll
  for (int t = 0; t < ICP_TERMS; ++t) term[t] = 0.0;
  const long j = index[i];
  if (j < 0 || j >= nt || flag[j] != ADAMVS_KNN_VALID) return;
  const double y[3] = {Y[3 * i], Y[3 * i + 1], Y[3 * i + 2]};
  if (!icp_finite3(y)) return;
  const double p[3] = {P[3 * j], P[3 * j + 1], P[3 * j + 2]}, n[3] = {N[3 * j], N[3 * j + 1], N[3 * j + 2]};
  icp_pair_terms(F, y, p, n, term);
}

// block_prims.h::wave_sum on the host: the butterfly 32, 16, .. 1 leaves  v[i] + v[i + off]  in the lower half at every level
static inline double icp_wave_tree(double* v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int i = 0; i < off; ++i) v[i] = v[i] + v[i + off];
  return v[0];
}

}  // namespace adamvs
