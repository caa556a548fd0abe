// Cloud registration: the arithmetic of point-to-plane ICP, so that a reconstruction can be aligned to a truth before it is scored
// (include/adamvs_hip.h "Cloud registration" states every operation).  The caller (ada-mvs_amd/register.py) moves the source,
// finds every moved point's nearest target with the search of "Cloud distance", and solves the 6 x 6 system on the host from the
// 32 sums below; cloud_register.h holds the motion of a point and the terms of a pair; here:
//
//   k_rigid_apply      one lane per point: y = R (x - c) + u
//   k_icp_accumulate   one 256-lane workgroup per 256 queries: every lane forms the 32 terms of its query (zeros unless it is a
//                      pair), each term is summed over the wave by the butterfly of wave_sum and over the four waves as
//                      (W0 + W1) + (W2 + W3): partial [nb][32]
//   k_icp_reduce       one workgroup: lane l sums partial[l], partial[l + 256], .. ascending, then the same combine: sums [32]
//
// No atomics and no inter-workgroup waits: the order of every sum is fixed by the queries' order alone, so the sums are
// bit-identical from run to run and do not depend on the order of the targets.
#include <math.h>

#include <vector>

#include "block_prims.h"
#include "cloud_register.h"
#include "common.h"
#include "kernels.h"

// The header states the arithmetic as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

__global__ __launch_bounds__(256) void k_rigid_apply(const RigidMotion M, const double* __restrict__ x, long n, double* __restrict__ y) {
  const long i = (long)blockIdx.x * CLOUD_TILE + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
  double q[3];
  rigid_point(M, p, q);
  y[3 * i] = q[0], y[3 * i + 1] = q[1], y[3 * i + 2] = q[2];
}

// The workgroup's sum of every term: the wave butterfly, then (W0 + W1) + (W2 + W3); lane t < 32 writes out[t].  After the
// butterfly every lane of a wave holds the same bits, so lane t of each wave hands over term t.  Every lane must call it.
__device__ __forceinline__ void icp_block_sums(const double* term, double* __restrict__ out) {
  __shared__ double waves[4][ICP_TERMS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < ICP_TERMS; ++t) {
    const double s = wave_sum(term[t]);
    if (lane == t) waves[wv][t] = s;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < ICP_TERMS) out[t] = (waves[0][t] + waves[1][t]) + (waves[2][t] + waves[3][t]);
}

__global__ __launch_bounds__(256) void k_icp_accumulate(const IcpFrame F, const double* __restrict__ Y, const int* __restrict__ index, long nq,
                                                        const double* __restrict__ P, const double* __restrict__ N,
                                                        const unsigned char* __restrict__ flag, long nt, double* __restrict__ partial) {
  const long i = (long)blockIdx.x * CLOUD_TILE + threadIdx.x;
  double term[ICP_TERMS];
  if (i < nq) {
    icp_query_terms(F, Y, index, i, P, N, flag, nt, term);
  } else {
#pragma unroll
    for (int t = 0; t < ICP_TERMS; ++t) term[t] = 0.0;
  }
  icp_block_sums(term, partial + (long)blockIdx.x * ICP_TERMS);
}

__global__ __launch_bounds__(256) void k_icp_reduce(const double* __restrict__ partial, long nb, double* __restrict__ sums) {
  double term[ICP_TERMS];
#pragma unroll
  for (int t = 0; t < ICP_TERMS; ++t) term[t] = 0.0;
  for (long b = threadIdx.x; b < nb; b += CLOUD_TILE) {
#pragma unroll
    for (int t = 0; t < ICP_TERMS; ++t) term[t] = term[t] + partial[b * ICP_TERMS + t];
  }
  icp_block_sums(term, sums);
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
static RigidMotion rigid_motion(const double* R, const double* c, const double* u) {
  RigidMotion M;
  for (int k = 0; k < 9; ++k) M.R[k] = R[k];
  for (int k = 0; k < 3; ++k) M.c[k] = c[k], M.u[k] = u[k];
  return M;
}

static IcpFrame icp_frame(const double* c, double L, double delta) {
  IcpFrame F;
  for (int k = 0; k < 3; ++k) F.c[k] = c[k];
  F.L = L, F.delta = delta;
  return F;
}

int launch_rigid_apply(const double* R, const double* c, const double* u, const double* x, long n, double* y, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_rigid_apply, dim3(tiles256(n)), dim3(CLOUD_TILE), 0, st, rigid_motion(R, c, u), x, n, y);
  ADAMVS_CHECK_LAUNCH("rigid_apply");
  return 0;
}

int launch_icp_accumulate(const double* y, const int* index, long nq, const double* targets, const double* normals, const unsigned char* flag,
                          long nt, const double* c, double L, double delta, double* partial, hipStream_t st) {
  if (nq == 0) return 0;
  hipLaunchKernelGGL(k_icp_accumulate, dim3(tiles256(nq)), dim3(CLOUD_TILE), 0, st, icp_frame(c, L, delta), y, index, nq, targets, normals,
                     flag, nt, partial);
  ADAMVS_CHECK_LAUNCH("icp_accumulate");
  return 0;
}

int launch_icp_reduce(const double* partial, long nb, double* sums, hipStream_t st) {
  hipLaunchKernelGGL(k_icp_reduce, dim3(1), dim3(CLOUD_TILE), 0, st, partial, nb, sums);
  ADAMVS_CHECK_LAUNCH("icp_reduce");
  return 0;
}

// ---- the same on the host, for checks of the arithmetic and of the whole loop without a device ---------------------------------
int rigid_apply_host(const double* R, const double* c, const double* u, const double* x, long n, double* y) {
  const RigidMotion M = rigid_motion(R, c, u);
  for (long i = 0; i < n; ++i) rigid_point(M, x + 3 * i, y + 3 * i);
  return 0;
}

// term [256][32] of one workgroup -> out [32], in the order of icp_block_sums
static void icp_block_sums_host(const std::vector<double>& term, double* out) {
  double v[64], w[4];
  for (int t = 0; t < ICP_TERMS; ++t) {
    for (int wv = 0; wv < 4; ++wv) {
      for (int l = 0; l < 64; ++l) v[l] = term[(size_t)(64 * wv + l) * ICP_TERMS + t];
      w[wv] = icp_wave_tree(v);
    }
    out[t] = (w[0] + w[1]) + (w[2] + w[3]);
  }
}

int icp_accumulate_host(const double* y, const int* index, long nq, const double* targets, const double* normals, const unsigned char* flag,
                        long nt, const double* c, double L, double delta, double* partial) {
  const IcpFrame F = icp_frame(c, L, delta);
  std::vector<double> term((size_t)CLOUD_TILE * ICP_TERMS);
  for (long b = 0; b * CLOUD_TILE < nq; ++b) {
    for (int l = 0; l < CLOUD_TILE; ++l) {
      const long i = b * CLOUD_TILE + l;
      double* t = term.data() + (size_t)l * ICP_TERMS;
      if (i < nq) icp_query_terms(F, y, index, i, targets, normals, flag, nt, t);
      else for (int k = 0; k < ICP_TERMS; ++k) t[k] = 0.0;
    }
    icp_block_sums_host(term, partial + b * ICP_TERMS);
  }
  return 0;
}

int icp_reduce_host(const double* partial, long nb, double* sums) {
  std::vector<double> term((size_t)CLOUD_TILE * ICP_TERMS, 0.0);
  for (int l = 0; l < CLOUD_TILE; ++l)
    for (long b = l; b < nb; b += CLOUD_TILE)
      for (int t = 0; t < ICP_TERMS; ++t) term[(size_t)l * ICP_TERMS + t] = term[(size_t)l * ICP_TERMS + t] + partial[b * ICP_TERMS + t];
  icp_block_sums_host(term, sums);
  return 0;
}

}  // namespace adamvs
