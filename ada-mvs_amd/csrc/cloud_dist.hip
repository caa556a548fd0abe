// Cloud distance: the bounded nearest neighbour of every query among the targets, and a deterministic surface sampler, so that
// clouds and meshes can be scored against a truth (include/adamvs_hip.h "Cloud distance" states every operation).  The caller
// (ada-mvs_amd/accuracy.py) keys both clouds on the lattice of side c = D (adamvs_simplify_keys), sorts them stably, numbers the
// occupied target cells (unique) and cuts the sorted queries into work items of one cell and at most 256 queries
// (ada-mvs_amd/cloud_lattice.py).  cloud_lattice.h holds the walk that cloud_knn.hip shares: the nine rows of a work item, the
// candidate tiles in the LDS, the split of the lanes into slices, the pair arithmetic and the keep rule, and on the host the keyed,
// sorted cloud and the candidates of a query; here:
//
//   k_cloud_nearest       one 256-lane workgroup per work item walks the item's candidates (CloudWalk) in tiles of 256; each slice
//                         sweeps its share of a tile with reads of one address per slice and keeps (d2, index) under the
//                         lexicographic rule, the slices meet in a tree, and the truncation at D closes
//   k_cloud_sample_count  one lane per face: n = max(1, ceil(longest edge / s))
//   k_cloud_sample_emit   one wave per face: the (n + 1)(n + 2) / 2 barycentric lattice points, i ascending, then j
//
// No atomics and no inter-workgroup waits: every lane writes its own element only, and the result of a query is a function of
// the targets as a set, so the output is bit-identical from run to run and under any permutation of either cloud.
#include <math.h>

#include "block_prims.h"
#include "cloud_lattice.h"
#include "common.h"
#include "kernels.h"

// The header states the arithmetic as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

__global__ __launch_bounds__(256) void k_cloud_nearest(const CloudLattice L, float limit, const long long* __restrict__ ukeys,
                                                       const long long* __restrict__ tstart, int nc, const double* __restrict__ targets,
                                                       const int* __restrict__ tindex, long nt, const double* __restrict__ queries, long nq,
                                                       const long long* __restrict__ qorder, long nqs,
                                                       const long long* __restrict__ item_key, const long long* __restrict__ item_first,
                                                       const int* __restrict__ item_count, float* __restrict__ d2, int* __restrict__ index,
                                                       unsigned long long* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) CloudWalk<CLOUD_TILE> w;
  const int lane = threadIdx.x;
  const long item = blockIdx.x;
  const long long key = item_key[item];
  const long long first = item_first[item];
  int count = item_count[item];
  count = count < 0 ? 0 : (count > CLOUD_TILE ? CLOUD_TILE : count);
  double ctr[3];
  cloud_centre(L, key < 0 ? 0 : key, ctr);
  cloud_walk_rows(w, ukeys, tstart, nc, key, nt);
  const CloudSlices sl = cloud_slices(count, CLOUD_TILE, lane);
  const int P = sl.P, S = sl.S, ql = sl.ql, slice = sl.slice;
  const long long slot = first + ql;
  long long qi = -1;
  if (ql < count && slot >= 0 && slot < nqs) qi = qorder[slot];
  const bool live = qi >= 0 && qi < nq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) {
    qx = (float)(queries[3 * qi] - ctr[0]);
    qy = (float)(queries[3 * qi + 1] - ctr[1]);
    qz = (float)(queries[3 * qi + 2] - ctr[2]);
  }
  float best = INFINITY;
  int best_idx = 0x7fffffff;
  const int total = cloud_walk_total(w);
  for (long long base = 0; base < total; base += CLOUD_TILE) {
    cloud_walk_fill(w, base, targets, tindex, nt, ctr);
    __syncthreads();
    const int n = total - base < CLOUD_TILE ? (int)(total - base) : CLOUD_TILE;
#pragma unroll 8
    for (int k = slice; k < n; k += S) {
      const CloudEntry p = w.tile[k];
      cloud_pair_update(qx, qy, qz, p.x, p.y, p.z, p.idx, best, best_idx);
    }
    __syncthreads();
  }
  // the S partial results of a query meet in a tree through the LDS (the tile is free after the last barrier); S is uniform
  for (int h = S >> 1; h >= 1; h >>= 1) {
    w.tile[lane].x = best;
    w.tile[lane].idx = best_idx;
    __syncthreads();
    if (slice < h) cloud_keep(w.tile[lane + h * P].x, w.tile[lane + h * P].idx, best, best_idx);
    __syncthreads();
  }
  if (live && slice == 0) {
    cloud_truncate(limit, best, best_idx);
    d2[qi] = best;
    index[qi] = best_idx;
  }
  if (lane == 0) pairs[item] = (unsigned long long)total * (unsigned long long)count;
}

// ---- the surface sampler ------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ double cloud_edge2(const double* a, const double* b) {
  const double x = b[0] - a[0], y = b[1] - a[1], z = b[2] - a[2];
  return (x * x + y * y) + z * z;
}

// n of a face: max(1, ceil(longest edge / s)); ADAMVS_CLOUD_MAX_SUBDIV + 1 stands for anything larger or not finite
__host__ __device__ __forceinline__ int cloud_face_n(const double* v0, const double* v1, const double* v2, double s) {
  const double e = fmax(fmax(cloud_edge2(v0, v1), cloud_edge2(v1, v2)), cloud_edge2(v2, v0));
  const double t = ceil(sqrt(e) / s);
  if (!(t <= (double)ADAMVS_CLOUD_MAX_SUBDIV)) return ADAMVS_CLOUD_MAX_SUBDIV + 1;
  return t < 1.0 ? 1 : (int)t;
}

__global__ __launch_bounds__(256) void k_cloud_sample_count(const double* __restrict__ xyz, long nv, const unsigned* __restrict__ faces,
                                                            long nf, double s, int* __restrict__ subdiv) {
  const long f = (long)blockIdx.x * CLOUD_TILE + threadIdx.x;
  if (f >= nf) return;
  const unsigned a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  int n = 0;                                   // a face with an index >= nv has no samples
  if ((long)a < nv && (long)b < nv && (long)c < nv) n = cloud_face_n(xyz + 3 * (long)a, xyz + 3 * (long)b, xyz + 3 * (long)c, s);
  subdiv[f] = n;
}

__global__ __launch_bounds__(256) void k_cloud_sample_emit(const double* __restrict__ xyz, long nv, const unsigned* __restrict__ faces,
                                                           long nf, const int* __restrict__ subdiv, const long long* __restrict__ offsets,
                                                           double* __restrict__ points, long capacity) {
  const int lane = threadIdx.x & 63;
  const long f = (long)blockIdx.x * (CLOUD_TILE / 64) + (threadIdx.x >> 6);      // the wave's face
  if (f >= nf) return;
  const int n = subdiv[f];
  const unsigned a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (n < 1 || n > ADAMVS_CLOUD_MAX_SUBDIV || (long)a >= nv || (long)b >= nv || (long)c >= nv) return;
  const long long off = offsets[f];
  double v0[3], u[3], w[3];
  for (int k = 0; k < 3; ++k) {
    v0[k] = xyz[3 * (long)a + k];
    u[k] = xyz[3 * (long)b + k] - v0[k];
    w[k] = xyz[3 * (long)c + k] - v0[k];
  }
  const double dn = (double)n;
  for (int i = 0; i <= n; ++i) {
    const long long row = off + (long long)i * (n + 1) - (long long)i * (i - 1) / 2;      // rows 0 .. i - 1 hold n + 1 - i' samples each
    const double s = (double)i / dn;
    for (int j = lane; j <= n - i; j += 64) {
      const long long q = row + j;
      if (q < 0 || q >= capacity) continue;
      const double t = (double)j / dn;
      for (int k = 0; k < 3; ++k) points[3 * q + k] = (v0[k] + s * u[k]) + t * w[k];
    }
  }
}

// ---- launches -------------------------------------------------------------------------------------------------------------------

int launch_cloud_nearest(const double* origin, double D, const long long* ukeys, const long long* tstart, int nc, const double* targets,
                         const int* tindex, long nt, const double* queries, long nq, const long long* qorder, long nqs,
                         const long long* item_key, const long long* item_first, const int* item_count, long ni, float* d2, int* index,
                         unsigned long long* pairs, hipStream_t st) {
  hipLaunchKernelGGL(k_cloud_nearest, dim3((unsigned)ni), dim3(CLOUD_TILE), 0, st, cloud_lattice(origin, D), (float)(D * D), ukeys, tstart, nc,
                     targets, tindex, nt, queries, nq, qorder, nqs, item_key, item_first, item_count, d2, index, pairs);
  ADAMVS_CHECK_LAUNCH("cloud_nearest");
  return 0;
}

int launch_cloud_sample_count(const double* xyz, long nv, const unsigned* faces, long nf, double spacing, int* subdiv, hipStream_t st) {
  hipLaunchKernelGGL(k_cloud_sample_count, dim3(tiles256(nf)), dim3(CLOUD_TILE), 0, st, xyz, nv, faces, nf, spacing, subdiv);
  ADAMVS_CHECK_LAUNCH("cloud_sample_count");
  return 0;
}

int launch_cloud_sample_emit(const double* xyz, long nv, const unsigned* faces, long nf, const int* subdiv, const long long* offsets,
                             double* points, long capacity, hipStream_t st) {
  hipLaunchKernelGGL(k_cloud_sample_emit, dim3(tiles256(nf * 64)), dim3(CLOUD_TILE), 0, st, xyz, nv, faces, nf, subdiv, offsets, points,
                     capacity);
  ADAMVS_CHECK_LAUNCH("cloud_sample_emit");
  return 0;
}

// ---- the same search on the host, for checks of the rule without a device ------------------------------------------------------
int cloud_nearest_host(const double* origin, double D, const double* targets, long nt, const double* queries, long nq, float* d2, int* index,
                       unsigned long long* pairs) {
  const CloudLattice L = cloud_lattice(origin, D);
  const float limit = (float)(D * D);
  CloudCells cells;
  if (int rc = cloud_cells_host(L, targets, nt, "cloud_nearest_host: target", cells)) return rc;
  unsigned long long evaluated = 0;
  for (long q = 0; q < nq; ++q) {
    int err;
    const long long key = cloud_key(L, queries + 3 * q, &err);
    float best = INFINITY;
    int best_idx = 0x7fffffff;
    if (!err)
      evaluated += cloud_visit_host(L, cells, targets, key, queries + 3 * q, [&](float qx, float qy, float qz, float px, float py, float pz, int idx) {
        cloud_pair_update(qx, qy, qz, px, py, pz, idx, best, best_idx);
      });
    cloud_truncate(limit, best, best_idx);
    d2[q] = best, index[q] = best_idx;
  }
  if (pairs) *pairs = evaluated;
  return 0;
}

}  // namespace adamvs
