// The workgroup and mesh-topology primitives that fusion.hip, mesh.hip, mesh_simplify.hip, mesh_smooth.hip, mesh_clean.hip,
// cloud_dist.hip, cloud_knn.hip, cloud_register.hip, texture.hip, texture_level.hip and the raster stages (dsm_buildings.hip,
// dsm_roofs.hip, dsm_trees.hip, dsm_contours.hip; what only they share is in raster_prims.h) share: the 256-lane tile count, ranks and
// scans over a workgroup of four waves, wave reductions in a fixed butterfly order, undirected edge keys, half-edges, the
// run-of-one test on sorted keys and the walk to the root of a label forest.  Integer work and plain additions only: several
// includers switch fp contraction off after their includes, and a helper that multiplies and then adds floats would round
// differently from one includer to the next.
#pragma once
#include "common.h"
#include "kernels.h"

namespace adamvs {

static_assert(FUSION_TILE == 256 && MESH_TILE == 256 && SIMPLIFY_TILE == 256 && SMOOTH_TILE == 256 && CLEAN_TILE == 256 &&
                  CLOUD_TILE == 256 && TEX_TILE == 256,
              "tiles256 and the ballot / scan / LDS layouts below assume workgroups of four waves of 64");

// workgroups of 256 lanes that cover n elements
static inline unsigned tiles256(long n) { return (unsigned)((n + 255) / 256); }

// ---- ranks and scans over the workgroup -----------------------------------------------------------------------------------
// rank of a lane among the lanes of its wave that are set in the ballot and sit below it
__device__ __forceinline__ unsigned lane_rank(unsigned long long bal) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// rank of a flagged lane among the flagged lanes of its workgroup (every lane must call it); *total = their number
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned* total) {
  __shared__ unsigned wave_n[4];
  const unsigned long long bal = __ballot(flag);
  unsigned rank = lane_rank(bal);
  if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = (unsigned)__popcll(bal);
  __syncthreads();
  const int wv = threadIdx.x >> 6;
  for (int i = 0; i < wv; ++i) rank += wave_n[i];
  *total = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
  return rank;
}

// exclusive scan of v over the workgroup (256 lanes); *total = the sum.  Every lane must call it.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* total) {
  __shared__ unsigned wave_sum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned inc = v;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_sum[wv] = inc;
  __syncthreads();
  unsigned base = 0;
  for (int i = 0; i < wv; ++i) base += wave_sum[i];
  *total = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
  return base + inc - v;
}

// ---- wave reductions: a fixed butterfly (32, 16, .. 1), so every lane holds the same bits and a sum is stable from run to run
__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int off = 32; off >= 1; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_min(int x) {
  for (int m = 32; m >= 1; m >>= 1) {
    const int y = __shfl_xor(x, m);
    x = y < x ? y : x;
  }
  return x;
}
__device__ __forceinline__ int wave_max(int x) {
  for (int m = 32; m >= 1; m >>= 1) {
    const int y = __shfl_xor(x, m);
    x = y > x ? y : x;
  }
  return x;
}

// ---- mesh topology ----------------------------------------------------------------------------------------------------------
// the undirected edge (a, b) as  min << 32 | max  (unsigned: a vertex number with bit 31 set stays in its half)
__device__ __forceinline__ long long edge_key(unsigned a, unsigned b) {
  const unsigned lo = a < b ? a : b, hi = a < b ? b : a;
  return (long long)(((unsigned long long)lo << 32) | hi);
}

// half-edge h = 3 f + k runs from corner k of face f to corner (k + 1) % 3
__device__ __forceinline__ void half_edge(const unsigned* __restrict__ faces, long h, unsigned& tail, unsigned& head) {
  const long s = h / 3;
  const int k = (int)(h - 3 * s);
  tail = faces[3 * s + k];
  head = faces[3 * s + (k == 2 ? 0 : k + 1)];
}

// whether keys[i] differs from both of its neighbours in the SORTED keys [0, n)
__device__ __forceinline__ bool key_occurs_once(const long long* __restrict__ keys, long i, long n) {
  const long long key = keys[i];
  return !((i > 0 && keys[i - 1] == key) || (i + 1 < n && keys[i + 1] == key));
}

// Entry v of a label forest to its root.  parent[x] <= x everywhere and other lanes only lower their own entries to ancestors:
// the walk ends at the root.  Strictly downwards, so it ends (and stays inside [0, v]) whatever the caller passed.
__device__ __forceinline__ void compress_to_root(int* parent, long v) {
  const int p0 = parent[v];
  if (p0 < 0 || (long)p0 > v) return;
  int p = p0;
  for (int q = parent[p]; q >= 0 && q < p; q = parent[p]) p = q;
  if (p != p0) parent[v] = p;
}

}  // namespace adamvs
