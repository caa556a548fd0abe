// The lattice search that cloud_dist.hip (the nearest target of every query) and cloud_knn.hip (the k nearest neighbours of every
// point) share: cell centres, the nine-row search in the sorted unique keys, the pair arithmetic in fp32 and the lexicographic
// keep rule (include/adamvs_hip.h "Cloud distance", steps 1 to 4).  Inline and __host__ __device__: the kernels and their host
// twins run the same functions.
#pragma once
#include <math.h>

#include "common.h"
#include "kernels.h"

// The header states the arithmetic as separate roundings: no fused multiply-add in any file that includes this one.
#pragma clang fp contract(off)

namespace adamvs {

static_assert(CLOUD_TILE == 256, "the tile, the work item and the workgroup are 256 wide");
constexpr int CKEY_BITS = ADAMVS_SIMPLIFY_KEY_BITS;
constexpr long long CKEY_MASK = (1LL << CKEY_BITS) - 1;

struct CloudLattice {
  double o[3], c;
};

// key (>= 0) -> the centre of its cell, as mesh_simplify.hip's cell_centre
__host__ __device__ __forceinline__ void cloud_centre(const CloudLattice& L, long long key, double* ctr) {
  ctr[0] = L.o[0] + ((double)(key & CKEY_MASK) + 0.5) * L.c;
  ctr[1] = L.o[1] + ((double)((key >> CKEY_BITS) & CKEY_MASK) + 0.5) * L.c;
  ctr[2] = L.o[2] + ((double)(key >> (2 * CKEY_BITS)) + 0.5) * L.c;
}

// first position in the ascending keys [0, n) whose key is >= k (past = false) or > k (past = true)
__host__ __device__ __forceinline__ int cloud_bound(const long long* keys, int n, long long k, bool past) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const long long v = keys[mid];
    if (v < k || (past && v == k)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Row (dy, dz) of the neighbourhood of the cell `key`: the occupied cells (iy + dy, iz + dz, ix - 1 .. ix + 1), clipped to the
// lattice, as positions [*a, *b) of the ascending unique keys.  A row outside the lattice and an empty row give a = b.
__host__ __device__ __forceinline__ void cloud_row_range(const long long* ukeys, int nc, long long key, int dy, int dz, int* a, int* b) {
  const long long ix = key & CKEY_MASK, jy = ((key >> CKEY_BITS) & CKEY_MASK) + dy, jz = (key >> (2 * CKEY_BITS)) + dz;
  *a = *b = 0;
  if (key < 0 || jy < 0 || jy > CKEY_MASK || jz < 0 || jz > CKEY_MASK) return;
  const long long x0 = ix > 0 ? ix - 1 : 0, x1 = ix < CKEY_MASK ? ix + 1 : CKEY_MASK;
  const long long base = (jz << (2 * CKEY_BITS)) | (jy << CKEY_BITS);
  *a = cloud_bound(ukeys, nc, base | x0, false);
  *b = cloud_bound(ukeys, nc, base | x1, true);         // not (base | x1) + 1: the lattice's last key is the largest int64
  if (*b < *a) *b = *a;
}

// (d2, idx) against the best so far: the nearer wins, and among equal d2 the lower index.  A lexicographic minimum, so the order
// in which candidates or partial results meet does not matter.  best starts at +inf.  Selects, not branches: the sweep stays
// straight-line and its LDS reads run ahead of their use.
__host__ __device__ __forceinline__ void cloud_keep(float d2, int idx, float& best, int& best_idx) {
  const bool take = (d2 < best) | ((d2 == best) & (idx < best_idx));
  best = take ? d2 : best;
  best_idx = take ? idx : best_idx;
}

// d2 of one (query, candidate) pair in fp32, both relative to the centre of the query's cell: every operation rounded.
__host__ __device__ __forceinline__ float cloud_pair_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (dx * dx + dy * dy) + dz * dz;
}

// One (query, candidate) pair against the best so far.
__host__ __device__ __forceinline__ void cloud_pair_update(float qx, float qy, float qz, float px, float py, float pz, int idx, float& best,
                                                           int& best_idx) {
  cloud_keep(cloud_pair_d2(qx, qy, qz, px, py, pz), idx, best, best_idx);
}

// the truncation: d2 stays iff d2 <= fp32(D D)
__host__ __device__ __forceinline__ void cloud_truncate(float limit, float& best, int& best_idx) {
  if (!(best <= limit)) best = INFINITY, best_idx = -1;
}

struct CloudEntry {      // one candidate in the LDS: 16 bytes, read as one ds_read_b128 at an address a slice's lanes share
  float x, y, z;
  int idx;
};

static inline CloudLattice cloud_lattice(const double* origin, double cell) {
  CloudLattice L;
  for (int i = 0; i < 3; ++i) L.o[i] = origin[i];
  L.c = cell;
  return L;
}


// key of step 1 of "Mesh simplification" (k_simplify_keys' arithmetic), -1 for a point that is not finite or outside the lattice
static inline long long cloud_key_host(const CloudLattice& L, const double* p, int* err) {
  long long key = 0;
  *err = 0;
  for (int ax = 0; ax < 3; ++ax) {
    const double x = p[ax];
    const double t = (x - L.o[ax]) / L.c;
    if (!(fabs(x) <= 1.7976931348623157e308)) *err = *err ? *err : 1;
    else if (!(t >= 0.0 && t < (double)(1 << CKEY_BITS))) *err = *err ? *err : 2;
    else key |= (long long)floor(t) << (ax * CKEY_BITS);
  }
  return *err ? -1 : key;
}

}  // namespace adamvs
