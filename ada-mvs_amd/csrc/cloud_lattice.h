// The lattice of cubic cells under the 63-bit keys of adamvs_simplify_keys, and the one walk of it that every search runs:
// the key of a point (mesh_simplify.hip's k_simplify_keys is this function per vertex), cell centres, the nine-row search in
// the sorted unique keys, the pair arithmetic in fp32 and the lexicographic keep rule (include/adamvs_hip.h "Cloud distance",
// steps 1 to 4).  On the device the walk is CloudWalk: the rows of a work item, the candidate tiles in the LDS and the split of
// the lanes into slices (cloud_dist.hip sweeps the tiles for the nearest target, cloud_knn.hip for the k nearest).  On the
// host it is CloudCells (the keyed, sorted cloud) and cloud_visit_host (the candidates of one query).  Inline and
// __host__ __device__ wherever both sides compute: the kernels and their host twins run the same functions.
#pragma once
#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

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

static inline CloudLattice cloud_lattice(const double* origin, double cell) {
  CloudLattice L;
  for (int i = 0; i < 3; ++i) L.o[i] = origin[i];
  L.c = cell;
  return L;
}

// Step 1 of "Mesh simplification": the key of the point p, or -1 with *err = 1 (a coordinate is NaN or infinite) or 2 (outside
// the lattice); the first axis at fault names the error.
__host__ __device__ __forceinline__ long long cloud_key(const CloudLattice& L, const double* p, int* err) {
  long long key = 0;
  int e = 0;
  for (int ax = 0; ax < 3; ++ax) {
    const double x = p[ax];
    const double t = (x - L.o[ax]) / L.c;
    if (!(fabs(x) <= 1.7976931348623157e308)) e = e ? e : 1;
    else if (!(t >= 0.0 && t < (double)(1 << CKEY_BITS))) e = e ? e : 2;
    else key |= (long long)floor(t) << (ax * CKEY_BITS);
  }
  *err = e;
  return e ? -1 : key;
}

// key (>= 0) -> the centre of its cell
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

// ---- the walk on the device: one workgroup of LANES lanes per work item (one cell, at most CLOUD_TILE queries) -------------------
struct CloudEntry {      // one candidate in the LDS: 16 bytes, read as one ds_read_b128 at an address a slice's lanes share
  float x, y, z;
  int idx;
};

template <int LANES>
struct CloudWalk {       // a __shared__ variable of the kernel
  __attribute__((aligned(16))) CloudEntry tile[LANES];
  long long row_start[9];
  int row_off[10], row_len[9];
};

// Nine lanes find the nine (dy, dz) rows of the 27 cells around `key` (two binary searches each: with x in the low key bits the
// three x-neighbours are one run of the n sorted points), clamped to [0, n]; after a barrier lane 0 packs the runs end to end
// (row_off, saturating).  Every lane of the workgroup calls this, then cloud_walk_total.
template <int LANES>
__device__ __forceinline__ void cloud_walk_rows(CloudWalk<LANES>& w, const long long* __restrict__ ukeys, const long long* __restrict__ tstart,
                                                int nc, long long key, long n) {
  const int lane = threadIdx.x;
  if (lane < 9) {
    int a, b;
    cloud_row_range(ukeys, nc, key, lane % 3 - 1, lane / 3 - 1, &a, &b);
    long long s = tstart[a], e = tstart[b];
    s = s < 0 ? 0 : (s > n ? n : s);
    e = e < s ? s : (e > n ? n : e);
    w.row_start[lane] = s;
    w.row_len[lane] = (int)(e - s);
  }
  __syncthreads();
  if (lane == 0) {
    int acc = 0;
    for (int r = 0; r < 9; ++r) {
      w.row_off[r] = acc;
      const int len = w.row_len[r];
      acc = len > 0x7fffffff - acc ? 0x7fffffff : acc + len;
    }
    w.row_off[9] = acc;
  }
}

// The barrier that publishes cloud_walk_rows' packing -> the item's candidates.  Apart from the rows so that a kernel can set up
// its queries while lane 0 packs.
template <int LANES>
__device__ __forceinline__ int cloud_walk_total(const CloudWalk<LANES>& w) {
  __syncthreads();
  return w.row_off[9];
}

// Candidate base + lane of the packed runs into the tile: centre-relative fp32 and its number in the caller's order; past the
// last candidate a padding entry.  The caller's barrier follows.
template <int LANES>
__device__ __forceinline__ void cloud_walk_fill(CloudWalk<LANES>& w, long long base, const double* __restrict__ points,
                                                const int* __restrict__ pindex, long n, const double* ctr) {
  const int lane = threadIdx.x;
  const long long g = base + lane;
  long long src = -1;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int lo = w.row_off[r], hi = w.row_off[r + 1];
    if (g >= lo && g < hi) src = w.row_start[r] + (g - lo);
  }
  CloudEntry e = {0.f, 0.f, 0.f, 0x7fffffff};
  if (src >= 0 && src < n) {
    e.x = (float)(points[3 * src] - ctr[0]);
    e.y = (float)(points[3 * src + 1] - ctr[1]);
    e.z = (float)(points[3 * src + 2] - ctr[2]);
    e.idx = pindex[src];
  }
  w.tile[lane] = e;
}

// `count` queries take P lanes, P the smallest power of two >= count, and the LANES lanes split into S = LANES / P SLICES: lane l
// serves query ql = l mod P and sweeps candidates slice, slice + S, .. of every tile.  A cell of a fused cloud holds ten queries,
// not 256: with one lane per query the other lanes would idle through the sweep.  P and S are uniform over the workgroup.
struct CloudSlices {
  int P, S, ql, slice;
};

__device__ __forceinline__ CloudSlices cloud_slices(int count, int lanes, int lane) {
  int P = 1;
  while (P < count) P <<= 1;
  return {P, lanes / P, lane & (P - 1), lane / P};
}

// ---- the walk on the host --------------------------------------------------------------------------------------------------------
struct CloudCells {      // a cloud keyed and sorted stably: point order[s] is at position s, cell ukeys[j] is positions tstart[j] .. tstart[j + 1]
  std::vector<long long> key, ukeys, tstart;
  std::vector<long> order;
};

// Fills `cells` from points [n][3]; a point that is not finite or outside the lattice is refused as "<what> <i> is ..." (what:
// the caller's name and noun, "cloud_nearest_host: target").
static inline int cloud_cells_host(const CloudLattice& L, const double* points, long n, const char* what, CloudCells& cells) {
  cells.key.resize(n);
  for (long i = 0; i < n; ++i) {
    int err;
    cells.key[i] = cloud_key(L, points + 3 * i, &err);
    if (err) return set_error(-1, "%s %ld is %s", what, i, err == 1 ? "not finite" : "outside the lattice of 2^21 cells per axis");
  }
  const std::vector<long long>& key = cells.key;
  cells.order.resize(n);
  std::iota(cells.order.begin(), cells.order.end(), 0L);
  std::stable_sort(cells.order.begin(), cells.order.end(), [&](long a, long b) { return key[a] < key[b]; });
  for (long i = 0; i < n; ++i)
    if (i == 0 || key[cells.order[i]] != key[cells.order[i - 1]]) cells.ukeys.push_back(key[cells.order[i]]), cells.tstart.push_back(i);
  cells.tstart.push_back(n);
  return 0;
}

// The candidates of the query q (in the cell `key` >= 0) among `points`, the cloud of `cells`: the nine rows in order, every
// candidate as visit(qx, qy, qz, px, py, pz, its number), centre-relative fp32 -> the pairs evaluated.
template <class Visit>
static inline unsigned long long cloud_visit_host(const CloudLattice& L, const CloudCells& cells, const double* points, long long key,
                                                  const double* q, Visit&& visit) {
  double ctr[3];
  cloud_centre(L, key, ctr);
  const float qx = (float)(q[0] - ctr[0]), qy = (float)(q[1] - ctr[1]), qz = (float)(q[2] - ctr[2]);
  unsigned long long evaluated = 0;
  for (int r = 0; r < 9; ++r) {
    int a, b;
    cloud_row_range(cells.ukeys.data(), (int)cells.ukeys.size(), key, r % 3 - 1, r / 3 - 1, &a, &b);
    for (long long s = cells.tstart[a]; s < cells.tstart[b]; ++s, ++evaluated) {
      const double* p = points + 3 * cells.order[s];
      visit(qx, qy, qz, (float)(p[0] - ctr[0]), (float)(p[1] - ctr[1]), (float)(p[2] - ctr[2]), (int)cells.order[s]);
    }
  }
  return evaluated;
}

}  // namespace adamvs
