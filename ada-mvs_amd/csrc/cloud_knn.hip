// Cloud neighbourhoods: the k nearest neighbours of every point of a cloud within a radius, and a normal per point from them, so
// that a fused cloud can be filtered before anything reads it (include/adamvs_hip.h "Cloud neighbourhoods" states every
// operation).  The caller (ada-mvs_amd/cloud_filter.py) keys the cloud on the lattice of side c = R, sorts it stably, numbers the
// occupied cells and cuts the sorted points into the work items of "Cloud distance" (one cell, at most 256 queries); the cloud
// is both the targets and the queries (ada-mvs_amd/cloud_lattice.py).  cloud_lattice.h holds the walk that cloud_dist.hip
// shares: rows, candidate tiles, slices, pair arithmetic, and the host's keyed cloud and candidate visitor; here:
//
//   k_knn_search   one workgroup per work item walks the item's candidates (CloudWalk, the tile as wide as the workgroup), the
//                  lanes in S slices of P queries.  Each lane keeps a partial list of its k best in LDS
//                  columns (slot-major: the lanes of a wave hit different banks) and the list's worst (d2, index) in registers, so
//                  that once the list is full most candidates cost one compare.  The S lists of a query meet in a tree under the
//                  same total order; the result leaves ranked by counting.  One instantiation per class of k: k <= 8 and k <= 16
//                  with 256 lanes (16 and 32 KiB of lists), k <= 32 with 128 lanes (32 KiB; an item of more than 128 queries takes
//                  two passes over its candidates, every (query, candidate) pair still evaluated once).
//   k_knn_normals  one lane per point: mean and covariance of its neighbourhood in fp64, cyclic Jacobi (jacobi.h), the
//                  eigenvector of the least eigenvalue, oriented upward
//
// No atomics and no inter-workgroup waits: every lane writes its own elements only, and a point's result is a function of the
// cloud as a set, so the output is bit-identical from run to run and equivariant under any permutation of the cloud.
#include <math.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "block_prims.h"
#include "cloud_lattice.h"
#include "common.h"
#include "jacobi.h"
#include "kernels.h"

// The header states the arithmetic as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

static_assert(KNN_MAX_K == 32, "the classes of k below are 8, 16 and 32");
constexpr int KNN_BATCH = 4;            // candidates whose LDS reads are in flight together in the sweep

// (d2, idx) strictly before (wd, wi) in the lexicographic order of step 4 of "Cloud distance"
__host__ __device__ __forceinline__ bool knn_before(float d2, int idx, float wd, int wi) {
  return (d2 < wd) | ((d2 == wd) & (idx < wi));
}

// a candidate of the query `self` enters a list of m of k entries whose worst is (wd, wi)
__host__ __device__ __forceinline__ bool knn_accept(float d2, int idx, float limit, int self, int m, int k, float wd, int wi) {
  return (d2 <= limit) & (idx != self) & ((m < k) | knn_before(d2, idx, wd, wi));
}

// One lane's list: column `lane` of the slot-major LDS arrays, m of k entries in no order; (wd, wi) at slot ws is the worst once
// m = k.  A new entry is appended while m < k and replaces the worst afterwards; the worst is found again by one scan.
template <int KC, int LANES>
struct KnnList {
  float (*d)[LANES];
  int (*i)[LANES];
  int lane, k, m, ws, wi;
  float wd;

  __device__ __forceinline__ void reset() { m = 0, ws = 0, wi = 0x7fffffff, wd = INFINITY; }

  __device__ __forceinline__ void insert(float d2, int idx) {
    const int s = m < k ? m : ws;
    d[s][lane] = d2;
    i[s][lane] = idx;
    m += m < k ? 1 : 0;
    if (m == k) {                       // selects, not branches, as cloud_keep: the reads of the scan run ahead of their use
      wd = d[0][lane], wi = i[0][lane], ws = 0;
#pragma unroll 4
      for (int j = 1; j < k; ++j) {
        const float dj = d[j][lane];
        const int ij = i[j][lane];
        const bool worse = knn_before(wd, wi, dj, ij);
        wd = worse ? dj : wd, wi = worse ? ij : wi, ws = worse ? j : ws;
      }
    }
  }
};

template <int KC, int LANES>
__global__ __launch_bounds__(LANES) void k_knn_search(const CloudLattice L, float limit, int k, const long long* __restrict__ ukeys,
                                                      const long long* __restrict__ tstart, int nc, const double* __restrict__ sorted,
                                                      const int* __restrict__ pindex, long n, const long long* __restrict__ item_key,
                                                      const long long* __restrict__ item_first, const int* __restrict__ item_count,
                                                      long long row_base, long rows, float* __restrict__ d2, int* __restrict__ index,
                                                      int* __restrict__ count, unsigned long long* __restrict__ pairs) {
  __shared__ __attribute__((aligned(16))) CloudWalk<LANES> w;
  __shared__ float list_d[KC][LANES];
  __shared__ int list_i[KC][LANES];
  __shared__ int fill[LANES];
  const int lane = threadIdx.x;
  const long item = blockIdx.x;
  const long long key = item_key[item];
  const long long first = item_first[item];
  int cnt_item = item_count[item];
  cnt_item = cnt_item < 0 ? 0 : (cnt_item > CLOUD_TILE ? CLOUD_TILE : cnt_item);
  k = k < 1 ? 1 : (k > KC ? KC : k);
  double ctr[3];
  cloud_centre(L, key < 0 ? 0 : key, ctr);
  cloud_walk_rows(w, ukeys, tstart, nc, key, n);
  const int total = cloud_walk_total(w);
  KnnList<KC, LANES> list;
  list.d = list_d, list.i = list_i, list.lane = lane, list.k = k;
  // an item of more than LANES queries takes its queries LANES at a time (uniform: every lane walks the same passes)
  for (int q0 = 0; q0 < cnt_item; q0 += LANES) {
    const int cnt = cnt_item - q0 < LANES ? cnt_item - q0 : LANES;
    const CloudSlices sl = cloud_slices(cnt, LANES, lane);
    const int P = sl.P, S = sl.S, ql = sl.ql, slice = sl.slice;
    const long long slot = first + q0 + ql;
    const bool live = ql < cnt && slot >= 0 && slot < n;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int self = -1;
    if (live) {
      qx = (float)(sorted[3 * slot] - ctr[0]);
      qy = (float)(sorted[3 * slot + 1] - ctr[1]);
      qz = (float)(sorted[3 * slot + 2] - ctr[2]);
      self = pindex[slot];
    }
    list.reset();
    for (long long base = 0; base < total; base += LANES) {
      cloud_walk_fill(w, base, sorted, pindex, n, ctr);
      __syncthreads();
      const int nn = total - base < LANES ? (int)(total - base) : LANES;
      // four candidates at a time: their reads and distances come first, straight-line, the rare entries into the list after them,
      // in the candidates' order (a candidate past the tile's end has d2 = +inf and never enters)
      for (int c = slice; c < nn; c += KNN_BATCH * S) {
        float dd[KNN_BATCH];
        int id[KNN_BATCH];
#pragma unroll
        for (int u = 0; u < KNN_BATCH; ++u) {
          const int cu = c + u * S;
          const CloudEntry p = w.tile[cu < nn ? cu : c];
          dd[u] = cu < nn ? cloud_pair_d2(qx, qy, qz, p.x, p.y, p.z) : INFINITY;
          id[u] = p.idx;
        }
#pragma unroll
        for (int u = 0; u < KNN_BATCH; ++u)
          if (live && knn_accept(dd[u], id[u], limit, self, list.m, k, list.wd, list.wi)) list.insert(dd[u], id[u]);
      }
      __syncthreads();
    }
    // the S partial lists of a query meet in a tree: the lower half takes the upper half's entries under the same rule (S is uniform)
    for (int h = S >> 1; h >= 1; h >>= 1) {
      fill[lane] = list.m;
      __syncthreads();
      if (slice < h) {
        const int other = lane + h * P;
        const int om = fill[other];
        for (int j = 0; j < om; ++j) {
          const float dj = list_d[j][other];
          const int ij = list_i[j][other];
          if ((list.m < k) | knn_before(dj, ij, list.wd, list.wi)) list.insert(dj, ij);
        }
      }
      __syncthreads();
    }
    // the query's list is column ql now; its S lanes share the entries, rank each by counting and write it at its rank
    fill[lane] = list.m;
    __syncthreads();
    const long long row = slot - row_base;
    if (live && row >= 0 && row < rows) {
      const int mq = fill[ql];
      for (int j = slice; j < mq; j += S) {
        const float dj = list_d[j][ql];
        const int ij = list_i[j][ql];
        int rank = 0;
        for (int t = 0; t < mq; ++t) rank += knn_before(list_d[t][ql], list_i[t][ql], dj, ij) ? 1 : 0;
        d2[row * k + rank] = dj;
        index[row * k + rank] = ij;
      }
      for (int j = mq + slice; j < k; j += S) d2[row * k + j] = INFINITY, index[row * k + j] = -1;
      if (slice == 0) count[row] = mq;
    }
    __syncthreads();
  }
  if (lane == 0) pairs[item] = (unsigned long long)total * (unsigned long long)cnt_item;
}

// ---- normals --------------------------------------------------------------------------------------------------------------------
// Step N of the header for one point p with the neighbours nbr[0 .. cnt) (numbers into points [n][3]) -> the unit normal (fp64),
// the surface variation and the flag.
__host__ __device__ __forceinline__ void knn_normal_point(const double* points, long n, const double* p, const int* nbr, int cnt,
                                                          double* normal, float* curvature, uint8_t* flag) {
  const double m = (double)(cnt + 1);                       // the point itself is a member, as the difference 0
  double s0 = 0., s1 = 0., s2 = 0.;
  for (int j = 0; j < cnt; ++j) {
    const long v = nbr[j];
    if (v < 0 || v >= n) continue;
    s0 += points[3 * v] - p[0], s1 += points[3 * v + 1] - p[1], s2 += points[3 * v + 2] - p[2];
  }
  const double m0 = s0 / m, m1 = s1 / m, m2 = s2 / m;
  double a00 = 0., a01 = 0., a02 = 0., a11 = 0., a12 = 0., a22 = 0.;
  for (int j = 0; j <= cnt; ++j) {
    double e0 = 0.0 - m0, e1 = 0.0 - m1, e2 = 0.0 - m2;     // j = cnt: the point itself
    if (j < cnt) {
      const long v = nbr[j];
      if (v < 0 || v >= n) continue;
      e0 = (points[3 * v] - p[0]) - m0, e1 = (points[3 * v + 1] - p[1]) - m1, e2 = (points[3 * v + 2] - p[2]) - m2;
    }
    a00 += e0 * e0, a01 += e0 * e1, a02 += e0 * e2, a11 += e1 * e1, a12 += e1 * e2, a22 += e2 * e2;
  }
  a00 = a00 / m, a01 = a01 / m, a02 = a02 / m, a11 = a11 / m, a12 = a12 / m, a22 = a22 / m;
  double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
#pragma unroll
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  // the least eigenvalue (the lowest position among equals), the largest (the highest position among equals), the third between
  const int i0 = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);
  const int i2 = (a22 >= a00 && a22 >= a11) ? 2 : (a11 >= a00 ? 1 : 0);
  const int i1 = 3 - i0 - i2;
  const double l0 = i0 == 0 ? a00 : (i0 == 1 ? a11 : a22);
  const double l1 = i1 == 0 ? a00 : (i1 == 1 ? a11 : a22);
  const double l2 = i2 == 0 ? a00 : (i2 == 1 ? a11 : a22);
  double n0 = i0 == 0 ? v00 : (i0 == 1 ? v01 : v02);
  double n1 = i0 == 0 ? v10 : (i0 == 1 ? v11 : v12);
  double n2 = i0 == 0 ? v20 : (i0 == 1 ? v21 : v22);
  const int f = cnt < 3 ? ADAMVS_KNN_TOO_FEW : (l1 > ADAMVS_KNN_RANK_EPS * l2 ? ADAMVS_KNN_VALID : ADAMVS_KNN_COLLINEAR);
  *flag = (uint8_t)f;
  normal[0] = normal[1] = normal[2] = 0.0;
  *curvature = 0.f;
  if (f != ADAMVS_KNN_VALID) return;
  const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
  n0 = n0 / len, n1 = n1 / len, n2 = n2 / len;
  const double lead = n2 != 0.0 ? n2 : (n1 != 0.0 ? n1 : n0);          // upward: the first non-zero of (nz, ny, nx) is positive
  if (lead < 0.0) n0 = -n0, n1 = -n1, n2 = -n2;
  normal[0] = n0, normal[1] = n1, normal[2] = n2;
  const double c0 = l0 > 0.0 ? l0 : 0.0;
  *curvature = (float)(c0 / ((c0 + l1) + l2));
}

__global__ __launch_bounds__(256) void k_knn_normals(const double* __restrict__ points, long n, const int* __restrict__ index,
                                                     const int* __restrict__ count, int k, long rows, const int* __restrict__ row_point,
                                                     double* __restrict__ normal, float* __restrict__ curvature, uint8_t* __restrict__ flag) {
  const long r = (long)blockIdx.x * CLOUD_TILE + threadIdx.x;
  if (r >= rows) return;
  const long v = row_point ? (long)row_point[r] : r;
  int cnt = count[r];
  cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
  double nrm[3] = {0., 0., 0.};
  float curv = 0.f;
  uint8_t f = ADAMVS_KNN_TOO_FEW;
  if (v >= 0 && v < n) knn_normal_point(points, n, points + 3 * v, index + r * (long)k, cnt, nrm, &curv, &f);
  normal[3 * r] = nrm[0], normal[3 * r + 1] = nrm[1], normal[3 * r + 2] = nrm[2];
  curvature[r] = curv;
  flag[r] = f;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------
int launch_knn_search(const double* origin, double R, int k, const long long* ukeys, const long long* tstart, int nc, const double* sorted,
                      const int* pindex, long n, const long long* item_key, const long long* item_first, const int* item_count, long ni,
                      long long row_base, long rows, float* d2, int* index, int* count, unsigned long long* pairs, hipStream_t st) {
  const CloudLattice L = cloud_lattice(origin, R);
  const float limit = (float)(R * R);
#define ADAMVS_KNN_LAUNCH(KC, LANES)                                                                                                  \
  hipLaunchKernelGGL((k_knn_search<KC, LANES>), dim3((unsigned)ni), dim3(LANES), 0, st, L, limit, k, ukeys, tstart, nc, sorted, pindex, n, \
                     item_key, item_first, item_count, row_base, rows, d2, index, count, pairs)
  if (k <= 8) ADAMVS_KNN_LAUNCH(8, 256);
  else if (k <= 16) ADAMVS_KNN_LAUNCH(16, 256);
  else ADAMVS_KNN_LAUNCH(32, 128);
#undef ADAMVS_KNN_LAUNCH
  ADAMVS_CHECK_LAUNCH("knn_search");
  return 0;
}

int launch_knn_normals(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                       double* normal, float* curvature, uint8_t* flag, hipStream_t st) {
  hipLaunchKernelGGL(k_knn_normals, dim3(tiles256(rows)), dim3(CLOUD_TILE), 0, st, points, n, index, count, k,
                     rows, row_point, normal, curvature, flag);
  ADAMVS_CHECK_LAUNCH("knn_normals");
  return 0;
}

// ---- the same on the host, for checks of the rule without a device ----------------------------------------------------------------
int knn_search_host(const double* origin, double R, int k, const double* points, long n, float* d2, int* index, int* count,
                    unsigned long long* pairs) {
  const CloudLattice L = cloud_lattice(origin, R);
  const float limit = (float)(R * R);
  CloudCells cells;
  if (int rc = cloud_cells_host(L, points, n, "knn_search_host: point", cells)) return rc;
  unsigned long long evaluated = 0;
  std::vector<std::pair<float, int>> found;
  for (long q = 0; q < n; ++q) {
    found.clear();
    evaluated += cloud_visit_host(L, cells, points, cells.key[q], points + 3 * q, [&](float qx, float qy, float qz, float px, float py, float pz, int idx) {
      const float dd = cloud_pair_d2(qx, qy, qz, px, py, pz);
      if (knn_accept(dd, idx, limit, (int)q, 0, 1, INFINITY, 0x7fffffff)) found.emplace_back(dd, idx);
    });
    std::sort(found.begin(), found.end(), [](const std::pair<float, int>& a, const std::pair<float, int>& b) {
      return knn_before(a.first, a.second, b.first, b.second);
    });
    const int m = (int)std::min<size_t>(found.size(), (size_t)k);
    for (int j = 0; j < k; ++j) {
      d2[q * k + j] = j < m ? found[j].first : INFINITY;
      index[q * k + j] = j < m ? found[j].second : -1;
    }
    count[q] = m;
  }
  if (pairs) *pairs = evaluated;
  return 0;
}

int knn_normals_host(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point, double* normal,
                     float* curvature, unsigned char* flag) {
  for (long r = 0; r < rows; ++r) {
    const long v = row_point ? (long)row_point[r] : r;
    int cnt = count[r];
    cnt = cnt < 0 ? 0 : (cnt > k ? k : cnt);
    double nrm[3] = {0., 0., 0.};
    float curv = 0.f;
    uint8_t f = ADAMVS_KNN_TOO_FEW;
    if (v >= 0 && v < n) knn_normal_point(points, n, points + 3 * v, index + r * (long)k, cnt, nrm, &curv, &f);
    normal[3 * r] = nrm[0], normal[3 * r + 1] = nrm[1], normal[3 * r + 2] = nrm[2];
    curvature[r] = curv;
    flag[r] = f;
  }
  return 0;
}

}  // namespace adamvs
