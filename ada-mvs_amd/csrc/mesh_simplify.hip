// Mesh simplification by vertex clustering on a lattice with one quadric per cell (Lindstrom's out-of-core simplification with
// Garland-Heckbert quadrics; the step after mesh_whu.py; include/adamvs_hip.h "Mesh simplification" states every operation).
// The caller (ada-mvs_amd/simplify.py) numbers the cells (unique of the keys) and brings the (cell, face) and (cell, vertex)
// entries into runs with stable sorts; the arithmetic is here:
//
//   k_simplify_keys        one lane per vertex: the 63-bit cell key and an error code
//   k_simplify_corners     one lane per face: the cells of its corners, its (cell, face) entries, its survive bit
//   k_simplify_accumulate  one wave per cell: the quadric over its run of faces and the member sums over its run of vertices;
//                          lane l takes entries l, l + 64, .. in order, the 64 partials meet in a fixed butterfly
//                          (block_prims.h wave_sum)
//   k_simplify_solve       one lane per cell: cyclic Jacobi on the 3x3 (registers only), rank rule, pseudo-inverse step,
//                          in-cell test, colour
//   k_simplify_triples     one lane per surviving face: its three cells in ascending order (the caller sorts by them)
//   k_simplify_first       one lane per entry of that sorted order: the first face of each set of three cells is kept
//   k_simplify_mark        one lane per face: a kept face flags its three cells as used (plain stores of 1)
//   k_simplify_count       flags per workgroup (k_fusion_scan turns the counts into offsets)
//   k_simplify_emit_*      used cells and kept faces at  block offset + rank in the block  (block_prims.h block_rank)
//
// No atomics and no inter-workgroup waits: the order of every sum is a function of the sorted input only, the launches are
// the synchronisation, and the output is bit-identical from run to run.
#include <math.h>

#include "block_prims.h"
#include "cloud_lattice.h"
#include "common.h"
#include "jacobi.h"
#include "kernels.h"

// The header states every position as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

__global__ __launch_bounds__(256) void k_simplify_keys(const CloudLattice L, const double* __restrict__ xyz, long nv, long long* __restrict__ keys,
                                                       uint8_t* __restrict__ bad) {
  const long v = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (v >= nv) return;
  int err;
  keys[v] = cloud_key(L, xyz + 3 * v, &err);
  bad[v] = (uint8_t)err;
}

__global__ __launch_bounds__(256) void k_simplify_corners(const unsigned* __restrict__ faces, long nf, const int* __restrict__ vcell,
                                                          long nv, int nc, int* __restrict__ fcell, int* __restrict__ entry_cell,
                                                          uint8_t* __restrict__ survive) {
  const long f = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (f >= nf) return;
  const unsigned v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  const bool ok = (long)v0 < nv && (long)v1 < nv && (long)v2 < nv;
  const int c0 = ok ? vcell[v0] : nc, c1 = ok ? vcell[v1] : nc, c2 = ok ? vcell[v2] : nc;
  fcell[3 * f] = c0, fcell[3 * f + 1] = c1, fcell[3 * f + 2] = c2;
  entry_cell[3 * f] = c0;
  entry_cell[3 * f + 1] = c1 == c0 ? nc : c1;
  entry_cell[3 * f + 2] = (c2 == c0 || c2 == c1) ? nc : c2;
  survive[f] = (uint8_t)(ok && c0 != c1 && c1 != c2 && c0 != c2);
}

__global__ __launch_bounds__(256) void k_simplify_accumulate(const CloudLattice L, const long long* __restrict__ keys, int nc,
                                                             const double* __restrict__ xyz, const uint8_t* __restrict__ rgb, long nv,
                                                             const unsigned* __restrict__ faces, long nf,
                                                             const long long* __restrict__ entry, const long long* __restrict__ fstart,
                                                             const long long* __restrict__ vorder, const long long* __restrict__ vstart,
                                                             double* __restrict__ quadric, double* __restrict__ member,
                                                             unsigned long long* __restrict__ colour) {
  const int lane = threadIdx.x & 63;
  const int j = __builtin_amdgcn_readfirstlane(blockIdx.x * (SIMPLIFY_TILE / 64) + (threadIdx.x >> 6));     // the wave's cell
  if (j >= nc) return;
  double ctr[3];
  cloud_centre(L, keys[j], ctr);
  // the quadric: faces e0 .. e1 of the sorted (cell, face) entries
  const long long e0 = fstart[j], e1 = fstart[j + 1];
  double q[10] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
  for (long long i = e0 + lane; i < e1; i += 64) {
    const long long f = entry[i] / 3;
    if (f < 0 || f >= nf) continue;
    double p[3][3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      const unsigned v = faces[3 * f + k];
      ok = ok && (long)v < nv;
      const long vv = (long)v < nv ? (long)v : 0;
      for (int ax = 0; ax < 3; ++ax) p[k][ax] = xyz[3 * vv + ax] - ctr[ax];
    }
    if (!ok) continue;
    const double u[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
    const double w[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
    const double n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const double d = -(n[0] * p[0][0] + n[1] * p[0][1] + n[2] * p[0][2]);
    q[0] += n[0] * n[0], q[1] += n[0] * n[1], q[2] += n[0] * n[2];
    q[3] += n[1] * n[1], q[4] += n[1] * n[2], q[5] += n[2] * n[2];
    q[6] += d * n[0], q[7] += d * n[1], q[8] += d * n[2];
    q[9] += d * d;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = wave_sum(q[k]);
  // the members: vertices m0 .. m1 of the vertices sorted by cell
  const long long m0 = vstart[j], m1 = vstart[j + 1];
  double s[3] = {0., 0., 0.};
  unsigned long long c[3] = {0, 0, 0};
  for (long long i = m0 + lane; i < m1; i += 64) {
    const long long v = vorder[i];
    if (v < 0 || v >= nv) continue;
    for (int ax = 0; ax < 3; ++ax) {
      s[ax] += xyz[3 * v + ax] - ctr[ax];
      c[ax] += rgb[3 * v + ax];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) s[k] = wave_sum(s[k]), c[k] = wave_sum(c[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) quadric[10 * (size_t)j + k] = q[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) member[3 * (size_t)j + k] = s[k], colour[3 * (size_t)j + k] = c[k];
  }
}

// Step 4 of the header for one cell: q = {A00 A01 A02 A11 A12 A22, b, sum d^2}, m the members' mean; -> p (relative to the
// centre), the rank, whether p fell back to m, and the quadric's value at p.
__host__ __device__ __forceinline__ void simplify_solve_cell(const double* q, const double* m, double half, double rank_eps, double* p,
                                                             int* rank_out, int* fallback_out, double* error_out) {
  double a00 = q[0], a01 = q[1], a02 = q[2], a11 = q[3], a12 = q[4], a22 = q[5];
  double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
#pragma unroll
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
    jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
    jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
  }
  const double lmax = fmax(a00, fmax(a11, a22));
  const double g0 = -(q[6] + (q[0] * m[0] + q[1] * m[1] + q[2] * m[2]));
  const double g1 = -(q[7] + (q[1] * m[0] + q[3] * m[1] + q[4] * m[2]));
  const double g2 = -(q[8] + (q[2] * m[0] + q[4] * m[1] + q[5] * m[2]));
  const bool k0 = a00 > rank_eps * lmax, k1 = a11 > rank_eps * lmax, k2 = a22 > rank_eps * lmax;
  const double w0 = k0 ? (v00 * g0 + v10 * g1 + v20 * g2) / a00 : 0.0;
  const double w1 = k1 ? (v01 * g0 + v11 * g1 + v21 * g2) / a11 : 0.0;
  const double w2 = k2 ? (v02 * g0 + v12 * g1 + v22 * g2) / a22 : 0.0;
  p[0] = m[0] + (v00 * w0 + v01 * w1 + v02 * w2);
  p[1] = m[1] + (v10 * w0 + v11 * w1 + v12 * w2);
  p[2] = m[2] + (v20 * w0 + v21 * w1 + v22 * w2);
  const int rank = (int)k0 + (int)k1 + (int)k2;
  const bool inside = fabs(p[0]) <= half && fabs(p[1]) <= half && fabs(p[2]) <= half;      // false for NaN and infinity
  const bool fb = rank == 0 || !inside;
  if (fb) p[0] = m[0], p[1] = m[1], p[2] = m[2];
  const double ap0 = q[0] * p[0] + q[1] * p[1] + q[2] * p[2], ap1 = q[1] * p[0] + q[3] * p[1] + q[4] * p[2],
               ap2 = q[2] * p[0] + q[4] * p[1] + q[5] * p[2];
  *error_out = (p[0] * ap0 + p[1] * ap1 + p[2] * ap2) + 2.0 * (q[6] * p[0] + q[7] * p[1] + q[8] * p[2]) + q[9];
  *rank_out = rank;
  *fallback_out = fb ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_simplify_solve(const CloudLattice L, double rank_eps, const long long* __restrict__ keys, int nc,
                                                        const double* __restrict__ quadric, const double* __restrict__ member,
                                                        const unsigned long long* __restrict__ colour,
                                                        const long long* __restrict__ vstart, double* __restrict__ pos,
                                                        uint8_t* __restrict__ col, uint8_t* __restrict__ rank, uint8_t* __restrict__ fallback,
                                                        double* __restrict__ error) {
  const int j = blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (j >= nc) return;
  double q[10], m[3], p[3], ctr[3];
#pragma unroll
  for (int k = 0; k < 10; ++k) q[k] = quadric[10 * (size_t)j + k];
  const unsigned long long n = (unsigned long long)(vstart[j + 1] - vstart[j]);       // >= 1: a cell has a member
  const unsigned long long nn = n ? n : 1;
#pragma unroll
  for (int k = 0; k < 3; ++k) m[k] = member[3 * (size_t)j + k] / (double)nn;
  int rk, fb;
  double err;
  simplify_solve_cell(q, m, L.c / 2.0, rank_eps, p, &rk, &fb, &err);
  cloud_centre(L, keys[j], ctr);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    pos[3 * (size_t)j + k] = ctr[k] + p[k];
    col[3 * (size_t)j + k] = (uint8_t)((colour[3 * (size_t)j + k] + nn / 2) / nn);
  }
  rank[j] = (uint8_t)rk;
  fallback[j] = (uint8_t)fb;
  error[j] = err;
}

__global__ __launch_bounds__(256) void k_simplify_triples(const int* __restrict__ fcell, long nf, const long long* __restrict__ surv, long ns,
                                                          int* __restrict__ tri) {
  const long i = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (i >= ns) return;
  const long long f = surv[i];
  int a = 0, b = 0, c = 0;
  if (f >= 0 && f < nf) {
    a = fcell[3 * f], b = fcell[3 * f + 1], c = fcell[3 * f + 2];
    int t;
    if (a > b) t = a, a = b, b = t;
    if (b > c) t = b, b = c, c = t;
    if (a > b) t = a, a = b, b = t;
  }
  tri[i] = a, tri[ns + i] = b, tri[2 * ns + i] = c;
}

__global__ __launch_bounds__(256) void k_simplify_first(const int* __restrict__ tri, const long long* __restrict__ surv,
                                                        const long long* __restrict__ order, long ns, long nf, uint8_t* __restrict__ keep) {
  const long i = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (i >= ns) return;
  const long long s = order[i];
  if (s < 0 || s >= ns) return;
  bool first = i == 0;
  if (!first) {
    const long long r = order[i - 1];
    first = r < 0 || r >= ns || tri[r] != tri[s] || tri[ns + r] != tri[ns + s] || tri[2 * ns + r] != tri[2 * ns + s];
  }
  const long long f = surv[s];
  if (f >= 0 && f < nf) keep[f] = (uint8_t)first;
}

__global__ __launch_bounds__(256) void k_simplify_mark(const int* __restrict__ fcell, const uint8_t* __restrict__ keep, long nf, int nc,
                                                       uint8_t* __restrict__ used) {
  const long f = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  if (f >= nf || !keep[f]) return;
  for (int k = 0; k < 3; ++k) {
    const int c = fcell[3 * f + k];
    if (c >= 0 && c < nc) used[c] = 1;
  }
}

__global__ __launch_bounds__(256) void k_simplify_count(const uint8_t* __restrict__ flags, long n, unsigned* __restrict__ block_count) {
  const long i = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  unsigned total;
  block_rank(i < n && flags[i] != 0, &total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_simplify_emit_vertices(const double* __restrict__ pos, const uint8_t* __restrict__ col,
                                                                const uint8_t* __restrict__ used, int nc,
                                                                const unsigned* __restrict__ offsets, double* __restrict__ xyz,
                                                                uint8_t* __restrict__ rgb, unsigned* __restrict__ new_index, long capacity) {
  const long j = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  const bool flag = j < nc && used[j] != 0;
  unsigned total;
  const long q = (long)offsets[blockIdx.x] + block_rank(flag, &total);
  if (!flag || q >= capacity) return;
  new_index[j] = (unsigned)q;
  for (int k = 0; k < 3; ++k) {
    xyz[3 * q + k] = pos[3 * j + k];
    rgb[3 * q + k] = col[3 * j + k];
  }
}

__global__ __launch_bounds__(256) void k_simplify_emit_faces(const int* __restrict__ fcell, const uint8_t* __restrict__ keep, long nf, int nc,
                                                             const unsigned* __restrict__ new_index, const unsigned* __restrict__ offsets,
                                                             unsigned* __restrict__ faces, long capacity) {
  const long f = (long)blockIdx.x * SIMPLIFY_TILE + threadIdx.x;
  const bool flag = f < nf && keep[f] != 0;
  unsigned total;
  const long q = (long)offsets[blockIdx.x] + block_rank(flag, &total);
  if (!flag || q >= capacity) return;
  for (int k = 0; k < 3; ++k) {
    const int c = fcell[3 * f + k];
    faces[3 * q + k] = (c >= 0 && c < nc) ? new_index[c] : 0u;
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
int launch_simplify_keys(const double* origin, double cell, const double* xyz, long nv, long long* keys, uint8_t* bad, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_keys, dim3(tiles256(nv)), dim3(SIMPLIFY_TILE), 0, st, cloud_lattice(origin, cell), xyz, nv, keys, bad);
  ADAMVS_CHECK_LAUNCH("simplify_keys");
  return 0;
}

int launch_simplify_corners(const unsigned* faces, long nf, const int* vcell, long nv, int nc, int* fcell, int* entry_cell, uint8_t* survive,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_corners, dim3(tiles256(nf)), dim3(SIMPLIFY_TILE), 0, st, faces, nf, vcell, nv, nc, fcell, entry_cell, survive);
  ADAMVS_CHECK_LAUNCH("simplify_corners");
  return 0;
}

int launch_simplify_accumulate(const double* origin, double cell, const long long* keys, int nc, const double* xyz, const uint8_t* rgb,
                               long nv, const unsigned* faces, long nf, const long long* entry, const long long* fstart,
                               const long long* vorder, const long long* vstart, double* quadric, double* member,
                               unsigned long long* colour, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_accumulate, dim3(tiles256((long)nc * 64)), dim3(SIMPLIFY_TILE), 0, st, cloud_lattice(origin, cell), keys, nc, xyz, rgb,
                     nv, faces, nf, entry, fstart, vorder, vstart, quadric, member, colour);
  ADAMVS_CHECK_LAUNCH("simplify_accumulate");
  return 0;
}

int launch_simplify_solve(const double* origin, double cell, double rank_eps, const long long* keys, int nc, const double* quadric,
                          const double* member, const unsigned long long* colour, const long long* vstart, double* pos, uint8_t* col,
                          uint8_t* rank, uint8_t* fallback, double* error, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_solve, dim3(tiles256(nc)), dim3(SIMPLIFY_TILE), 0, st, cloud_lattice(origin, cell), rank_eps, keys, nc, quadric,
                     member, colour, vstart, pos, col, rank, fallback, error);
  ADAMVS_CHECK_LAUNCH("simplify_solve");
  return 0;
}

int launch_simplify_triples(const int* fcell, long nf, const long long* surv, long ns, int* tri, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_triples, dim3(tiles256(ns)), dim3(SIMPLIFY_TILE), 0, st, fcell, nf, surv, ns, tri);
  ADAMVS_CHECK_LAUNCH("simplify_triples");
  return 0;
}

int launch_simplify_first(const int* tri, const long long* surv, const long long* order, long ns, long nf, uint8_t* keep, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_first, dim3(tiles256(ns)), dim3(SIMPLIFY_TILE), 0, st, tri, surv, order, ns, nf, keep);
  ADAMVS_CHECK_LAUNCH("simplify_first");
  return 0;
}

int launch_simplify_mark(const int* fcell, const uint8_t* keep, long nf, int nc, uint8_t* used, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_mark, dim3(tiles256(nf)), dim3(SIMPLIFY_TILE), 0, st, fcell, keep, nf, nc, used);
  ADAMVS_CHECK_LAUNCH("simplify_mark");
  return 0;
}

int launch_simplify_count(const uint8_t* flags, long n, unsigned* block_count, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_count, dim3(tiles256(n)), dim3(SIMPLIFY_TILE), 0, st, flags, n, block_count);
  ADAMVS_CHECK_LAUNCH("simplify_count");
  return 0;
}

int launch_simplify_emit(const double* pos, const uint8_t* col, const uint8_t* used, int nc, const unsigned* cell_offsets, const int* fcell,
                         const uint8_t* keep, long nf, const unsigned* face_offsets, double* xyz, uint8_t* rgb, unsigned* new_index,
                         long vert_capacity, unsigned* faces, long face_capacity, hipStream_t st) {
  hipLaunchKernelGGL(k_simplify_emit_vertices, dim3(tiles256(nc)), dim3(SIMPLIFY_TILE), 0, st, pos, col, used, nc, cell_offsets, xyz, rgb,
                     new_index, vert_capacity);
  ADAMVS_CHECK_LAUNCH("simplify_emit_vertices");
  hipLaunchKernelGGL(k_simplify_emit_faces, dim3(tiles256(nf)), dim3(SIMPLIFY_TILE), 0, st, fcell, keep, nf, nc, new_index, face_offsets, faces,
                     face_capacity);
  ADAMVS_CHECK_LAUNCH("simplify_emit_faces");
  return 0;
}

// Step 4 on the host, for checks of the solve without a device (the same inline function the kernel runs).
void simplify_solve_host(const double* quadric, const double* mean, double cell, double rank_eps, double* p, int* rank, int* fallback,
                         double* error) {
  simplify_solve_cell(quadric, mean, cell / 2.0, rank_eps, p, rank, fallback, error);
}

}  // namespace adamvs
