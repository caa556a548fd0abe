// Mesh smoothing by bilateral normal filtering (Zheng, Fu, Au, Tai: the local iterative scheme; the step between mesh_whu.py and
// simplify_whu.py; include/adamvs_hip.h "Mesh smoothing" states every operation).  The caller (ada-mvs_amd/smooth.py) welds the
// mesh, forms p = xyz - O, sorts the (vertex, face) entries stably by vertex into runs and sorts the edge keys; the arithmetic
// is here, one lane per element:
//
//   k_smooth_faces      one lane per face: the 64-byte record  centroid, area | normal, 0  of step 1
//   k_mesh_edge_keys    one lane per edge: the key  min << 32 | max  of its corner pair (the caller sorts them); the one edge-key
//                       kernel of the library, behind adamvs_smooth_edge_keys and adamvs_texture_edge_keys
//   k_smooth_boundary   one lane per sorted key: a run of length one stores 1 at both ends of the edge (plain stores)
//   k_smooth_filter     one lane per face: the bilateral sum over N(f), gathered through the vertex -> face runs in the header's
//                       order; whether a face already appeared at an earlier corner is decided by comparing its three vertex
//                       numbers with that corner's, so a fan apex of any valence needs no list
//   k_smooth_centroids  one lane per face: the centroids of the current positions
//   k_smooth_update     one lane per vertex: the sum over F(v), the step and the clamp of step 5
//
// No atomics and no inter-workgroup waits: every lane writes only its own element, every sum runs in an order fixed by the
// sorted input, the launches are the synchronisation, and the output is bit-identical from run to run.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "kernels.h"

// The header states every value as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

typedef double double4_t __attribute__((ext_vector_type(4)));

// rec[2 f] = centroid, area;  rec[2 f + 1] = normal of step 1, 0: one aligned 64-byte record per face, read as two 32-byte halves
__device__ __forceinline__ double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

__global__ __launch_bounds__(256) void k_smooth_faces(const double* __restrict__ p, long nv, const unsigned* __restrict__ faces, long nf,
                                                      double4_t* __restrict__ rec) {
  const long f = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (f >= nf) return;
  const unsigned v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  double4_t lo = {0., 0., 0., 0.}, hi = {0., 0., 0., 0.};
  if ((long)v0 < nv && (long)v1 < nv && (long)v2 < nv) {
    const double a[3] = {p[3 * (long)v0], p[3 * (long)v0 + 1], p[3 * (long)v0 + 2]};
    const double b[3] = {p[3 * (long)v1], p[3 * (long)v1 + 1], p[3 * (long)v1 + 2]};
    const double c[3] = {p[3 * (long)v2], p[3 * (long)v2 + 1], p[3 * (long)v2 + 2]};
    const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    const double w[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double m[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
    const double len = norm3(m[0], m[1], m[2]);
    lo = double4_t{((a[0] + b[0]) + c[0]) / 3.0, ((a[1] + b[1]) + c[1]) / 3.0, ((a[2] + b[2]) + c[2]) / 3.0, len / 2.0};
    if (len > 0.0) hi = double4_t{m[0] / len, m[1] / len, m[2] / len, 0.0};
  }
  rec[2 * f] = lo;
  rec[2 * f + 1] = hi;
}

// one lane per edge, so consecutive lanes store consecutive keys; mesh cleaning and texturing take their keys from here too
__global__ __launch_bounds__(256) void k_mesh_edge_keys(const unsigned* __restrict__ faces, long n, long long* __restrict__ keys) {
  const long e = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (e >= n) return;
  unsigned a, b;
  half_edge(faces, e, a, b);
  keys[e] = edge_key(a, b);
}

__global__ __launch_bounds__(256) void k_smooth_boundary(const long long* __restrict__ keys, long n, long nv, uint8_t* __restrict__ fixed) {
  const long i = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (i >= n) return;
  if (!key_occurs_once(keys, i, n)) return;
  const long long key = keys[i];
  const long lo = (long)((unsigned long long)key >> 32), hi = (long)((unsigned long long)key & 0xFFFFFFFFull);
  if (lo < nv) fixed[lo] = 1;
  if (hi < nv) fixed[hi] = 1;
}

struct FilterTerm {
  double cf[3], nf[3], ds, dr, s[3];
};

// s += A_g exp(-(|c_f - c_g|^2 / ds + |n_f - n_g|^2 / dr)) n_g
__device__ __forceinline__ void filter_add(FilterTerm& t, const double4_t* __restrict__ rec, const double* __restrict__ nin, long g) {
  const double4_t r = rec[2 * g];
  const double n[3] = {nin[3 * g], nin[3 * g + 1], nin[3 * g + 2]};
  const double dc[3] = {t.cf[0] - r.x, t.cf[1] - r.y, t.cf[2] - r.z};
  const double dn[3] = {t.nf[0] - n[0], t.nf[1] - n[1], t.nf[2] - n[2]};
  const double dc2 = (dc[0] * dc[0] + dc[1] * dc[1]) + dc[2] * dc[2];
  const double dn2 = (dn[0] * dn[0] + dn[1] * dn[1]) + dn[2] * dn[2];
  const double w = r.w * exp(-(dc2 / t.ds + dn2 / t.dr));
  t.s[0] = t.s[0] + w * n[0];
  t.s[1] = t.s[1] + w * n[1];
  t.s[2] = t.s[2] + w * n[2];
}

__global__ __launch_bounds__(256) void k_smooth_filter(const double4_t* __restrict__ rec, const double* __restrict__ nin,
                                                       double* __restrict__ nout, const unsigned* __restrict__ faces, long nf, long nv,
                                                       const int* __restrict__ vface, const long long* __restrict__ vstart, double ds,
                                                       double dr) {
  const long f = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (f >= nf) return;
  const long ne = 3 * nf;
  const unsigned v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  FilterTerm t;
  const double4_t rf = rec[2 * f];
  t.cf[0] = rf.x, t.cf[1] = rf.y, t.cf[2] = rf.z;
  t.nf[0] = nin[3 * f], t.nf[1] = nin[3 * f + 1], t.nf[2] = nin[3 * f + 2];
  t.ds = ds, t.dr = dr;
  t.s[0] = t.s[1] = t.s[2] = 0.0;
  filter_add(t, rec, nin, f);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned v = k == 0 ? v0 : (k == 1 ? v1 : v2);
    if ((long)v >= nv) continue;
    if ((k >= 1 && v == v0) || (k == 2 && v == v1)) continue;              // the corner repeats an earlier one: its run is done
    long long i0 = vstart[v], i1 = vstart[v + 1];
    i0 = i0 < 0 ? 0 : i0;
    i1 = i1 > ne ? ne : i1;
    for (long long i = i0; i < i1; ++i) {
      const long g = vface[i];
      if (g < 0 || g >= nf || g == f) continue;
      if (k >= 1) {                                                        // did g appear in the run of an earlier corner?
        const unsigned g0 = faces[3 * g], g1 = faces[3 * g + 1], g2 = faces[3 * g + 2];
        if (g0 == v0 || g1 == v0 || g2 == v0) continue;
        if (k == 2 && (g0 == v1 || g1 == v1 || g2 == v1)) continue;
      }
      filter_add(t, rec, nin, g);
    }
  }
  const double len = norm3(t.s[0], t.s[1], t.s[2]);
  const bool ok = len > 1e-12;                                             // false for NaN
  nout[3 * f] = ok ? t.s[0] / len : t.nf[0];
  nout[3 * f + 1] = ok ? t.s[1] / len : t.nf[1];
  nout[3 * f + 2] = ok ? t.s[2] / len : t.nf[2];
}

__global__ __launch_bounds__(256) void k_smooth_centroids(const double* __restrict__ p, long nv, const unsigned* __restrict__ faces, long nf,
                                                          double* __restrict__ cen) {
  const long f = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (f >= nf) return;
  const unsigned v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  const bool ok = (long)v0 < nv && (long)v1 < nv && (long)v2 < nv;
  const long a = ok ? (long)v0 : 0, b = ok ? (long)v1 : 0, c = ok ? (long)v2 : 0;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) cen[3 * f + ax] = ((p[3 * a + ax] + p[3 * b + ax]) + p[3 * c + ax]) / 3.0;
}

__global__ __launch_bounds__(256) void k_smooth_update(const double* __restrict__ p0, const double* __restrict__ p, double* __restrict__ pout,
                                                       long nv, const double* __restrict__ nrm, const double* __restrict__ cen, long nf,
                                                       const int* __restrict__ vface, const long long* __restrict__ vstart,
                                                       const uint8_t* __restrict__ fixed, double cap, uint8_t* __restrict__ clamped) {
  const long v = (long)blockIdx.x * SMOOTH_TILE + threadIdx.x;
  if (v >= nv) return;
  const long ne = 3 * nf;
  const double x0[3] = {p0[3 * v], p0[3 * v + 1], p0[3 * v + 2]};
  long long i0 = vstart[v], i1 = vstart[v + 1];
  i0 = i0 < 0 ? 0 : i0;
  i1 = i1 > ne ? ne : i1;
  const long long count = i1 - i0;
  double out[3] = {x0[0], x0[1], x0[2]};
  bool hit = false;
  if (!fixed[v] && count > 0) {
    const double x[3] = {p[3 * v], p[3 * v + 1], p[3 * v + 2]};
    double s[3] = {0., 0., 0.};
    for (long long i = i0; i < i1; ++i) {
      const long f = vface[i];
      if (f < 0 || f >= nf) continue;
      const double n[3] = {nrm[3 * f], nrm[3 * f + 1], nrm[3 * f + 2]};
      const double e[3] = {cen[3 * f] - x[0], cen[3 * f + 1] - x[1], cen[3 * f + 2] - x[2]};
      const double t = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
      s[0] = s[0] + n[0] * t;
      s[1] = s[1] + n[1] * t;
      s[2] = s[2] + n[2] * t;
    }
    const double cnt = (double)count;
    const double d[3] = {(x[0] + s[0] / cnt) - x0[0], (x[1] + s[1] / cnt) - x0[1], (x[2] + s[2] / cnt) - x0[2]};
    const double len = norm3(d[0], d[1], d[2]);
    hit = len > cap;
    const double t = hit ? cap / len : 1.0;
    out[0] = x0[0] + d[0] * t, out[1] = x0[1] + d[1] * t, out[2] = x0[2] + d[2] * t;
  }
  pout[3 * v] = out[0], pout[3 * v + 1] = out[1], pout[3 * v + 2] = out[2];
  clamped[v] = (uint8_t)hit;
}

// ---- launches -----------------------------------------------------------------------------------------------------------
int launch_smooth_faces(const double* p, long nv, const unsigned* faces, long nf, double* rec, hipStream_t st) {
  hipLaunchKernelGGL(k_smooth_faces, dim3(tiles256(nf)), dim3(SMOOTH_TILE), 0, st, p, nv, faces, nf, (double4_t*)rec);
  ADAMVS_CHECK_LAUNCH("smooth_faces");
  return 0;
}

int launch_mesh_edge_keys(const unsigned* faces, long nf, long long* keys, const char* what, hipStream_t st) {
  if (nf == 0) return 0;
  hipLaunchKernelGGL(k_mesh_edge_keys, dim3(tiles256(3 * nf)), dim3(SMOOTH_TILE), 0, st, faces, 3 * nf, keys);
  ADAMVS_CHECK_LAUNCH(what);
  return 0;
}

int launch_smooth_boundary(const long long* keys, long n, long nv, uint8_t* fixed, hipStream_t st) {
  hipLaunchKernelGGL(k_smooth_boundary, dim3(tiles256(n)), dim3(SMOOTH_TILE), 0, st, keys, n, nv, fixed);
  ADAMVS_CHECK_LAUNCH("smooth_boundary");
  return 0;
}

int launch_smooth_filter(const double* rec, const double* nin, double* nout, const unsigned* faces, long nf, long nv, const int* vface,
                         const long long* vstart, double sigma_s, double sigma_r, hipStream_t st) {
  const double ds = 2.0 * sigma_s * sigma_s, dr = 2.0 * sigma_r * sigma_r;
  hipLaunchKernelGGL(k_smooth_filter, dim3(tiles256(nf)), dim3(SMOOTH_TILE), 0, st, (const double4_t*)rec, nin, nout, faces, nf, nv, vface,
                     vstart, ds, dr);
  ADAMVS_CHECK_LAUNCH("smooth_filter");
  return 0;
}

int launch_smooth_centroids(const double* p, long nv, const unsigned* faces, long nf, double* cen, hipStream_t st) {
  hipLaunchKernelGGL(k_smooth_centroids, dim3(tiles256(nf)), dim3(SMOOTH_TILE), 0, st, p, nv, faces, nf, cen);
  ADAMVS_CHECK_LAUNCH("smooth_centroids");
  return 0;
}

int launch_smooth_update(const double* p0, const double* p, double* pout, long nv, const double* nrm, const double* cen, long nf,
                         const int* vface, const long long* vstart, const uint8_t* fixed, double cap, uint8_t* clamped, hipStream_t st) {
  hipLaunchKernelGGL(k_smooth_update, dim3(tiles256(nv)), dim3(SMOOTH_TILE), 0, st, p0, p, pout, nv, nrm, cen, nf, vface, vstart, fixed, cap,
                     clamped);
  ADAMVS_CHECK_LAUNCH("smooth_update");
  return 0;
}

}  // namespace adamvs
