// Mesh cleaning: small components dropped and small holes closed (the step between mesh_whu.py and smooth_whu.py;
// include/adamvs_hip.h "Mesh cleaning" states every operation).  The caller (ada-mvs_amd/clean.py) welds the mesh, drops the
// degenerate faces, forms p = xyz - O and does the sorts, the scans and the compactions with torch; the rest is here, one lane
// per element:
//
//   k_clean_hook / k_clean_compress   one round of the vertex labels: every face hooks the larger roots of its corners to the
//                                     smallest (read from the previous round's snapshot, integer atomicMin into the new one),
//                                     then every vertex walks to its root (block_prims.h compress_to_root)
//   k_clean_area_chunks / _segments   the area of every component: one lane per chunk of 1024 sorted faces, then one per component
//   k_clean_boundary                  one lane per sorted edge key: whether its half-edge is the only one with that key
//   k_clean_vinit / _count / _succ    per vertex the boundary half-edges leaving and entering it, and every half-edge's successor
//   k_clean_double                    one round of pointer doubling over the successor map
//   k_clean_mark / k_clean_decide     which label groups are whole loops, and which of those are short enough to close
//   k_clean_accumulate                one lane per closed loop: the centre and its colour, summed in ascending half-edge
//   k_clean_emit_*                    the output: surviving vertices and faces renumbered, the fill vertices and the fans
//
// The only atomics are integer atomicMin and atomicAdd whose results do not depend on the order (a minimum, a count); every
// floating-point sum runs in an order fixed by the sorted input, so the output is bit-identical from run to run.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace adamvs {

// ---- components -------------------------------------------------------------------------------------------------------------
// pin is the snapshot the round starts from (every pin[v] is a root: pin[pin[v]] == pin[v]); pout starts as its copy
__global__ __launch_bounds__(256) void k_clean_hook(const unsigned* __restrict__ faces, long nf, long nv, const int* __restrict__ pin,
                                                    int* pout, unsigned* __restrict__ changed) {
  const long f = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (f >= nf) return;
  const unsigned v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  if ((long)v0 >= nv || (long)v1 >= nv || (long)v2 >= nv) return;
  const int r0 = pin[v0], r1 = pin[v1], r2 = pin[v2];
  const int m = min(r0, min(r1, r2));
  if (m < 0 || (long)max(r0, max(r1, r2)) >= nv) return;
  bool any = false;
  if (r0 != m) atomicMin(pout + r0, m), any = true;
  if (r1 != m) atomicMin(pout + r1, m), any = true;
  if (r2 != m) atomicMin(pout + r2, m), any = true;
  if (any) changed[0] = 1u;
}

__global__ __launch_bounds__(256) void k_clean_compress(int* parent, long nv) {
  const long v = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (v < nv) compress_to_root(parent, v);
}

// ---- component areas ----------------------------------------------------------------------------------------------------------
// chunk j covers the sorted positions [j C, (j + 1) C).  Its first piece (the positions up to the first change of component)
// goes to lead[j]; every later piece begins a component and goes to first[that component].
__global__ __launch_bounds__(256) void k_clean_area_chunks(const double* __restrict__ area, long nf, const long long* __restrict__ order,
                                                           const long long* __restrict__ seg_of, long ncomp, double* __restrict__ lead,
                                                           double* __restrict__ first) {
  const long j = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  const long p0 = j * CLEAN_CHUNK;
  if (p0 >= nf) return;
  const long p1 = p0 + CLEAN_CHUNK < nf ? p0 + CLEAN_CHUNK : nf;
  long long cur = seg_of[p0];
  bool leading = true;
  double acc = 0.0;
  for (long i = p0; i < p1; ++i) {
    const long long s = seg_of[i];
    if (s != cur) {
      if (leading) lead[j] = acc;
      else if (cur >= 0 && cur < ncomp) first[cur] = acc;
      leading = false, cur = s, acc = 0.0;
    }
    const long long f = order[i];
    acc = acc + ((f >= 0 && f < nf) ? area[f] : 0.0);
  }
  if (leading) lead[j] = acc;
  else if (cur >= 0 && cur < ncomp) first[cur] = acc;
}

__global__ __launch_bounds__(256) void k_clean_area_segments(const long long* __restrict__ seg_start, long ncomp, long nf,
                                                             const double* __restrict__ lead, const double* __restrict__ first,
                                                             double* __restrict__ out) {
  const long c = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (c >= ncomp) return;
  long long s = seg_start[c], e = seg_start[c + 1];
  s = s < 0 ? 0 : s;
  e = e > nf ? nf : e;
  double total = 0.0;
  if (e > s) {
    long j = s / CLEAN_CHUNK;
    const long j1 = (e - 1) / CLEAN_CHUNK;
    if (s % CLEAN_CHUNK != 0) total = first[c], ++j;
    for (; j <= j1; ++j) total = total + lead[j];
  }
  out[c] = total;
}

// ---- boundary -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clean_boundary(const long long* __restrict__ keys, const long long* __restrict__ entry, long n,
                                                        uint8_t* __restrict__ bnd) {
  const long i = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (i >= n) return;
  const long long h = entry[i];
  const bool once = key_occurs_once(keys, i, n);
  if (h >= 0 && h < n) bnd[h] = (uint8_t)once;
}

__global__ __launch_bounds__(256) void k_clean_vinit(int* __restrict__ out_cnt, int* __restrict__ in_cnt, int* __restrict__ out_he, long nv) {
  const long v = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (v >= nv) return;
  out_cnt[v] = 0, in_cnt[v] = 0, out_he[v] = 0x7FFFFFFF;
}

__global__ __launch_bounds__(256) void k_clean_count(const unsigned* __restrict__ faces, long n, long nv, const uint8_t* __restrict__ bnd,
                                                     int* out_cnt, int* in_cnt, int* out_he) {
  const long h = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (h >= n || !bnd[h]) return;
  unsigned a, b;
  half_edge(faces, h, a, b);
  if ((long)a >= nv || (long)b >= nv) return;
  atomicAdd(out_cnt + a, 1);
  atomicAdd(in_cnt + b, 1);
  atomicMin(out_he + a, (int)h);
}

__global__ __launch_bounds__(256) void k_clean_succ(const unsigned* __restrict__ faces, long n, long nv, const uint8_t* __restrict__ bnd,
                                                    const int* __restrict__ out_cnt, const int* __restrict__ in_cnt,
                                                    const int* __restrict__ out_he, int* __restrict__ succ, int* __restrict__ lab,
                                                    int* __restrict__ nxt, uint8_t* __restrict__ broken) {
  const long h = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (h >= n) return;
  int s = -1;
  if (bnd[h]) {
    unsigned a, b;
    half_edge(faces, h, a, b);
    if ((long)b < nv && out_cnt[b] == 1 && in_cnt[b] == 1) {
      const int g = out_he[b];
      if (g >= 0 && (long)g < n && bnd[g]) s = g;
    }
  }
  succ[h] = s;
  lab[h] = (int)h;
  nxt[h] = s < 0 ? (int)h : s;
  broken[h] = (uint8_t)(s < 0);
}

// ---- loops ----------------------------------------------------------------------------------------------------------------------
// Half-edges off the boundary point at themselves, nobody points at them and both buffers hold their initial values: skipped.
__global__ __launch_bounds__(256) void k_clean_double(const uint8_t* __restrict__ bnd, long n, const int* __restrict__ lab_in,
                                                      const int* __restrict__ nxt_in, const uint8_t* __restrict__ broken_in,
                                                      int* __restrict__ lab_out, int* __restrict__ nxt_out, uint8_t* __restrict__ broken_out) {
  const long h = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (h >= n || !bnd[h]) return;
  int j = nxt_in[h];
  if (j < 0 || (long)j >= n) j = (int)h;
  const int la = lab_in[h], lb = lab_in[j];
  lab_out[h] = la < lb ? la : lb;
  broken_out[h] = (uint8_t)(broken_in[h] | broken_in[j]);
  const int jj = nxt_in[j];
  nxt_out[h] = (jj < 0 || (long)jj >= n) ? j : jj;
}

// a label group is a whole loop only if none of its members is broken and every member's ORIGINAL successor carries its label
__global__ __launch_bounds__(256) void k_clean_mark(const uint8_t* __restrict__ bnd, const int* __restrict__ succ, const int* __restrict__ lab,
                                                    const uint8_t* __restrict__ broken, long n, int* cnt, uint8_t* bad) {
  const long h = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (h >= n || !bnd[h]) return;
  const int l = lab[h];
  if (l < 0 || (long)l >= n) return;
  const int s = succ[h];
  const bool ok = !broken[h] && s >= 0 && (long)s < n && lab[s] == l;
  atomicAdd(cnt + l, 1);
  if (!ok) bad[l] = 1;
}

__global__ __launch_bounds__(256) void k_clean_decide(const uint8_t* __restrict__ bnd, const int* __restrict__ lab, long n, int M,
                                                      const int* __restrict__ cnt, const uint8_t* __restrict__ bad, int* __restrict__ loop,
                                                      uint8_t* __restrict__ closed) {
  const long h = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (h >= n) return;
  int l = bnd[h] ? lab[h] : -1;
  if (l < 0 || (long)l >= n || bad[l] || !bnd[l] || lab[l] != l) l = -1;
  loop[h] = l;
  closed[h] = (uint8_t)(l >= 0 && cnt[l] >= 3 && cnt[l] <= M);
}

// ---- fill -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_clean_accumulate(const double* __restrict__ p, const uint8_t* __restrict__ rgb, long nv,
                                                          const unsigned* __restrict__ faces, long n, const int* __restrict__ members,
                                                          const long long* __restrict__ start, long nl, long nm, double ox, double oy,
                                                          double oz, double* __restrict__ centre, uint8_t* __restrict__ colour) {
  const long l = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (l >= nl) return;
  long long i0 = start[l], i1 = start[l + 1];
  i0 = i0 < 0 ? 0 : i0;
  i1 = i1 > nm ? nm : i1;
  double s[3] = {0., 0., 0.};
  long long c[3] = {0, 0, 0};
  for (long long i = i0; i < i1; ++i) {
    const long h = members[i];
    if (h < 0 || h >= n) continue;
    unsigned a, b;
    half_edge(faces, h, a, b);
    if ((long)a >= nv) continue;
    s[0] = s[0] + p[3 * (long)a], s[1] = s[1] + p[3 * (long)a + 1], s[2] = s[2] + p[3 * (long)a + 2];
    c[0] += rgb[3 * (long)a], c[1] += rgb[3 * (long)a + 1], c[2] += rgb[3 * (long)a + 2];
  }
  const double L = (double)(i1 > i0 ? i1 - i0 : 1);
  const double o[3] = {ox, oy, oz};
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) {
    centre[3 * l + ax] = o[ax] + s[ax] / L;
    colour[3 * l + ax] = (uint8_t)floor((double)c[ax] / L + 0.5);
  }
}

__global__ __launch_bounds__(256) void k_clean_emit_vertices(const double* __restrict__ xyz, const uint8_t* __restrict__ rgb, long nv,
                                                             const int* __restrict__ new_index, long nvs, double* __restrict__ xyz_out,
                                                             uint8_t* __restrict__ rgb_out) {
  const long v = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (v >= nv) return;
  const long i = new_index[v];
  if (i < 0 || i >= nvs) return;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) xyz_out[3 * i + ax] = xyz[3 * v + ax], rgb_out[3 * i + ax] = rgb[3 * v + ax];
}

__global__ __launch_bounds__(256) void k_clean_emit_centres(const double* __restrict__ centre, const uint8_t* __restrict__ colour, long nl,
                                                            long nvs, double* __restrict__ xyz_out, uint8_t* __restrict__ rgb_out) {
  const long l = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (l >= nl) return;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) xyz_out[3 * (nvs + l) + ax] = centre[3 * l + ax], rgb_out[3 * (nvs + l) + ax] = colour[3 * l + ax];
}

__device__ __forceinline__ unsigned renumber(const int* __restrict__ new_index, long nv, unsigned v) {
  return (long)v < nv && new_index[v] >= 0 ? (unsigned)new_index[v] : 0u;
}

__global__ __launch_bounds__(256) void k_clean_emit_faces(const unsigned* __restrict__ faces, long ns, long nv, const int* __restrict__ new_index,
                                                          unsigned* __restrict__ out) {
  const long e = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (e >= 3 * ns) return;
  out[e] = renumber(new_index, nv, faces[e]);
}

// the fan: half-edge a -> b of a closed loop gives the face (b, a, centre), so the shared edge runs the other way in it
__global__ __launch_bounds__(256) void k_clean_emit_fans(const unsigned* __restrict__ faces, long ns, long nv, const int* __restrict__ new_index,
                                                         const int* __restrict__ fill_h, const int* __restrict__ loop_of, long nfill, long nl,
                                                         long nvs, unsigned* __restrict__ out) {
  const long j = (long)blockIdx.x * CLEAN_TILE + threadIdx.x;
  if (j >= nfill) return;
  const long h = fill_h[j], l = loop_of[j];
  unsigned a = 0, b = 0;
  if (h >= 0 && h < 3 * ns) half_edge(faces, h, a, b);
  unsigned* o = out + 3 * (ns + j);
  o[0] = renumber(new_index, nv, b);
  o[1] = renumber(new_index, nv, a);
  o[2] = (unsigned)(nvs + (l >= 0 && l < nl ? l : 0));
}

// ---- launches -----------------------------------------------------------------------------------------------------------
#define CLEAN_ASYNC(call, what) \
  do { hipError_t e_ = (call); \
       if (e_ != hipSuccess) return set_error((int)e_, "%s: %s", what, hipGetErrorString(e_)); } while (0)

int launch_clean_components(const unsigned* faces, long nf, long nv, const int* parent_in, int* parent_out, unsigned* changed,
                            hipStream_t st) {
  CLEAN_ASYNC(hipMemsetAsync(changed, 0, sizeof(unsigned), st), "clean_components: hipMemsetAsync");
  CLEAN_ASYNC(hipMemcpyAsync(parent_out, parent_in, sizeof(int) * (size_t)nv, hipMemcpyDeviceToDevice, st), "clean_components: hipMemcpyAsync");
  hipLaunchKernelGGL(k_clean_hook, dim3(tiles256(nf)), dim3(CLEAN_TILE), 0, st, faces, nf, nv, parent_in, parent_out, changed);
  ADAMVS_CHECK_LAUNCH("clean_hook");
  hipLaunchKernelGGL(k_clean_compress, dim3(tiles256(nv)), dim3(CLEAN_TILE), 0, st, parent_out, nv);
  ADAMVS_CHECK_LAUNCH("clean_compress");
  return 0;
}

int launch_clean_area(const double* area, long nf, const long long* order, const long long* seg_of, const long long* seg_start, long ncomp,
                      double* lead, double* first, double* out, hipStream_t st) {
  const long chunks = (nf + CLEAN_CHUNK - 1) / CLEAN_CHUNK;
  hipLaunchKernelGGL(k_clean_area_chunks, dim3(tiles256(chunks)), dim3(CLEAN_TILE), 0, st, area, nf, order, seg_of, ncomp, lead, first);
  ADAMVS_CHECK_LAUNCH("clean_area_chunks");
  hipLaunchKernelGGL(k_clean_area_segments, dim3(tiles256(ncomp)), dim3(CLEAN_TILE), 0, st, seg_start, ncomp, nf, lead, first, out);
  ADAMVS_CHECK_LAUNCH("clean_area_segments");
  return 0;
}

int launch_clean_boundary(const long long* keys, const long long* entry, long n, uint8_t* bnd, hipStream_t st) {
  hipLaunchKernelGGL(k_clean_boundary, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, keys, entry, n, bnd);
  ADAMVS_CHECK_LAUNCH("clean_boundary");
  return 0;
}

int launch_clean_successor(const unsigned* faces, long ns, long nv, const uint8_t* bnd, int* out_cnt, int* in_cnt, int* out_he, int* succ,
                           int* lab, int* nxt, uint8_t* broken, hipStream_t st) {
  const long n = 3 * ns;
  hipLaunchKernelGGL(k_clean_vinit, dim3(tiles256(nv)), dim3(CLEAN_TILE), 0, st, out_cnt, in_cnt, out_he, nv);
  ADAMVS_CHECK_LAUNCH("clean_vinit");
  hipLaunchKernelGGL(k_clean_count, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, faces, n, nv, bnd, out_cnt, in_cnt, out_he);
  ADAMVS_CHECK_LAUNCH("clean_count");
  hipLaunchKernelGGL(k_clean_succ, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, faces, n, nv, bnd, out_cnt, in_cnt, out_he, succ, lab, nxt,
                     broken);
  ADAMVS_CHECK_LAUNCH("clean_succ");
  return 0;
}

int launch_clean_double(const uint8_t* bnd, long n, const int* lab_in, const int* nxt_in, const uint8_t* broken_in, int* lab_out, int* nxt_out,
                        uint8_t* broken_out, hipStream_t st) {
  hipLaunchKernelGGL(k_clean_double, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, bnd, n, lab_in, nxt_in, broken_in, lab_out, nxt_out,
                     broken_out);
  ADAMVS_CHECK_LAUNCH("clean_double");
  return 0;
}

int launch_clean_validate(const uint8_t* bnd, const int* succ, const int* lab, const uint8_t* broken, long n, int M, int* cnt, uint8_t* bad,
                          int* loop, uint8_t* closed, hipStream_t st) {
  CLEAN_ASYNC(hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)n, st), "clean_validate: hipMemsetAsync");
  CLEAN_ASYNC(hipMemsetAsync(bad, 0, (size_t)n, st), "clean_validate: hipMemsetAsync");
  hipLaunchKernelGGL(k_clean_mark, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, bnd, succ, lab, broken, n, cnt, bad);
  ADAMVS_CHECK_LAUNCH("clean_mark");
  hipLaunchKernelGGL(k_clean_decide, dim3(tiles256(n)), dim3(CLEAN_TILE), 0, st, bnd, lab, n, M, cnt, bad, loop, closed);
  ADAMVS_CHECK_LAUNCH("clean_decide");
  return 0;
}

int launch_clean_accumulate(const double* p, const uint8_t* rgb, long nv, const unsigned* faces, long ns, const int* members,
                            const long long* start, long nl, long nm, const double* origin, double* centre, uint8_t* colour, hipStream_t st) {
  hipLaunchKernelGGL(k_clean_accumulate, dim3(tiles256(nl)), dim3(CLEAN_TILE), 0, st, p, rgb, nv, faces, 3 * ns, members, start, nl, nm,
                     origin[0], origin[1], origin[2], centre, colour);
  ADAMVS_CHECK_LAUNCH("clean_accumulate");
  return 0;
}

int launch_clean_emit(const double* xyz, const uint8_t* rgb, long nv, const int* new_index, const unsigned* faces, long ns, const int* fill_h,
                      const int* loop_of, long nfill, const double* centre, const uint8_t* colour, long nl, long nvs, double* xyz_out,
                      uint8_t* rgb_out, unsigned* faces_out, hipStream_t st) {
  hipLaunchKernelGGL(k_clean_emit_vertices, dim3(tiles256(nv)), dim3(CLEAN_TILE), 0, st, xyz, rgb, nv, new_index, nvs, xyz_out, rgb_out);
  ADAMVS_CHECK_LAUNCH("clean_emit_vertices");
  hipLaunchKernelGGL(k_clean_emit_faces, dim3(tiles256(3 * ns)), dim3(CLEAN_TILE), 0, st, faces, ns, nv, new_index, faces_out);
  ADAMVS_CHECK_LAUNCH("clean_emit_faces");
  if (nl > 0) {
    hipLaunchKernelGGL(k_clean_emit_centres, dim3(tiles256(nl)), dim3(CLEAN_TILE), 0, st, centre, colour, nl, nvs, xyz_out, rgb_out);
    ADAMVS_CHECK_LAUNCH("clean_emit_centres");
  }
  if (nfill > 0) {
    hipLaunchKernelGGL(k_clean_emit_fans, dim3(tiles256(nfill)), dim3(CLEAN_TILE), 0, st, faces, ns, nv, new_index, fill_h, loop_of, nfill,
                       nl, nvs, faces_out);
    ADAMVS_CHECK_LAUNCH("clean_emit_fans");
  }
  return 0;
}

}  // namespace adamvs
