// Global seam levelling of the textured mesh (the opt-in step after texture.hip; include/adamvs_hip.h "Mesh texturing",
// "Seam levelling", states every operation).  The node graph (one node per (vertex, chart)) arrives as a CSR whose column
// words carry the edge kind: bit 31 a data edge (weight 1), otherwise a smoothness edge (weight 1 / lambda), bit 30 a
// smoothness edge that lies on a seam; the low 30 bits are the neighbour.  Rows are sorted by neighbour.
//
//   k_lvl_observe       one lane per node: the observed colour f (fp32), averaged along the node's seam edges
//   k_lvl_rhs           one lane per node: b = sum over data neighbours of (f_j - f_i) (fp64)
//   k_lvl_init          g = 0, r = p = b and the partials of b.b
//   k_lvl_spmv          Ap = L p by row gather and the partials of p.Ap
//   k_lvl_update_xr     g += alpha p, r -= alpha Ap and the partials of r.r
//   k_lvl_update_p      p = r + beta p
//   k_lvl_reduce_*      one workgroup: the partials summed in a fixed order into alpha / beta / the stop flag
//   k_lvl_owner_small   one lane per textured face: atomicMin of the face index on the texels of its image triangle
//   k_lvl_owner_large   one wave per listed face on a resident grid
//   k_lvl_dilate        one lane per chart texel: one round of the owner dilation (double-buffered)
//   k_lvl_apply         one lane per chart texel: g interpolated in the owner's triangle and added to the texel
//
// Three channels are one interleaved vector [n][3] sharing the matrix, each with its own alpha and beta.  No floating-point
// atomics: every vector entry is owned by one lane, every dot product is LVL_BLOCKS-shaped partials (each workgroup owns a
// fixed run of rows, lanes stride it, a fixed shuffle tree and a fixed sum over the four waves) summed by one workgroup in
// a fixed order.  The scalars and the stop flag stay on the device (state[]): once the flag is set every later launch
// returns without writing, so g and the iteration count are those of the stopping iteration.  The only atomics are the
// owner's integer min (order-independent) and the large-face list counter.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "persistent.h"
#include "raster.h"

#include <climits>

#pragma clang fp contract(off)

namespace adamvs {

constexpr int LVL_BATCH = 8;                  // CSR entries of a row in flight at once in the SpMV
constexpr unsigned LVL_DATA = 0x80000000u, LVL_SEAM = 0x40000000u, LVL_INDEX = 0x3FFFFFFFu;
// state[]: r.r, b.b, alpha, beta per channel, the stop flag, the iteration count, tol^2
constexpr int ST_RR = 0, ST_BB = 3, ST_ALPHA = 6, ST_BETA = 9, ST_DONE = 12, ST_ITERS = 13, ST_TOL2 = 14;

static int lvl_grid(long n) {
  const long b = tiles256(n);
  return (int)(b < 1 ? 1 : (b < TEX_LEVEL_BLOCKS ? b : TEX_LEVEL_BLOCKS));
}

// ---- observed colour ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void lvl_sample(const unsigned* __restrict__ rgba, int W, int H, float x, float y, float s[3]) {
  // the orthophoto's bilinear sample; the clamps only guard (a textured face's corners lie inside its image)
  x = fminf(fmaxf(x, 0.f), (float)(W - 1));
  y = fminf(fmaxf(y, 0.f), (float)(H - 1));
  const int xa = (int)floorf(x), ya = (int)floorf(y);
  const float fx = x - (float)xa, fy = y - (float)ya;
  const int xb = xa + 1 < W ? xa + 1 : W - 1, yb = ya + 1 < H ? ya + 1 : H - 1;
  const unsigned p00 = rgba[(long)ya * W + xa], p10 = rgba[(long)ya * W + xb];
  const unsigned p01 = rgba[(long)yb * W + xa], p11 = rgba[(long)yb * W + xb];
  for (int ch = 0; ch < 3; ++ch) {
    const float c00 = (float)((p00 >> (8 * ch)) & 255u), c10 = (float)((p10 >> (8 * ch)) & 255u);
    const float c01 = (float)((p01 >> (8 * ch)) & 255u), c11 = (float)((p11 >> (8 * ch)) & 255u);
    s[ch] = (1.f - fy) * ((1.f - fx) * c00 + fx * c10) + fy * ((1.f - fx) * c01 + fx * c11);
  }
}

__global__ __launch_bounds__(256) void k_lvl_observe(const long long* __restrict__ view_tab, int nviews, const int* __restrict__ rowptr,
                                                     const unsigned* __restrict__ col, long nnz, const int* __restrict__ node_view,
                                                     const float* __restrict__ pos, long n, float* __restrict__ f) {
  const long i = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (i >= n) return;
  const int v = node_view[i];
  float acc[3] = {0.f, 0.f, 0.f}, s[3];
  if (v < 0 || v >= nviews) {
    for (int ch = 0; ch < 3; ++ch) f[3 * i + ch] = 0.f;
    return;
  }
  const unsigned* rgba = (const unsigned*)view_tab[3 * v];
  const int W = (int)view_tab[3 * v + 1], H = (int)view_tab[3 * v + 2];
  const float pu = pos[2 * i], pv = pos[2 * i + 1];
  float wsum = 0.f;
  long a = rowptr[i], e = rowptr[i + 1];
  a = a < 0 ? 0 : a;
  e = e > nnz ? nnz : e;
  for (long k = a; k < e; ++k) {
    const unsigned cj = col[k];
    if ((cj & LVL_DATA) || !(cj & LVL_SEAM)) continue;
    const long j = cj & LVL_INDEX;
    if (j >= n) continue;
    const float du = pos[2 * j] - pu, dv = pos[2 * j + 1] - pv;
    const float ts[3] = {0.f, 0.25f, 0.5f}, ws[3] = {1.f, 0.75f, 0.5f};
    for (int t = 0; t < 3; ++t) {
      lvl_sample(rgba, W, H, pu + ts[t] * du, pv + ts[t] * dv, s);
      for (int ch = 0; ch < 3; ++ch) acc[ch] = acc[ch] + ws[t] * s[ch];
      wsum = wsum + ws[t];
    }
  }
  if (wsum == 0.f) {
    lvl_sample(rgba, W, H, pu, pv, s);
    for (int ch = 0; ch < 3; ++ch) f[3 * i + ch] = s[ch];
    return;
  }
  for (int ch = 0; ch < 3; ++ch) f[3 * i + ch] = acc[ch] / wsum;
}

__global__ __launch_bounds__(256) void k_lvl_rhs(const int* __restrict__ rowptr, const unsigned* __restrict__ col, long nnz,
                                                 const float* __restrict__ f, long n, double* __restrict__ b) {
  const long i = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (i >= n) return;
  double s[3] = {0.0, 0.0, 0.0};
  const double fi[3] = {(double)f[3 * i], (double)f[3 * i + 1], (double)f[3 * i + 2]};
  long a = rowptr[i], e = rowptr[i + 1];
  a = a < 0 ? 0 : a;
  e = e > nnz ? nnz : e;
  for (long k = a; k < e; ++k) {
    const unsigned cj = col[k];
    const long j = cj & LVL_INDEX;
    if (!(cj & LVL_DATA) || j >= n) continue;
    for (int ch = 0; ch < 3; ++ch) s[ch] += (double)f[3 * j + ch] - fi[ch];
  }
  for (int ch = 0; ch < 3; ++ch) b[3 * i + ch] = s[ch];
}

// ---- conjugate gradients ----------------------------------------------------------------------------------------------
// The workgroup's three sums -> out[0..2]: a xor tree over the 64 lanes, then the four waves in order.
__device__ __forceinline__ void block_sum3(double v[3], double* __restrict__ out) {
  __shared__ double s[4][3];
  for (int ch = 0; ch < 3; ++ch)
    for (int m = 32; m >= 1; m >>= 1) v[ch] += __shfl_xor(v[ch], m);
  if ((threadIdx.x & 63) == 0)
    for (int ch = 0; ch < 3; ++ch) s[threadIdx.x >> 6][ch] = v[ch];
  __syncthreads();
  if (threadIdx.x == 0)
    for (int ch = 0; ch < 3; ++ch) out[ch] = ((s[0][ch] + s[1][ch]) + s[2][ch]) + s[3][ch];
}

// One workgroup: the nb partial triples summed (lane t takes t, t + 256, ... in order, then block_sum3) -> tot[0..2] in every lane.
__device__ __forceinline__ void total3(const double* __restrict__ partials, int nb, double tot[3]) {
  __shared__ double out[3];
  double v[3] = {0.0, 0.0, 0.0};
  for (int k = threadIdx.x; k < nb; k += TEX_TILE)
    for (int ch = 0; ch < 3; ++ch) v[ch] += partials[3 * k + ch];
  block_sum3(v, out);
  __syncthreads();
  for (int ch = 0; ch < 3; ++ch) tot[ch] = out[ch];
}

__device__ __forceinline__ bool lvl_converged(const double* state) {
  bool ok = true;
  for (int ch = 0; ch < 3; ++ch) ok = ok && state[ST_RR + ch] <= state[ST_TOL2] * state[ST_BB + ch];     // NaN never converges
  return ok;
}

__global__ __launch_bounds__(256) void k_lvl_init(const double* __restrict__ b, long n, long chunk, double* __restrict__ g,
                                                  double* __restrict__ r, double* __restrict__ p, double* __restrict__ partials) {
  double acc[3] = {0.0, 0.0, 0.0};
  const long lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  for (long i = lo + threadIdx.x; i < hi; i += TEX_TILE)
    for (int ch = 0; ch < 3; ++ch) {
      const double v = b[3 * i + ch];
      g[3 * i + ch] = 0.0;
      r[3 * i + ch] = v;
      p[3 * i + ch] = v;
      acc[ch] += v * v;
    }
  block_sum3(acc, partials + 3 * blockIdx.x);
}

__global__ __launch_bounds__(256) void k_lvl_reduce_init(const double* __restrict__ partials, int nb, double tol, double* state) {
  double tot[3];
  total3(partials, nb, tot);
  if (threadIdx.x != 0) return;
  for (int ch = 0; ch < 3; ++ch) {
    state[ST_RR + ch] = tot[ch];
    state[ST_BB + ch] = tot[ch];
    state[ST_ALPHA + ch] = 0.0;
    state[ST_BETA + ch] = 0.0;
  }
  state[ST_ITERS] = 0.0;
  state[ST_TOL2] = tol * tol;
  state[ST_DONE] = lvl_converged(state) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_lvl_spmv(const int* __restrict__ rowptr, const unsigned* __restrict__ col, long nnz, long n,
                                                  long chunk, double w_smooth, const double* __restrict__ p, double* __restrict__ ap,
                                                  double* __restrict__ partials, const double* __restrict__ state) {
  if (state[ST_DONE] != 0.0) return;
  double acc[3] = {0.0, 0.0, 0.0};
  const long lo = blockIdx.x * chunk, hi = lo + chunk < n ? lo + chunk : n;
  for (long i = lo + threadIdx.x; i < hi; i += TEX_TILE) {
    long a = rowptr[i], e = rowptr[i + 1];
    a = a < 0 ? 0 : a;
    e = e > nnz ? nnz : e;
    double d = 0.0, s[3] = {0.0, 0.0, 0.0};
    // LVL_BATCH entries at a time: their column words, then their gathers, are issued together (a row holds about six), and
    // the sums then run in ascending entry order as a one-by-one loop would
    for (long k0 = a; k0 < e; k0 += LVL_BATCH) {
      unsigned cj[LVL_BATCH];
      double pj[LVL_BATCH][3];
#pragma unroll
      for (int u = 0; u < LVL_BATCH; ++u) cj[u] = k0 + u < e ? col[k0 + u] : LVL_INDEX;
#pragma unroll
      for (int u = 0; u < LVL_BATCH; ++u) {
        const long j = cj[u] & LVL_INDEX;
        const bool ok = k0 + u < e && j < n;
        for (int ch = 0; ch < 3; ++ch) pj[u][ch] = ok ? p[3 * j + ch] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < LVL_BATCH; ++u) {
        if (!(k0 + u < e && (long)(cj[u] & LVL_INDEX) < n)) continue;
        const double w = (cj[u] & LVL_DATA) ? 1.0 : w_smooth;
        d += w;
        for (int ch = 0; ch < 3; ++ch) s[ch] += w * pj[u][ch];
      }
    }
    for (int ch = 0; ch < 3; ++ch) {
      const double pi = p[3 * i + ch];
      const double y = d * pi - s[ch];
      ap[3 * i + ch] = y;
      acc[ch] += pi * y;
    }
  }
  block_sum3(acc, partials + 3 * blockIdx.x);
}

__global__ __launch_bounds__(256) void k_lvl_reduce_alpha(const double* __restrict__ partials, int nb, double* state) {
  if (state[ST_DONE] != 0.0) return;
  double tot[3];
  total3(partials, nb, tot);
  if (threadIdx.x != 0) return;
  for (int ch = 0; ch < 3; ++ch) state[ST_ALPHA + ch] = tot[ch] > 0.0 ? state[ST_RR + ch] / tot[ch] : 0.0;
}

// The two update passes see the vectors as flat arrays of 3 n doubles read and written 16 bytes per lane: pair e holds the
// flat entries 2 e and 2 e + 1, of channels (2 e) mod 3 and the next.  With 3 n odd the last pair's second entry is the spare
// entry the vectors carry; it is computed on and never summed or read as data.
__device__ __forceinline__ double pick3(const double v[3], unsigned c) { return c == 0 ? v[0] : (c == 1 ? v[1] : v[2]); }

__global__ __launch_bounds__(256) void k_lvl_update_xr(long pairs, long total, long chunk, const double2* __restrict__ p,
                                                       const double2* __restrict__ ap, double2* __restrict__ g, double2* __restrict__ r,
                                                       double* __restrict__ partials, const double* __restrict__ state) {
  if (state[ST_DONE] != 0.0) return;
  const double alpha[3] = {state[ST_ALPHA], state[ST_ALPHA + 1], state[ST_ALPHA + 2]};
  double acc[3] = {0.0, 0.0, 0.0};
  const long lo = blockIdx.x * chunk, hi = lo + chunk < pairs ? lo + chunk : pairs;
  for (long e = lo + threadIdx.x; e < hi; e += TEX_TILE) {
    const unsigned c0 = (unsigned)((2 * (unsigned long)e) % 3u), c1 = c0 == 2u ? 0u : c0 + 1u;
    const double a0 = pick3(alpha, c0), a1 = pick3(alpha, c1);
    const double2 P = p[e], A = ap[e];
    double2 G = g[e], R = r[e];
    G.x = G.x + a0 * P.x;
    G.y = G.y + a1 * P.y;
    R.x = R.x - a0 * A.x;
    R.y = R.y - a1 * A.y;
    g[e] = G;
    r[e] = R;
    const double sx = R.x * R.x, sy = 2 * e + 1 < total ? R.y * R.y : 0.0;
    for (unsigned ch = 0; ch < 3; ++ch) acc[ch] += (c0 == ch ? sx : 0.0) + (c1 == ch ? sy : 0.0);
  }
  block_sum3(acc, partials + 3 * blockIdx.x);
}

__global__ __launch_bounds__(256) void k_lvl_reduce_beta(const double* __restrict__ partials, int nb, double* state) {
  if (state[ST_DONE] != 0.0) return;
  double tot[3];
  total3(partials, nb, tot);
  if (threadIdx.x != 0) return;
  for (int ch = 0; ch < 3; ++ch) {
    const double old = state[ST_RR + ch];
    // a channel whose step was refused (alpha = 0: p.Ap <= 0 or NaN) restarts from its residual: beta = r'.r' / r.r would be 1
    // there and p = r + p would double every iteration until it overflows and 0 * inf reaches g
    state[ST_BETA + ch] = old > 0.0 && state[ST_ALPHA + ch] != 0.0 ? tot[ch] / old : 0.0;
    state[ST_RR + ch] = tot[ch];
  }
  state[ST_ITERS] = state[ST_ITERS] + 1.0;
  state[ST_DONE] = lvl_converged(state) ? 1.0 : 0.0;
}

__global__ __launch_bounds__(256) void k_lvl_update_p(long pairs, long chunk, const double2* __restrict__ r, double2* __restrict__ p,
                                                      const double* __restrict__ state) {
  if (state[ST_DONE] != 0.0) return;
  const double beta[3] = {state[ST_BETA], state[ST_BETA + 1], state[ST_BETA + 2]};
  const long lo = blockIdx.x * chunk, hi = lo + chunk < pairs ? lo + chunk : pairs;
  for (long e = lo + threadIdx.x; e < hi; e += TEX_TILE) {
    const unsigned c0 = (unsigned)((2 * (unsigned long)e) % 3u), c1 = c0 == 2u ? 0u : c0 + 1u;
    const double2 R = r[e];
    double2 P = p[e];
    P.x = R.x + pick3(beta, c0) * P.x;
    P.y = R.y + pick3(beta, c1) * P.y;
    p[e] = P;
  }
}

// ---- owner, dilation, apply ------------------------------------------------------------------------------------------
// Face f's image triangle clamped to its chart's box (x0, y0, w, h); pixel centres are the chart's texel centres.
__device__ __forceinline__ bool lvl_tri(const float* __restrict__ q, const int* __restrict__ c, Tri& t) {
  for (int k = 0; k < 3; ++k)
    if (!tri_vertex(q[2 * k], q[2 * k + 1], 1.f, k, t)) return false;
  if (c[2] < 1 || c[3] < 1 || !tri_setup(t, c[0] + c[2], c[1] + c[3])) return false;
  t.u0 = t.u0 < c[0] ? c[0] : t.u0;
  t.v0 = t.v0 < c[1] ? c[1] : t.v0;
  return t.u0 <= t.u1 && t.v0 <= t.v1;
}

__device__ __forceinline__ void lvl_owner_pixel(const Tri& t, int pu, int pv, const int* __restrict__ c, long base, long texels, int f,
                                                int* __restrict__ owner) {
  const float x = (float)pu, y = (float)pv;
  const float e0 = (t.u[2] - t.u[1]) * (y - t.v[1]) - (t.v[2] - t.v[1]) * (x - t.u[1]);
  const float e1 = (t.u[0] - t.u[2]) * (y - t.v[2]) - (t.v[0] - t.v[2]) * (x - t.u[2]);
  const float e2 = (t.u[1] - t.u[0]) * (y - t.v[0]) - (t.v[1] - t.v[0]) * (x - t.u[0]);
  if (!(e0 >= 0.f && e1 >= 0.f && e2 >= 0.f)) return;
  const long k = base + (long)(pv - c[1]) * c[2] + (pu - c[0]);
  if (k >= 0 && k < texels) atomicMin(owner + k, f);
}

__global__ __launch_bounds__(256) void k_lvl_owner_clear(int* __restrict__ owner, long n) {
  const long k = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (k < n) owner[k] = INT_MAX;
}

__global__ __launch_bounds__(256) void k_lvl_owner_small(const float* __restrict__ uv, const int* __restrict__ chart, long nf,
                                                         const int* __restrict__ charts, const long long* __restrict__ prefix, int nc,
                                                         long texels, int* __restrict__ owner, unsigned* __restrict__ big_count,
                                                         unsigned* __restrict__ big_list) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (f >= nf) return;
  const int ci = chart[f];
  if (ci < 0 || ci >= nc) return;
  const int* c = charts + 8 * (long)ci;
  Tri t;
  if (!lvl_tri(uv + 6 * f, c, t)) return;
  const int bw = t.u1 - t.u0 + 1, bh = t.v1 - t.v0 + 1;
  if ((long)bw * bh > ORTHO_SMALL_PX) {
    const unsigned slot = atomicAdd(big_count, 1u);          // slot < nf: every face is appended at most once
    big_list[slot] = (unsigned)f;
    return;
  }
  for (int pv = t.v0; pv <= t.v1; ++pv)
    for (int pu = t.u0; pu <= t.u1; ++pu) lvl_owner_pixel(t, pu, pv, c, prefix[ci], texels, (int)f, owner);
}

__global__ __launch_bounds__(256) void k_lvl_owner_large(const float* __restrict__ uv, const int* __restrict__ chart, long nf,
                                                         const int* __restrict__ charts, const long long* __restrict__ prefix, int nc,
                                                         long texels, int* __restrict__ owner, const unsigned* __restrict__ big_count,
                                                         const unsigned* __restrict__ big_list) {
  const unsigned n = *big_count;
  const int lane = threadIdx.x & 63;
  const unsigned waves = gridDim.x * (TEX_TILE / 64);
  for (unsigned e = blockIdx.x * (TEX_TILE / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    const long f = big_list[e];
    if (f >= nf) continue;
    const int ci = chart[f];
    if (ci < 0 || ci >= nc) continue;
    const int* c = charts + 8 * (long)ci;
    Tri t;
    if (!lvl_tri(uv + 6 * f, c, t)) continue;
    const int bw = t.u1 - t.u0 + 1;
    const long npx = (long)bw * (t.v1 - t.v0 + 1);
    for (long k = lane; k < npx; k += 64)
      lvl_owner_pixel(t, t.u0 + (int)(k % bw), t.v0 + (int)(k / bw), c, prefix[ci], texels, (int)f, owner);
  }
}

// The chart of texel t of the concatenated boxes: the last chart whose prefix is <= t (empty boxes share a prefix with the next)
__device__ __forceinline__ int lvl_chart_of(const long long* __restrict__ prefix, int nc, long t) {
  int lo = 0, hi = nc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_lvl_dilate(const int* __restrict__ charts, const long long* __restrict__ prefix, int nc,
                                                    const int* __restrict__ in, int* __restrict__ out) {
  const long t = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (t >= prefix[nc]) return;
  int o = in[t];
  if (o == INT_MAX) {
    const int ci = lvl_chart_of(prefix, nc, t);
    const int w = charts[8 * (long)ci + 2], h = charts[8 * (long)ci + 3];
    const long base = prefix[ci], local = t - base;
    const int dx = (int)(local % w), dy = (int)(local / w);
    for (int y = dy - 1; y <= dy + 1 && o == INT_MAX; ++y)
      for (int x = dx - 1; x <= dx + 1 && o == INT_MAX; ++x)
        if (x >= 0 && x < w && y >= 0 && y < h) o = in[base + (long)y * w + x];
  }
  out[t] = o;
}

__global__ __launch_bounds__(256) void k_lvl_apply(const float* __restrict__ uv, const int* __restrict__ corner_node, long nf,
                                                   const double* __restrict__ g, long n, const int* __restrict__ charts,
                                                   const long long* __restrict__ prefix, int nc, const int* __restrict__ owner, int P,
                                                   long pages, unsigned* __restrict__ atlas) {
  const long t = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (t >= prefix[nc]) return;
  const int o = owner[t];
  if (o == INT_MAX || o < 0 || o >= nf) return;
  const int ci = lvl_chart_of(prefix, nc, t);
  const int* c = charts + 8 * (long)ci;
  const long local = t - prefix[ci];
  const int dx = (int)(local % c[2]), dy = (int)(local / c[2]);
  const int ax = c[4] + dx, ay = c[5] + dy;
  if (ax < 0 || ay < 0 || ax >= P || ay >= P || c[6] < 0 || c[6] >= pages) return;
  const float* q = uv + 6 * (long)o;
  const int* cn = corner_node + 3 * (long)o;
  if (cn[0] < 0 || cn[1] < 0 || cn[2] < 0 || cn[0] >= n || cn[1] >= n || cn[2] >= n) return;
  const float x = (float)(c[0] + dx), y = (float)(c[1] + dy);
  const float area = (q[2] - q[0]) * (q[5] - q[1]) - (q[3] - q[1]) * (q[4] - q[0]);
  const float e1 = (q[0] - q[4]) * (y - q[5]) - (q[1] - q[5]) * (x - q[4]);
  const float e2 = (q[2] - q[0]) * (y - q[1]) - (q[3] - q[1]) * (x - q[0]);
  const float b1 = e1 / area, b2 = e2 / area;
  unsigned* px = atlas + ((long)c[6] * P + ay) * P + ax;
  const unsigned old = *px;
  unsigned out = old & 0xFF000000u;
  for (int ch = 0; ch < 3; ++ch) {
    const float g0 = (float)g[3 * (long)cn[0] + ch], g1 = (float)g[3 * (long)cn[1] + ch], g2 = (float)g[3 * (long)cn[2] + ch];
    float gi = g0 + b1 * (g1 - g0) + b2 * (g2 - g0);
    gi = fminf(fmaxf(gi, fminf(fminf(g0, g1), g2)), fmaxf(fmaxf(g0, g1), g2));
    const float v = fminf(fmaxf(floorf((float)((old >> (8 * ch)) & 255u) + gi + 0.5f), 0.f), 255.f);
    out |= (unsigned)v << (8 * ch);
  }
  *px = out;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
int launch_lvl_observe(const long long* view_tab, int nviews, const int* rowptr, const unsigned* col, long nnz, const int* node_view,
                       const float* pos, long n, float* f, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_lvl_observe, dim3(tiles256(n)), dim3(TEX_TILE), 0, st, view_tab, nviews, rowptr, col, nnz, node_view, pos, n, f);
  ADAMVS_CHECK_LAUNCH("texture_level_observe");
  return 0;
}

int launch_lvl_rhs(const int* rowptr, const unsigned* col, long nnz, const float* f, long n, double* b, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_lvl_rhs, dim3(tiles256(n)), dim3(TEX_TILE), 0, st, rowptr, col, nnz, f, n, b);
  ADAMVS_CHECK_LAUNCH("texture_level_rhs");
  return 0;
}

int launch_lvl_cg_init(const double* b, long n, double tol, double* g, double* r, double* p, double* partials, double* state,
                       hipStream_t st) {
  const int nb = lvl_grid(n);
  const long chunk = (n + nb - 1) / nb;
  hipLaunchKernelGGL(k_lvl_init, dim3(nb), dim3(TEX_TILE), 0, st, b, n, chunk, g, r, p, partials);
  ADAMVS_CHECK_LAUNCH("texture_level_init");
  hipLaunchKernelGGL(k_lvl_reduce_init, dim3(1), dim3(TEX_TILE), 0, st, (const double*)partials, nb, tol, state);
  ADAMVS_CHECK_LAUNCH("texture_level_reduce_init");
  return 0;
}

int launch_lvl_cg(const int* rowptr, const unsigned* col, long nnz, long n, double lambda, int count, double* g, double* r, double* p,
                  double* ap, double* partials, double* state, hipStream_t st) {
  const int nb = lvl_grid(n);
  const long chunk = (n + nb - 1) / nb;
  const double w_smooth = 1.0 / lambda;
  const long pairs = (3 * n + 1) / 2, pchunk = (pairs + nb - 1) / nb;
  for (int it = 0; it < count; ++it) {
    hipLaunchKernelGGL(k_lvl_spmv, dim3(nb), dim3(TEX_TILE), 0, st, rowptr, col, nnz, n, chunk, w_smooth, (const double*)p, ap, partials,
                       (const double*)state);
    hipLaunchKernelGGL(k_lvl_reduce_alpha, dim3(1), dim3(TEX_TILE), 0, st, (const double*)partials, nb, state);
    hipLaunchKernelGGL(k_lvl_update_xr, dim3(nb), dim3(TEX_TILE), 0, st, pairs, 3 * n, pchunk, (const double2*)p, (const double2*)ap,
                       (double2*)g, (double2*)r, partials, (const double*)state);
    hipLaunchKernelGGL(k_lvl_reduce_beta, dim3(1), dim3(TEX_TILE), 0, st, (const double*)partials, nb, state);
    hipLaunchKernelGGL(k_lvl_update_p, dim3(nb), dim3(TEX_TILE), 0, st, pairs, pchunk, (const double2*)r, (double2*)p,
                       (const double*)state);
    ADAMVS_CHECK_LAUNCH("texture_level_cg");
  }
  return 0;
}

int launch_lvl_owner(const float* uv, const int* chart, long nf, const int* charts, const long long* prefix, int nc, long texels,
                     int* owner, unsigned* big_count, unsigned* big_list, hipStream_t st) {
  if (texels == 0) return 0;
  hipLaunchKernelGGL(k_lvl_owner_clear, dim3(tiles256(texels)), dim3(TEX_TILE), 0, st, owner, texels);
  ADAMVS_CHECK_LAUNCH("texture_level_owner_clear");
  if (nf == 0 || nc == 0) return 0;
  hipError_t e = hipMemsetAsync(big_count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return set_error((int)e, "texture_level_owner: hipMemsetAsync: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_lvl_owner_small, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, uv, chart, nf, charts, prefix, nc, texels, owner,
                     big_count, big_list);
  ADAMVS_CHECK_LAUNCH("texture_level_owner_small");
  return launch_resident<k_lvl_owner_large>((nf + 3) / 4, 0, st, "texture_level_owner_large", uv, chart, nf, charts, prefix, nc, texels,
                                            owner, (const unsigned*)big_count, (const unsigned*)big_list);
}

int launch_lvl_dilate(const int* charts, const long long* prefix, int nc, long texels, const int* in, int* out, hipStream_t st) {
  if (texels == 0 || nc == 0) return 0;
  hipLaunchKernelGGL(k_lvl_dilate, dim3(tiles256(texels)), dim3(TEX_TILE), 0, st, charts, prefix, nc, in, out);
  ADAMVS_CHECK_LAUNCH("texture_level_dilate");
  return 0;
}

int launch_lvl_apply(const float* uv, const int* corner_node, long nf, const double* g, long n, const int* charts,
                     const long long* prefix, int nc, long texels, const int* owner, int P, long pages, unsigned char* atlas,
                     hipStream_t st) {
  if (texels == 0 || nc == 0 || nf == 0) return 0;
  hipLaunchKernelGGL(k_lvl_apply, dim3(tiles256(texels)), dim3(TEX_TILE), 0, st, uv, corner_node, nf, g, n, charts, prefix, nc, owner, P,
                     pages, (unsigned*)atlas);
  ADAMVS_CHECK_LAUNCH("texture_level_apply");
  return 0;
}

}  // namespace adamvs
