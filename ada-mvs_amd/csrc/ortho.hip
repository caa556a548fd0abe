// Image orthophoto: the source images mosaicked over a DSM into a true orthophoto (the step after dsm_whu.py;
// include/adamvs_hip.h "Image orthophoto" states every operation).  Per scene, then per view in ascending image id:
//
//   k_ortho_surface      once: one lane per orthophoto cell, the height of the triangulated DSM at its centre (fp64)
//   k_ortho_zbuf_clear   per view: the depth buffer to +inf
//   k_ortho_zbuf_small   per view: one lane per DSM quad, its two triangles; a triangle whose pixel box holds at most
//                        ORTHO_SMALL_PX pixel centres is rasterised by the lane, a larger one is appended to a list
//   k_ortho_zbuf_large   per view: one wave per listed triangle, the lanes stride over its pixel box
//   k_ortho_compose      per view: one lane per cell, visibility against the depth buffer and the cell's state update (the
//                        visibility test and the bilinear sample are ortho_sample.h's, shared with ortho_balance.hip)
//   k_ortho_finalize     once: RGBA, chosen view and visible-view count
//
// The only atomics are the depth buffer's 32-bit unsigned min on the bits of positive floats (order-independent) and the
// large-triangle list counter (its order only decides which wave writes which min).  Every cell's state is owned by one lane
// across the views, so the output is bit-identical from run to run.
#include "common.h"
#include "kernels.h"
#include "persistent.h"
#include "ortho_sample.h"
#include "raster.h"

// The header states the arithmetic operation by operation: no contraction into fma in this file.
#pragma clang fp contract(off)

namespace adamvs {

static_assert(ORTHO_TILE == 256, "kernels below assume workgroups of four waves");

// ---- surface --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ortho_surface(const OrthoArgs a, const float* __restrict__ dsm, double* __restrict__ height) {
  const int Wo = a.W * a.K, Ho = a.H * a.K;
  const long n = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (n >= (long)Wo * Ho) return;
  const int i = (int)(n % Wo), j = (int)(n / Wo);
  double s = ((double)i + 0.5) / (double)a.K - 0.5, t = ((double)j + 0.5) / (double)a.K - 0.5;
  s = fmin(fmax(s, 0.0), (double)(a.W - 1));
  t = fmin(fmax(t, 0.0), (double)(a.H - 1));
  const int ia = (int)floor(s), ib = (int)floor(t);
  const double fs = s - (double)ia, ft = t - (double)ib;
  int va[3], vb[3];
  double w[3];
  va[0] = ia, vb[0] = ib, va[2] = ia + 1, vb[2] = ib + 1;
  if (fs >= ft) {
    va[1] = ia + 1, vb[1] = ib;
    w[0] = 1.0 - fs, w[1] = fs - ft, w[2] = ft;
  } else {
    va[1] = ia, vb[1] = ib + 1;
    w[0] = 1.0 - ft, w[1] = ft - fs, w[2] = fs;
  }
  double h = 0.0;
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    if (!(w[k] > 0.0)) continue;                       // a vertex of weight 0 is not read (it may lie past the grid)
    const float z = dsm[(long)vb[k] * a.W + va[k]];
    ok = ok && isfinite(z);
    h = h + w[k] * (double)z;
  }
  height[n] = ok ? h : __longlong_as_double(0x7FF8000000000000ll);
}

// ---- z-buffer -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ortho_zbuf_clear(unsigned* __restrict__ zbuf, long n) {
  const long k = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (k < n) zbuf[k] = ZBUF_EMPTY;
}

// Vertex q of triangle `half` of quad (qa, qb): half 0 = (a,b) (a+1,b) (a+1,b+1), half 1 = (a,b) (a,b+1) (a+1,b+1).
__device__ __forceinline__ bool setup_tri(const OrthoArgs& a, const ViewCam& c, const float* __restrict__ dsm, int qa, int qb,
                                          int half, Tri& t) {
  const int da[3] = {0, half == 0 ? 1 : 0, 1}, db[3] = {0, half == 0 ? 0 : 1, 1};
  for (int k = 0; k < 3; ++k) {
    const int va = qa + da[k], vb = qb + db[k];
    const float zw = dsm[(long)vb * a.W + va];
    if (!isfinite(zw)) return false;
    const Proj p = project(c, a.x0 + ((double)va + 0.5) * a.gsd, a.y_top - ((double)vb + 0.5) * a.gsd, (double)zw);
    if (!tri_vertex(p.u, p.v, p.z, k, t)) return false;
  }
  return tri_setup(t, c.W, c.H);
}

__global__ __launch_bounds__(256) void k_ortho_zbuf_small(const OrthoArgs a, const ViewCam c, const float* __restrict__ dsm,
                                                          unsigned* __restrict__ zbuf, unsigned* __restrict__ big_count,
                                                          unsigned* __restrict__ big_list) {
  const long nq = (long)(a.W - 1) * (a.H - 1);
  const long q = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (q >= nq) return;
  const int qa = (int)(q % (a.W - 1)), qb = (int)(q / (a.W - 1));
  for (int half = 0; half < 2; ++half) {
    Tri t;
    if (!setup_tri(a, c, dsm, qa, qb, half, t)) continue;
    const int bw = t.u1 - t.u0 + 1, bh = t.v1 - t.v0 + 1;
    if ((long)bw * bh > ORTHO_SMALL_PX) {
      const unsigned slot = atomicAdd(big_count, 1u);        // slot < 2 nq: every triangle is appended at most once
      big_list[slot] = (unsigned)(2 * q + half);
      continue;
    }
    for (int pv = t.v0; pv <= t.v1; ++pv)
      for (int pu = t.u0; pu <= t.u1; ++pu) raster_pixel(t, pu, pv, c.W, zbuf);
  }
}

__global__ __launch_bounds__(256) void k_ortho_zbuf_large(const OrthoArgs a, const ViewCam c, const float* __restrict__ dsm,
                                                          unsigned* __restrict__ zbuf, const unsigned* __restrict__ big_count,
                                                          const unsigned* __restrict__ big_list) {
  const unsigned n = *big_count;
  const int lane = threadIdx.x & 63;
  const unsigned waves = gridDim.x * (ORTHO_TILE / 64);
  for (unsigned e = blockIdx.x * (ORTHO_TILE / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    const unsigned id = big_list[e];
    const long q = (long)(id >> 1);
    Tri t;
    if (!setup_tri(a, c, dsm, (int)(q % (a.W - 1)), (int)(q / (a.W - 1)), (int)(id & 1u), t)) continue;
    const int bw = t.u1 - t.u0 + 1;
    const long npx = (long)bw * (t.v1 - t.v0 + 1);
    for (long k = lane; k < npx; k += 64) raster_pixel(t, t.u0 + (int)(k % bw), t.v0 + (int)(k / bw), c.W, zbuf);
  }
}

// ---- compose and finalize -------------------------------------------------------------------------------------------
template <bool FEATHER>
__global__ __launch_bounds__(256) void k_ortho_compose(const OrthoArgs a, const ViewCam c, const uint8_t* __restrict__ rgba, int view_id,
                                                       const double* __restrict__ height, const unsigned* __restrict__ zbuf, float border,
                                                       float feather_px, float tol, f32x4* __restrict__ acc, float* __restrict__ wmax,
                                                       int* __restrict__ view, int* __restrict__ nvis) {
  const int Wo = a.W * a.K, Ho = a.H * a.K;
  const long n = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (n >= (long)Wo * Ho) return;
  const double h = height[n];
  if (isnan(h)) return;
  const int i = (int)(n % Wo), j = (int)(n / Wo);
  const double g = a.gsd / (double)a.K;
  Proj p;
  if (!ortho_visible(c, zbuf, border, tol, a.x0 + ((double)i + 0.5) * g, a.y_top - ((double)j + 0.5) * g, h, p)) return;
  const float s = -p.dz / sqrtf(p.dx * p.dx + p.dy * p.dy + p.dz * p.dz);
  float col[3];
  ortho_bilinear(c, rgba, p, col);
  nvis[n] = nvis[n] + 1;
  if (FEATHER) {
    const float e = fminf(fminf(p.u, (float)(c.W - 1) - p.u), fminf(p.v, (float)(c.H - 1) - p.v));
    const float s2 = s * s;
    const float w = s2 * s2 * fminf(1.f, (e - border) / feather_px);
    f32x4 A = acc[n];
    A[0] = A[0] + w;
    A[1] = A[1] + w * col[0];
    A[2] = A[2] + w * col[1];
    A[3] = A[3] + w * col[2];
    acc[n] = A;
    if (w > wmax[n]) {
      wmax[n] = w;
      view[n] = view_id;
    }
  } else if (s > wmax[n]) {
    wmax[n] = s;
    view[n] = view_id;
    acc[n] = f32x4{1.f, col[0], col[1], col[2]};
  }
}

__global__ __launch_bounds__(256) void k_ortho_finalize(long ncell, const f32x4* __restrict__ acc, const int* __restrict__ view,
                                                        const int* __restrict__ nvis, unsigned* __restrict__ rgba_out,
                                                        int* __restrict__ view_out, uint16_t* __restrict__ nvis_out) {
  const long n = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (n >= ncell) return;
  const f32x4 A = acc[n];
  const int vw = view[n];
  unsigned px = 0u;
  if (vw >= 0 && A[0] > 0.f) {
    px = 255u << 24;
    for (int ch = 0; ch < 3; ++ch) {
      const float q = floorf(A[1 + ch] / A[0] + 0.5f);
      px |= (unsigned)fminf(fmaxf(q, 0.f), 255.f) << (8 * ch);
    }
  }
  rgba_out[n] = px;
  view_out[n] = px ? vw : -1;
  const int k = nvis[n];
  nvis_out[n] = (uint16_t)(k < 65535 ? k : 65535);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static unsigned ortho_blocks(long n) { return (unsigned)((n + ORTHO_TILE - 1) / ORTHO_TILE); }

int launch_ortho_surface(const adamvs_ortho_grid& g, const float* dsm, double* height, hipStream_t st) {
  const long n = (long)g.W * g.K * g.H * g.K;
  hipLaunchKernelGGL(k_ortho_surface, dim3(ortho_blocks(n)), dim3(ORTHO_TILE), 0, st, ortho_args(g), dsm, height);
  ADAMVS_CHECK_LAUNCH("ortho_surface");
  return 0;
}

int launch_ortho_zbuf(const adamvs_ortho_grid& g, const float* dsm, const adamvs_ortho_view& v, unsigned* zbuf, unsigned* big_count,
                      unsigned* big_list, hipStream_t st) {
  const OrthoArgs a = ortho_args(g);
  const ViewCam c = view_cam(v);
  const long npx = (long)v.W * v.H;
  hipLaunchKernelGGL(k_ortho_zbuf_clear, dim3(ortho_blocks(npx)), dim3(ORTHO_TILE), 0, st, zbuf, npx);
  ADAMVS_CHECK_LAUNCH("ortho_zbuf_clear");
  const long nq = (long)(g.W - 1) * (g.H - 1);
  if (nq == 0) return 0;
  hipError_t e = hipMemsetAsync(big_count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return set_error((int)e, "ortho_zbuf: hipMemsetAsync: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_ortho_zbuf_small, dim3(ortho_blocks(nq)), dim3(ORTHO_TILE), 0, st, a, c, dsm, zbuf, big_count, big_list);
  ADAMVS_CHECK_LAUNCH("ortho_zbuf_small");
  // the list length is known on the device only: a resident grid strides over it, one wave per triangle
  return launch_resident<k_ortho_zbuf_large>((nq * 2 + 3) / 4, 0, st, "ortho_zbuf_large", a, c, dsm, zbuf, (const unsigned*)big_count,
                                             (const unsigned*)big_list);
}

int launch_ortho_compose(const adamvs_ortho_grid& g, const adamvs_ortho_view& v, int view_id, const double* height, const unsigned* zbuf,
                         int mode, float border, float feather_px, float tol, float* acc, float* wmax, int* view, int* nvis, hipStream_t st) {
  const long n = (long)g.W * g.K * g.H * g.K;
  if (mode == ADAMVS_ORTHO_FEATHER)
    hipLaunchKernelGGL(k_ortho_compose<true>, dim3(ortho_blocks(n)), dim3(ORTHO_TILE), 0, st, ortho_args(g), view_cam(v), v.rgba,
                       view_id, height, zbuf, border, feather_px, tol, (f32x4*)acc, wmax, view, nvis);
  else
    hipLaunchKernelGGL(k_ortho_compose<false>, dim3(ortho_blocks(n)), dim3(ORTHO_TILE), 0, st, ortho_args(g), view_cam(v), v.rgba,
                       view_id, height, zbuf, border, feather_px, tol, (f32x4*)acc, wmax, view, nvis);
  ADAMVS_CHECK_LAUNCH("ortho_compose");
  return 0;
}

int launch_ortho_finalize(const adamvs_ortho_grid& g, const float* acc, const int* view, const int* nvis, uint8_t* rgba, int* view_out,
                          uint16_t* nvis_out, hipStream_t st) {
  const long n = (long)g.W * g.K * g.H * g.K;
  hipLaunchKernelGGL(k_ortho_finalize, dim3(ortho_blocks(n)), dim3(ORTHO_TILE), 0, st, n, (const f32x4*)acc, view, nvis, (unsigned*)rgba,
                     view_out, nvis_out);
  ADAMVS_CHECK_LAUNCH("ortho_finalize");
  return 0;
}

}  // namespace adamvs
