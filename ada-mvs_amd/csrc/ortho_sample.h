// The sample of one surface point in one view, shared by the mosaic (ortho.hip, k_ortho_compose) and the radiometric balance
// (ortho_balance.hip, k_ortho_observe): projection, the visibility rule and the bilinear colour exactly as include/adamvs_hip.h
// "Image orthophoto" states them, operation by operation: no contraction into fma here either.
#pragma once
#include "common.h"
#include "kernels.h"
#include "raster.h"

#pragma clang fp contract(off)

namespace adamvs {

struct OrthoArgs {
  double x0, y_top, gsd;        // the DSM grid
  int W, H, K;                  // DSM cells, upsample
};

static OrthoArgs ortho_args(const adamvs_ortho_grid& g) { return OrthoArgs{g.x0, g.y_top, g.gsd, g.W, g.H, g.K}; }

// Whether the world point (X, Y, h) (h not NaN) is visible in the view: in front, inside the border, and not behind the depth
// buffer by more than tol.  p is its projection (set in every case).
__device__ __forceinline__ bool ortho_visible(const ViewCam& c, const unsigned* __restrict__ zbuf, float border, float tol, double X,
                                              double Y, double h, Proj& p) {
  p = project(c, X, Y, h);
  if (!(p.z > 0.f)) return false;
  const float umax = (float)(c.W - 1) - border, vmax = (float)(c.H - 1) - border;
  if (!(p.u >= border && p.u <= umax && p.v >= border && p.v <= vmax)) return false;       // NaN fails too
  const int pu = (int)floorf(p.u + 0.5f), pv = (int)floorf(p.v + 0.5f);
  const float zb = __uint_as_float(zbuf[(long)pv * c.W + pu]);
  return p.z <= zb + tol;
}

// The bilinear sample of the image at the projection of a visible point.
__device__ __forceinline__ void ortho_bilinear(const ViewCam& c, const uint8_t* __restrict__ rgba, const Proj& p, float col[3]) {
  const int xa = (int)floorf(p.u), ya = (int)floorf(p.v);
  const float fx = p.u - (float)xa, fy = p.v - (float)ya;
  const int xb = xa + 1 < c.W ? xa + 1 : c.W - 1, yb = ya + 1 < c.H ? ya + 1 : c.H - 1;
  const unsigned p00 = *(const unsigned*)(rgba + 4 * ((long)ya * c.W + xa)), p10 = *(const unsigned*)(rgba + 4 * ((long)ya * c.W + xb));
  const unsigned p01 = *(const unsigned*)(rgba + 4 * ((long)yb * c.W + xa)), p11 = *(const unsigned*)(rgba + 4 * ((long)yb * c.W + xb));
  for (int ch = 0; ch < 3; ++ch) {
    const float c00 = (float)((p00 >> (8 * ch)) & 255u), c10 = (float)((p10 >> (8 * ch)) & 255u);
    const float c01 = (float)((p01 >> (8 * ch)) & 255u), c11 = (float)((p11 >> (8 * ch)) & 255u);
    col[ch] = (1.f - fy) * ((1.f - fx) * c00 + fx * c10) + fy * ((1.f - fx) * c01 + fx * c11);
  }
}

}  // namespace adamvs
