// Perspective projection and the inclusive z-buffer rasteriser shared by the image orthophoto (ortho.hip) and the mesh
// texture (texture.hip); include/adamvs_hip.h "Image orthophoto" states the arithmetic operation by operation, and both
// files keep it: no contraction into fma here either.
#pragma once
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace adamvs {

constexpr unsigned ZBUF_EMPTY = 0x7F800000u;     // +inf

struct ViewCam {
  double C[3];
  float R[9], Kc[6];            // R_cw, the first two rows of K
  int H, W;
};

static ViewCam view_cam(const adamvs_ortho_view& v) {
  ViewCam c;
  for (int k = 0; k < 3; ++k) c.C[k] = v.C[k];
  for (int k = 0; k < 9; ++k) c.R[k] = v.R[k];
  for (int k = 0; k < 6; ++k) c.Kc[k] = v.K[k];
  c.H = v.H;
  c.W = v.W;
  return c;
}

// World point (fp64) -> d = (float)(X - C), camera-frame p = R_cw d, pixel (u, v) and depth z (fp32).
struct Proj {
  float dx, dy, dz, u, v, z;
};

__device__ __forceinline__ Proj project(const ViewCam& c, double X, double Y, double Z) {
  Proj r;
  r.dx = (float)(X - c.C[0]);
  r.dy = (float)(Y - c.C[1]);
  r.dz = (float)(Z - c.C[2]);
  const float px = c.R[0] * r.dx + c.R[1] * r.dy + c.R[2] * r.dz;
  const float py = c.R[3] * r.dx + c.R[4] * r.dy + c.R[5] * r.dz;
  r.z = c.R[6] * r.dx + c.R[7] * r.dy + c.R[8] * r.dz;
  r.u = (c.Kc[0] * px + c.Kc[1] * py + c.Kc[2] * r.z) / r.z;
  r.v = (c.Kc[3] * px + c.Kc[4] * py + c.Kc[5] * r.z) / r.z;
  return r;
}

// One triangle in screen space, oriented (area > 0), with its clamped pixel box.
struct Tri {
  float u[3], v[3], iz[3], area;
  int u0, u1, v0, v1;       // inclusive pixel-centre box; empty if u0 > u1 or v0 > v1
};

// Vertex k of a triangle from its projection: false unless z > NEAR and u, v, z are finite.
__device__ __forceinline__ bool tri_vertex(float u, float v, float z, int k, Tri& t) {
  if (!(z > ORTHO_NEAR) || !isfinite(u) || !isfinite(v) || !isfinite(z)) return false;
  t.u[k] = u;
  t.v[k] = v;
  t.iz[k] = 1.f / z;
  return true;
}

// The set-up after three tri_vertex calls: orient (vertices 1 and 2 swap if the area is negative) and clamp the box of pixel
// centres to the W x H image.  False for a zero or non-finite area or an empty box.
__device__ __forceinline__ bool tri_setup(Tri& t, int W, int H) {
  float area = (t.u[1] - t.u[0]) * (t.v[2] - t.v[0]) - (t.v[1] - t.v[0]) * (t.u[2] - t.u[0]);
  if (!(area != 0.f) || !isfinite(area)) return false;
  if (area < 0.f) {
    float x = t.u[1]; t.u[1] = t.u[2]; t.u[2] = x;
    x = t.v[1]; t.v[1] = t.v[2]; t.v[2] = x;
    x = t.iz[1]; t.iz[1] = t.iz[2]; t.iz[2] = x;
    area = -area;
  }
  t.area = area;
  const float umn = fminf(fminf(t.u[0], t.u[1]), t.u[2]), umx = fmaxf(fmaxf(t.u[0], t.u[1]), t.u[2]);
  const float vmn = fminf(fminf(t.v[0], t.v[1]), t.v[2]), vmx = fmaxf(fmaxf(t.v[0], t.v[1]), t.v[2]);
  // clamp in float before the conversion: a vertex near the camera plane projects far outside the image
  t.u0 = (int)fminf(fmaxf(ceilf(umn), 0.f), (float)W);
  t.u1 = (int)fmaxf(fminf(floorf(umx), (float)(W - 1)), -1.f);
  t.v0 = (int)fminf(fmaxf(ceilf(vmn), 0.f), (float)H);
  t.v1 = (int)fmaxf(fminf(floorf(vmx), (float)(H - 1)), -1.f);
  return t.u0 <= t.u1 && t.v0 <= t.v1;
}

__device__ __forceinline__ void raster_pixel(const Tri& t, int pu, int pv, int W, unsigned* __restrict__ zbuf) {
  const float x = (float)pu, y = (float)pv;
  const float e0 = (t.u[2] - t.u[1]) * (y - t.v[1]) - (t.v[2] - t.v[1]) * (x - t.u[1]);
  const float e1 = (t.u[0] - t.u[2]) * (y - t.v[2]) - (t.v[0] - t.v[2]) * (x - t.u[2]);
  const float e2 = (t.u[1] - t.u[0]) * (y - t.v[0]) - (t.v[1] - t.v[0]) * (x - t.u[0]);
  if (!(e0 >= 0.f && e1 >= 0.f && e2 >= 0.f)) return;
  const float z = t.area / (e0 * t.iz[0] + e1 * t.iz[1] + e2 * t.iz[2]);
  if (!(z > 0.f) || !isfinite(z)) return;
  atomicMin(zbuf + (long)pv * W + pu, __float_as_uint(z));
}

}  // namespace adamvs
