// Mesh texture: a triangle mesh labelled face by face with the source view that sees it best, grouped into charts, and the
// charts' image boxes copied into atlas pages (the step after mesh_whu.py; include/adamvs_hip.h "Mesh texturing" states
// every operation).  Per view in ascending image id:
//
//   k_tex_project       one lane per vertex: (u, v, z) in fp32 (raster.h project)
//   k_tex_zbuf_clear    the depth buffer to +inf
//   k_tex_zbuf_small    one lane per face; a face whose pixel box holds more than ORTHO_SMALL_PX centres goes to a list
//   k_tex_zbuf_large    one wave per listed face on a resident grid
//   k_tex_score         one lane per face: visibility against the depth buffer and the face's state update
//
// then once:
//
//   (k_mesh_edge_keys of mesh_smooth.hip: 3 F keys min(a, b) << 32 | max(a, b); the host sorts them by key, then label, then entry)
//   k_tex_hook          one lane per sorted entry: two neighbours with the same key and label hook their roots
//   k_tex_compress      one lane per face: the walk to the root (block_prims.h compress_to_root; each lane writes its own entry only)
//   k_tex_count         per workgroup: chart roots and untextured faces
//   k_tex_rank          chart id of every root and palette index of every untextured face (ballot / mbcnt + a scan)
//   k_tex_boxes         one lane per textured face: its chart id and the chart's integer pixel box (atomic min / max)
//   k_tex_fill          per view: one lane per texel of the view's chart boxes, a copy of the image texel
//   k_tex_coords        one lane per face: texture coordinates and page; an untextured face writes its palette texel
//
// Atomics: the depth buffer's unsigned min on positive float bits and the integer box min / max (order-independent), the
// large-face list counter (decides only which wave writes which min) and the hook's min on a parent (the result of a round
// may depend on the order, the fixed point does not: every chart's root is its smallest face).  Everything else is owned by
// one lane, so the outputs are bit-identical from run to run.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "persistent.h"
#include "raster.h"

#include <climits>

#pragma clang fp contract(off)

namespace adamvs {

// ---- labelling ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tex_project(const ViewCam c, const double* __restrict__ xyz, long nv, f32x4* __restrict__ uvz) {
  const long i = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (i >= nv) return;
  const Proj p = project(c, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
  uvz[i] = f32x4{p.u, p.v, p.z, 0.f};
}

__global__ __launch_bounds__(256) void k_tex_zbuf_clear(unsigned* __restrict__ zbuf, long n) {
  const long k = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (k < n) zbuf[k] = ZBUF_EMPTY;
}

// Face f's three projected vertices -> false if an index is out of range (the face is then ignored everywhere)
__device__ __forceinline__ bool face_verts(const f32x4* __restrict__ uvz, long nv, const unsigned* __restrict__ faces, long f, f32x4 p[3]) {
  for (int k = 0; k < 3; ++k) {
    const unsigned i = faces[3 * f + k];
    if ((long)i >= nv) return false;
    p[k] = uvz[i];
  }
  return true;
}

__device__ __forceinline__ bool face_tri(const f32x4* __restrict__ uvz, long nv, const unsigned* __restrict__ faces, long f, int W, int H,
                                         Tri& t) {
  f32x4 p[3];
  if (!face_verts(uvz, nv, faces, f, p)) return false;
  for (int k = 0; k < 3; ++k)
    if (!tri_vertex(p[k][0], p[k][1], p[k][2], k, t)) return false;
  return tri_setup(t, W, H);
}

__global__ __launch_bounds__(256) void k_tex_zbuf_small(int W, int H, const f32x4* __restrict__ uvz, long nv, const unsigned* __restrict__ faces,
                                                        long nf, unsigned* __restrict__ zbuf, unsigned* __restrict__ big_count,
                                                        unsigned* __restrict__ big_list) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (f >= nf) return;
  Tri t;
  if (!face_tri(uvz, nv, faces, f, W, H, t)) return;
  const int bw = t.u1 - t.u0 + 1, bh = t.v1 - t.v0 + 1;
  if ((long)bw * bh > ORTHO_SMALL_PX) {
    const unsigned slot = atomicAdd(big_count, 1u);          // slot < nf: every face is appended at most once
    big_list[slot] = (unsigned)f;
    return;
  }
  for (int pv = t.v0; pv <= t.v1; ++pv)
    for (int pu = t.u0; pu <= t.u1; ++pu) raster_pixel(t, pu, pv, W, zbuf);
}

__global__ __launch_bounds__(256) void k_tex_zbuf_large(int W, int H, const f32x4* __restrict__ uvz, long nv, const unsigned* __restrict__ faces,
                                                        unsigned* __restrict__ zbuf, const unsigned* __restrict__ big_count,
                                                        const unsigned* __restrict__ big_list) {
  const unsigned n = *big_count;
  const int lane = threadIdx.x & 63;
  const unsigned waves = gridDim.x * (TEX_TILE / 64);
  for (unsigned e = blockIdx.x * (TEX_TILE / 64) + (threadIdx.x >> 6); e < n; e += waves) {
    Tri t;
    if (!face_tri(uvz, nv, faces, (long)big_list[e], W, H, t)) continue;
    const int bw = t.u1 - t.u0 + 1;
    const long npx = (long)bw * (t.v1 - t.v0 + 1);
    for (long k = lane; k < npx; k += 64) raster_pixel(t, t.u0 + (int)(k % bw), t.v0 + (int)(k / bw), W, zbuf);
  }
}

__device__ __forceinline__ bool depth_ok(const unsigned* __restrict__ zbuf, int W, float u, float v, float z, float tol) {
  const int pu = (int)floorf(u + 0.5f), pv = (int)floorf(v + 0.5f);
  return z <= __uint_as_float(zbuf[(long)pv * W + pu]) + tol;
}

__global__ __launch_bounds__(256) void k_tex_score(int W, int H, int view, const f32x4* __restrict__ uvz, long nv,
                                                   const unsigned* __restrict__ faces, long nf, const unsigned* __restrict__ zbuf, float border,
                                                   float tol, float* __restrict__ best, int* __restrict__ label, int* __restrict__ nvis,
                                                   float* __restrict__ uv) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (f >= nf) return;
  f32x4 p[3];
  if (!face_verts(uvz, nv, faces, f, p)) return;
  const float umax = (float)(W - 1) - border, vmax = (float)(H - 1) - border;
  for (int k = 0; k < 3; ++k) {
    if (!(p[k][2] > ORTHO_NEAR)) return;
    if (!(p[k][0] >= border && p[k][0] <= umax && p[k][1] >= border && p[k][1] <= vmax)) return;     // NaN fails too
  }
  // front-facing: negative signed area in the image (y down), taken before any swap
  const float area = (p[1][0] - p[0][0]) * (p[2][1] - p[0][1]) - (p[1][1] - p[0][1]) * (p[2][0] - p[0][0]);
  if (!(area < 0.f)) return;
  for (int k = 0; k < 3; ++k)
    if (!depth_ok(zbuf, W, p[k][0], p[k][1], p[k][2], tol)) return;
  const float uc = (p[0][0] + p[1][0] + p[2][0]) / 3.f, vc = (p[0][1] + p[1][1] + p[2][1]) / 3.f;
  const float zc = 3.f / (1.f / p[0][2] + 1.f / p[1][2] + 1.f / p[2][2]);
  if (!depth_ok(zbuf, W, uc, vc, zc, tol)) return;
  const float score = -area * 0.5f;
  nvis[f] = nvis[f] + 1;
  if (score > best[f]) {
    best[f] = score;
    label[f] = view;
    for (int k = 0; k < 3; ++k) {
      uv[6 * f + 2 * k] = p[k][0];
      uv[6 * f + 2 * k + 1] = p[k][1];
    }
  }
}

// ---- charts ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tex_hook(const long long* __restrict__ keys, const long long* __restrict__ entry, long n,
                                                  const int* __restrict__ label, int* parent, unsigned* __restrict__ changed) {
  const long i = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (i + 1 >= n || keys[i] != keys[i + 1]) return;
  const int a = (int)(entry[i] / 3), b = (int)(entry[i + 1] / 3);
  const int la = label[a];
  if (la < 0 || la != label[b]) return;
  const int ra = parent[a], rb = parent[b];
  if (ra == rb) return;
  atomicMin(parent + (ra > rb ? ra : rb), ra < rb ? ra : rb);
  changed[0] = 1u;
}

__global__ __launch_bounds__(256) void k_tex_compress(int* parent, long nf) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (f < nf) compress_to_root(parent, f);
}

__global__ __launch_bounds__(256) void k_tex_count(const int* __restrict__ label, const int* __restrict__ parent, long nf,
                                                   unsigned* __restrict__ block_roots, unsigned* __restrict__ block_untex) {
  __shared__ unsigned wr[4], wu[4];
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  const int l = f < nf ? label[f] : -2;
  const bool root = l >= 0 && parent[f] == (int)f, untex = l == -1;
  const unsigned long long br = __ballot(root), bu = __ballot(untex);
  if ((threadIdx.x & 63) == 0) {
    wr[threadIdx.x >> 6] = (unsigned)__popcll(br);
    wu[threadIdx.x >> 6] = (unsigned)__popcll(bu);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    block_roots[blockIdx.x] = wr[0] + wr[1] + wr[2] + wr[3];
    block_untex[blockIdx.x] = wu[0] + wu[1] + wu[2] + wu[3];
  }
}

__global__ __launch_bounds__(256) void k_tex_rank(const int* __restrict__ label, const int* __restrict__ parent, long nf,
                                                  const unsigned* __restrict__ root_off, const unsigned* __restrict__ untex_off,
                                                  int* __restrict__ root_chart, int* __restrict__ pal) {
  __shared__ unsigned wr[4], wu[4];
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  const int l = f < nf ? label[f] : -2;
  const bool root = l >= 0 && parent[f] == (int)f, untex = l == -1;
  const unsigned long long br = __ballot(root), bu = __ballot(untex);
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    wr[wv] = (unsigned)__popcll(br);
    wu[wv] = (unsigned)__popcll(bu);
  }
  __syncthreads();
  if (f >= nf) return;
  unsigned r = root_off[blockIdx.x] + lane_rank(br), u = untex_off[blockIdx.x] + lane_rank(bu);
  for (int k = 0; k < wv; ++k) {
    r += wr[k];
    u += wu[k];
  }
  root_chart[f] = root ? (int)r : -1;
  pal[f] = untex ? (int)u : -1;
}

// Neighbouring faces mostly share a chart, and a large chart's four box words would serialise every lane's atomics: the lanes
// of a wave that share the chart of the first remaining lane reduce their extremes first and one of them issues the atomics.
__global__ __launch_bounds__(256) void k_tex_boxes(const int* __restrict__ label, const int* __restrict__ parent,
                                                   const int* __restrict__ root_chart, const float* __restrict__ uv, long nf,
                                                   int* __restrict__ chart, int* __restrict__ box) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  const int lane = threadIdx.x & 63;
  bool todo = false;
  int c = -1, e[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};      // min floor u, min floor v, -max floor u, -max floor v
  if (f < nf) {
    if (label[f] >= 0) {
      c = root_chart[parent[f]];
      const float* q = uv + 6 * f;
      e[0] = (int)floorf(fminf(fminf(q[0], q[2]), q[4]));
      e[1] = (int)floorf(fminf(fminf(q[1], q[3]), q[5]));
      e[2] = -(int)floorf(fmaxf(fmaxf(q[0], q[2]), q[4]));
      e[3] = -(int)floorf(fmaxf(fmaxf(q[1], q[3]), q[5]));
      todo = true;
    }
    chart[f] = c;
  }
  for (unsigned long long live = __ballot(todo); live; live = __ballot(todo)) {
    const int lead = __ffsll((unsigned long long)live) - 1;
    const int c0 = __shfl(c, lead);
    const bool mine = todo && c == c0;
    int r[4];
    for (int k = 0; k < 4; ++k) r[k] = wave_min(mine ? e[k] : INT_MAX);
    if (lane == lead) {
      int* bx = box + 4 * (long)c0;
      atomicMin(bx, r[0]);
      atomicMin(bx + 1, r[1]);
      atomicMax(bx + 2, -r[2]);
      atomicMax(bx + 3, -r[3]);
    }
    todo = todo && !mine;
  }
}

// ---- atlas ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tex_fill(const unsigned* __restrict__ rgba, int W, int H, const int* __restrict__ items,
                                                  const long long* __restrict__ prefix, int n, int P, long pages, unsigned* __restrict__ atlas) {
  const long t = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (t >= prefix[n]) return;
  int lo = 0, hi = n - 1;                  // the last item whose prefix is <= t (empty items share a prefix with the next)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (prefix[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  const int* it = items + 8 * (long)lo;    // x0, y0, w, h, ox, oy, page, -
  const long local = t - prefix[lo];
  const int dx = (int)(local % it[2]), dy = (int)(local / it[2]);
  const int x = it[0] + dx, y = it[1] + dy, ax = it[4] + dx, ay = it[5] + dy;
  if (x >= W || y >= H || ax >= P || ay >= P || it[6] >= pages) return;     // the host's placement is checked; this only guards
  atlas[((long)it[6] * P + ay) * P + ax] = rgba[(long)y * W + x] & 0x00FFFFFFu;
}

// charts: [nc][8] = x0, y0, w, h, ox, oy, page, view; the palette block at (pal_ox, pal_oy) of page pal_page
__global__ __launch_bounds__(256) void k_tex_coords(const int* __restrict__ label, const int* __restrict__ chart, const int* __restrict__ pal,
                                                    const float* __restrict__ uv, long nf, const int* __restrict__ charts, int pal_ox,
                                                    int pal_oy, int pal_page, int P, long pages, const unsigned* __restrict__ faces, long nv,
                                                    const uint8_t* __restrict__ vrgb, unsigned* __restrict__ atlas, float* __restrict__ tc,
                                                    int* __restrict__ texnum) {
  const long f = (long)blockIdx.x * TEX_TILE + threadIdx.x;
  if (f >= nf) return;
  const float fP = (float)P;
  float* o = tc + 6 * f;
  if (label[f] >= 0) {
    const int* c = charts + 8 * (long)chart[f];
    const float x0 = (float)c[0], y0 = (float)c[1], ox = (float)c[4], oy = (float)c[5];
    for (int k = 0; k < 3; ++k) {
      o[2 * k] = (ox + (uv[6 * f + 2 * k] - x0) + 0.5f) / fP;
      o[2 * k + 1] = 1.f - (oy + (uv[6 * f + 2 * k + 1] - y0) + 0.5f) / fP;
    }
    texnum[f] = c[6];
    return;
  }
  const int k = pal[f];
  const int tx = pal_ox + k % P, ty = pal_oy + k / P;
  const float s = ((float)tx + 0.5f) / fP, t = 1.f - ((float)ty + 0.5f) / fP;
  for (int j = 0; j < 3; ++j) {
    o[2 * j] = s;
    o[2 * j + 1] = t;
  }
  texnum[f] = pal_page;
  unsigned sum[3] = {0u, 0u, 0u};
  for (int j = 0; j < 3; ++j) {
    const unsigned i = faces[3 * f + j];
    if ((long)i >= nv) continue;
    for (int ch = 0; ch < 3; ++ch) sum[ch] += vrgb[3 * (long)i + ch];
  }
  if (k < 0 || tx >= P || ty >= P || pal_page >= pages) return;
  // the rounded mean: floor(s / 3 + 1/2) = (s + 1) / 3 in integers (s / 3 is never halfway)
  atlas[((long)pal_page * P + ty) * P + tx] = (sum[0] + 1u) / 3u | ((sum[1] + 1u) / 3u) << 8 | ((sum[2] + 1u) / 3u) << 16;
}

// ---- launchers ------------------------------------------------------------------------------------------------------
int launch_tex_project(const adamvs_ortho_view& v, const double* xyz, long nv, float* uvz, hipStream_t st) {
  if (nv == 0) return 0;
  hipLaunchKernelGGL(k_tex_project, dim3(tiles256(nv)), dim3(TEX_TILE), 0, st, view_cam(v), xyz, nv, (f32x4*)uvz);
  ADAMVS_CHECK_LAUNCH("texture_project");
  return 0;
}

int launch_tex_zbuf(int W, int H, const float* uvz, long nv, const unsigned* faces, long nf, unsigned* zbuf, unsigned* big_count,
                    unsigned* big_list, hipStream_t st) {
  const long npx = (long)W * H;
  hipLaunchKernelGGL(k_tex_zbuf_clear, dim3(tiles256(npx)), dim3(TEX_TILE), 0, st, zbuf, npx);
  ADAMVS_CHECK_LAUNCH("texture_zbuf_clear");
  if (nf == 0) return 0;
  hipError_t e = hipMemsetAsync(big_count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return set_error((int)e, "texture_zbuf: hipMemsetAsync: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_tex_zbuf_small, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, W, H, (const f32x4*)uvz, nv, faces, nf, zbuf, big_count,
                     big_list);
  ADAMVS_CHECK_LAUNCH("texture_zbuf_small");
  // the list length is known on the device only: a resident grid strides over it, one wave per face
  return launch_resident<k_tex_zbuf_large>((nf + 3) / 4, 0, st, "texture_zbuf_large", W, H, (const f32x4*)uvz, nv, faces, zbuf,
                                           (const unsigned*)big_count, (const unsigned*)big_list);
}

int launch_tex_score(int W, int H, int view, const float* uvz, long nv, const unsigned* faces, long nf, const unsigned* zbuf, float border,
                     float tol, float* best, int* label, int* nvis, float* uv, hipStream_t st) {
  if (nf == 0) return 0;
  hipLaunchKernelGGL(k_tex_score, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, W, H, view, (const f32x4*)uvz, nv, faces, nf, zbuf, border, tol,
                     best, label, nvis, uv);
  ADAMVS_CHECK_LAUNCH("texture_score");
  return 0;
}

int launch_tex_components_round(const long long* keys, const long long* entry, long n, const int* label, int* parent, long nf,
                                unsigned* changed, hipStream_t st) {
  hipError_t e = hipMemsetAsync(changed, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return set_error((int)e, "texture_components: hipMemsetAsync: %s", hipGetErrorString(e));
  if (n > 1) {
    hipLaunchKernelGGL(k_tex_hook, dim3(tiles256(n - 1)), dim3(TEX_TILE), 0, st, keys, entry, n, label, parent, changed);
    ADAMVS_CHECK_LAUNCH("texture_hook");
  }
  if (nf > 0) {
    hipLaunchKernelGGL(k_tex_compress, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, parent, nf);
    ADAMVS_CHECK_LAUNCH("texture_compress");
  }
  return 0;
}

int launch_tex_rank(const int* label, const int* parent, long nf, unsigned* block_roots, unsigned* block_untex, unsigned* root_off,
                    unsigned* untex_off, int* root_chart, int* pal, hipStream_t st) {
  if (nf == 0) return 0;
  const int nb = (int)tiles256(nf);
  hipLaunchKernelGGL(k_tex_count, dim3(nb), dim3(TEX_TILE), 0, st, label, parent, nf, block_roots, block_untex);
  ADAMVS_CHECK_LAUNCH("texture_count");
  if (int rc = launch_fusion_scan(block_roots, root_off, nb, st)) return rc;
  if (int rc = launch_fusion_scan(block_untex, untex_off, nb, st)) return rc;
  hipLaunchKernelGGL(k_tex_rank, dim3(nb), dim3(TEX_TILE), 0, st, label, parent, nf, (const unsigned*)root_off, (const unsigned*)untex_off,
                     root_chart, pal);
  ADAMVS_CHECK_LAUNCH("texture_rank");
  return 0;
}

int launch_tex_boxes(const int* label, const int* parent, const int* root_chart, const float* uv, long nf, int* chart, int* box,
                     hipStream_t st) {
  if (nf == 0) return 0;
  hipLaunchKernelGGL(k_tex_boxes, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, label, parent, root_chart, uv, nf, chart, box);
  ADAMVS_CHECK_LAUNCH("texture_boxes");
  return 0;
}

int launch_tex_fill(const adamvs_ortho_view& v, const int* items, const long long* prefix, int n, long texels, int P, long pages,
                    unsigned char* atlas, hipStream_t st) {
  if (n == 0 || texels == 0) return 0;
  hipLaunchKernelGGL(k_tex_fill, dim3(tiles256(texels)), dim3(TEX_TILE), 0, st, (const unsigned*)v.rgba, v.W, v.H, items, prefix, n, P,
                     pages, (unsigned*)atlas);
  ADAMVS_CHECK_LAUNCH("texture_fill");
  return 0;
}

int launch_tex_coords(const int* label, const int* chart, const int* pal, const float* uv, long nf, const int* charts, int pal_ox,
                      int pal_oy, int pal_page, int P, long pages, const unsigned* faces, long nv, const unsigned char* vrgb,
                      unsigned char* atlas, float* tc, int* texnum, hipStream_t st) {
  if (nf == 0) return 0;
  hipLaunchKernelGGL(k_tex_coords, dim3(tiles256(nf)), dim3(TEX_TILE), 0, st, label, chart, pal, uv, nf, charts, pal_ox, pal_oy, pal_page,
                     P, pages, faces, nv, vrgb, (unsigned*)atlas, tc, texnum);
  ADAMVS_CHECK_LAUNCH("texture_coords");
  return 0;
}

}  // namespace adamvs
