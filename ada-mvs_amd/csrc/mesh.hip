// TSDF integration of depth maps and marching-tetrahedra extraction of its zero level set, brick by brick (the step after
// fuse_whu.py; include/adamvs_hip.h "TSDF mesh" states every operation).  Per brick:
//
//   k_tsdf_integrate       one lane per sample, the brick's view list in order: project, nearest-pixel depth, truncated sdf,
//                          colour sums; weight and colour are integers, the tsdf an fp32 sum in list order
//   k_mesh_classify        one lane per cube: processed bit, the six tet cases, triangles per cube and per workgroup
//   k_mesh_count_vertices  one lane per sample: which of its 7 positive edges carry a vertex, vertices per workgroup
//   (k_fusion_scan twice: the workgroup offsets of vertices and triangles)
//   k_mesh_emit_vertices   each sample's vertices at  block offset + rank in the block  (fp64 positions, rgb)
//   k_mesh_emit_triangles  each cube's triangles at  block offset + rank in the block  (uint32 indices)
//
// Workgroups cover MESH_TILE consecutive entries of the row-major sample / cube order, so block order is output order.  No
// atomics and no inter-workgroup waits: the launches are the synchronisation, and the output is bit-identical from run to run.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

// The header states the vertex position and colour as separate roundings: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace adamvs {

// ---- the Kuhn split, generated from the rule of the header --------------------------------------------------------------
// Tet t is the axis permutation PERM[t] = (a, b, c); vertices v0 = 000, v1 = e_a, v2 = e_a + e_b, v3 = 111, as corner bits
// (x = 1, y = 2, z = 4).  Tet edge k joins EDGE_PAIR[k]; every one runs in a positive lattice direction from its lower end.
constexpr int PERM[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
constexpr int EDGE_PAIR[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// lattice directions 0 +x, 1 +y, 2 +z, 3 +xy, 4 +xz, 5 +yz, 6 +xyz, as corner bits
constexpr int DIR_BITS[7] = {1, 2, 4, 3, 5, 6, 7};

struct TetTable {
  int vert[6][4];            // corner bits of v0 .. v3
  int edge_start[6][6];      // tet edge k of tet t: corner bits of its lower end ...
  int edge_dir[6][6];        // ... and its direction
  int ntri[16];              // triangles of a case (the same for every tet)
  int tri[6][16][2][3];      // tet edges of each triangle, oriented
  int users[7][6];           // corners s from which a cube uses the edge of direction e: the cube of sample g is g - s
  int nusers[7];
};

constexpr int dir_of(int bits) {
  int d = -1;
  for (int e = 0; e < 7; ++e)
    if (DIR_BITS[e] == bits) d = e;
  return d;
}

// doubled coordinates of the midpoint of tet edge (i, j): v_i + v_j per axis
constexpr int mid(const int* vert, int i, int j, int axis) { return ((vert[i] >> axis) & 1) + ((vert[j] >> axis) & 1); }

constexpr TetTable make_tet_table() {
  TetTable T{};
  for (int t = 0; t < 6; ++t) {
    const int a = 1 << PERM[t][0], b = 1 << PERM[t][1];
    T.vert[t][0] = 0;
    T.vert[t][1] = a;
    T.vert[t][2] = a | b;
    T.vert[t][3] = 7;
    for (int k = 0; k < 6; ++k) {
      const int lo = T.vert[t][EDGE_PAIR[k][0]], hi = T.vert[t][EDGE_PAIR[k][1]];
      T.edge_start[t][k] = lo;
      T.edge_dir[t][k] = dir_of(hi & ~lo);
    }
  }
  for (int e = 0; e < 7; ++e) T.nusers[e] = 0;
  for (int t = 0; t < 6; ++t)
    for (int k = 0; k < 6; ++k) {
      const int e = T.edge_dir[t][k], s = T.edge_start[t][k];
      bool seen = false;
      for (int u = 0; u < T.nusers[e]; ++u) seen = seen || T.users[e][u] == s;
      if (!seen) T.users[e][T.nusers[e]++] = s;
    }
  for (int c = 0; c < 16; ++c) {
    int nin = 0;
    for (int k = 0; k < 4; ++k) nin += (c >> k) & 1;
    T.ntri[c] = (nin == 0 || nin == 4) ? 0 : (nin == 2 ? 2 : 1);
  }
  auto edge_index = [](int i, int j) {
    int r = -1;
    for (int k = 0; k < 6; ++k)
      if ((EDGE_PAIR[k][0] == i && EDGE_PAIR[k][1] == j) || (EDGE_PAIR[k][0] == j && EDGE_PAIR[k][1] == i)) r = k;
    return r;
  };
  for (int t = 0; t < 6; ++t)
    for (int c = 0; c < 16; ++c) {
      int in[4] = {}, out[4] = {}, nin = 0, nout = 0;
      for (int k = 0; k < 4; ++k) {
        if ((c >> k) & 1) in[nin++] = k;
        else out[nout++] = k;
      }
      int tris[2][3] = {};
      if (nin == 1 || nin == 3) {
        const int lone = nin == 1 ? in[0] : out[0];
        int n = 0;
        for (int k = 0; k < 4; ++k)
          if (k != lone) tris[0][n++] = edge_index(lone, k);
      } else if (nin == 2) {
        const int q0 = edge_index(in[0], out[0]), q1 = edge_index(in[0], out[1]), q2 = edge_index(in[1], out[1]),
                  q3 = edge_index(in[1], out[0]);
        tris[0][0] = q0, tris[0][1] = q1, tris[0][2] = q2;
        tris[1][0] = q0, tris[1][1] = q2, tris[1][2] = q3;
      }
      // orientation: the normal at the edge midpoints against nin * sum(outside) - nout * sum(inside)  (centroid difference)
      for (int r = 0; r < T.ntri[c]; ++r) {
        int P[3][3] = {};
        for (int m = 0; m < 3; ++m)
          for (int ax = 0; ax < 3; ++ax)
            P[m][ax] = mid(T.vert[t], EDGE_PAIR[tris[r][m]][0], EDGE_PAIR[tris[r][m]][1], ax);
        const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
        const int w[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
        const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
        int D[3] = {};
        for (int ax = 0; ax < 3; ++ax) {
          int so = 0, si = 0;
          for (int k = 0; k < nout; ++k) so += (T.vert[t][out[k]] >> ax) & 1;
          for (int k = 0; k < nin; ++k) si += (T.vert[t][in[k]] >> ax) & 1;
          D[ax] = nin * so - nout * si;
        }
        const int dot = n[0] * D[0] + n[1] * D[1] + n[2] * D[2];
        T.tri[t][c][r][0] = tris[r][0];
        T.tri[t][c][r][1] = dot < 0 ? tris[r][2] : tris[r][1];
        T.tri[t][c][r][2] = dot < 0 ? tris[r][1] : tris[r][2];
      }
    }
  return T;
}

constexpr TetTable TETS_HOST = make_tet_table();
static_assert(TETS_HOST.nusers[0] == 4 && TETS_HOST.nusers[3] == 2 && TETS_HOST.nusers[6] == 1, "edge users of the Kuhn split");
__constant__ TetTable TETS = make_tet_table();

// ---- kernels ------------------------------------------------------------------------------------------------------------
struct MeshArgs {
  double o[3], s;      // origin, voxel (fp64: positions)
  float sf, muf;       // voxel, truncation (fp32: integration)
  int B, b[3];         // brick size and index
  int min_weight;
};

__device__ __forceinline__ bool positive_finite_(float v) { return v > 0.f && v <= 3.402823466e38f; }

__global__ __launch_bounds__(256) void k_tsdf_integrate(const MeshArgs a, const adamvs_mesh_view* __restrict__ views, int nviews,
                                                        const int* __restrict__ list, int nlist, float* __restrict__ tsdf,
                                                        uint16_t* __restrict__ weight, unsigned* __restrict__ rgba_out) {
  const int B1 = a.B + 1;
  const int n = blockIdx.x * MESH_TILE + threadIdx.x;
  if (n >= B1 * B1 * B1) return;
  const int lx = n % B1, ly = (n / B1) % B1, lz = n / (B1 * B1);
  const float gx = (float)(a.b[0] * a.B + lx) * a.sf, gy = (float)(a.b[1] * a.B + ly) * a.sf, gz = (float)(a.b[2] * a.B + lz) * a.sf;
  float T = 0.f;
  int w = 0, nc = 0;
  unsigned cr = 0, cg = 0, cb = 0;
  for (int i = 0; i < nlist; ++i) {
    const int vi = __builtin_amdgcn_readfirstlane(list[i]);
    if (vi < 0 || vi >= nviews) continue;
    const adamvs_mesh_view& V = views[vi];
    const float x0 = gx - V.c[0], x1 = gy - V.c[1], x2 = gz - V.c[2];
    const float px = V.R[0] * x0 + V.R[1] * x1 + V.R[2] * x2;
    const float py = V.R[3] * x0 + V.R[4] * x1 + V.R[5] * x2;
    const float z = V.R[6] * x0 + V.R[7] * x1 + V.R[8] * x2;
    if (!(z > 0.f)) continue;
    const float u = (V.K[0] * px + V.K[1] * py + V.K[2] * z) / z;
    const float v = (V.K[3] * px + V.K[4] * py + V.K[5] * z) / z;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.f && fu < (float)V.W && fv >= 0.f && fv < (float)V.H)) continue;     // NaN fails too
    const size_t pix = (size_t)(int)fv * V.W + (int)fu;
    const float d = V.depth[pix];
    if (!positive_finite_(d)) continue;
    const float sdf = d - z;
    if (sdf < -a.muf) continue;
    T += fminf(1.f, sdf / a.muf);
    ++w;
    if (fabsf(sdf) <= a.muf) {
      const unsigned px4 = *(const unsigned*)(V.rgba + 4 * pix);
      cr += px4 & 255u;
      cg += (px4 >> 8) & 255u;
      cb += (px4 >> 16) & 255u;
      ++nc;
    }
  }
  tsdf[n] = w > 0 ? T / (float)w : 0.f;
  weight[n] = (uint16_t)(w < 65535 ? w : 65535);
  const unsigned h = (unsigned)nc / 2u;
  rgba_out[n] = nc == 0 ? 0u
                        : ((cr + h) / nc) | (((cg + h) / nc) << 8) | (((cb + h) / nc) << 16) | (255u << 24);
}

__global__ __launch_bounds__(256) void k_mesh_classify(const MeshArgs a, const float* __restrict__ tsdf,
                                                       const uint16_t* __restrict__ weight, unsigned* __restrict__ cube_code,
                                                       unsigned* __restrict__ block_tris) {
  const int B = a.B, B1 = B + 1;
  const int n = blockIdx.x * MESH_TILE + threadIdx.x;         // B^3 is a multiple of the tile: every lane has a cube
  const int lx = n % B, ly = (n / B) % B, lz = n / (B * B);
  const int s0 = (lz * B1 + ly) * B1 + lx;
  bool processed = true;
  int inside = 0;
  for (int c = 0; c < 8; ++c) {
    const int s = s0 + (c & 1) + ((c >> 1) & 1) * B1 + ((c >> 2) & 1) * B1 * B1;
    processed = processed && weight[s] >= a.min_weight;
    inside |= (tsdf[s] < 0.f ? 1 : 0) << c;
  }
  unsigned code = 0, ntri = 0;
  if (processed) {
    code = 1;
    for (int t = 0; t < 6; ++t) {
      int cs = 0;
      for (int k = 0; k < 4; ++k) cs |= ((inside >> TETS.vert[t][k]) & 1) << k;
      code |= (unsigned)cs << (1 + 4 * t);
      ntri += TETS.ntri[cs];
    }
    code |= ntri << 25;
  }
  cube_code[n] = code;
  unsigned total;
  block_exclusive_scan(ntri, &total);
  if (threadIdx.x == 0) block_tris[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_mesh_count_vertices(const MeshArgs a, const float* __restrict__ tsdf,
                                                             const unsigned* __restrict__ cube_code, uint8_t* __restrict__ edge_mask,
                                                             unsigned* __restrict__ block_verts) {
  const int B = a.B, B1 = B + 1;
  const int n = blockIdx.x * MESH_TILE + threadIdx.x;
  const bool live = n < B1 * B1 * B1;
  unsigned mask = 0;
  if (live) {
    const int l[3] = {n % B1, (n / B1) % B1, n / (B1 * B1)};
    const bool in0 = tsdf[n] < 0.f;
#pragma unroll
    for (int e = 0; e < 7; ++e) {
      const int d = DIR_BITS[e];
      const int m[3] = {l[0] + (d & 1), l[1] + ((d >> 1) & 1), l[2] + ((d >> 2) & 1)};
      if (m[0] > B || m[1] > B || m[2] > B) continue;
      if ((tsdf[(m[2] * B1 + m[1]) * B1 + m[0]] < 0.f) == in0) continue;
      bool used = false;
      for (int u = 0; u < TETS.nusers[e]; ++u) {
        const int s = TETS.users[e][u];
        const int c[3] = {l[0] - (s & 1), l[1] - ((s >> 1) & 1), l[2] - ((s >> 2) & 1)};
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= B || c[1] >= B || c[2] >= B) continue;
        used = used || (cube_code[(c[2] * B + c[1]) * B + c[0]] & 1u);
      }
      if (used) mask |= 1u << e;
    }
    edge_mask[n] = (uint8_t)mask;
  }
  unsigned total;
  block_exclusive_scan((unsigned)__popc(mask), &total);
  if (threadIdx.x == 0) block_verts[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void k_mesh_emit_vertices(const MeshArgs a, const float* __restrict__ tsdf,
                                                            const unsigned* __restrict__ rgba, const uint8_t* __restrict__ edge_mask,
                                                            const unsigned* __restrict__ vert_offsets, double* __restrict__ xyz,
                                                            uint8_t* __restrict__ rgb, unsigned* __restrict__ first_vertex,
                                                            long capacity) {
  const int B = a.B, B1 = B + 1;
  const int n = blockIdx.x * MESH_TILE + threadIdx.x;
  const bool live = n < B1 * B1 * B1;
  const unsigned mask = live ? edge_mask[n] : 0u;
  unsigned total;
  const unsigned first = vert_offsets[blockIdx.x] + block_exclusive_scan((unsigned)__popc(mask), &total);
  if (!live) return;
  first_vertex[n] = first;
  if (!mask) return;
  const int l[3] = {n % B1, (n / B1) % B1, n / (B1 * B1)};
  const float ta = tsdf[n];
  const unsigned ca = rgba[n];
  unsigned q = first;
  for (int e = 0; e < 7; ++e) {
    if (!((mask >> e) & 1u)) continue;
    const int d = DIR_BITS[e];
    const int m = ((l[2] + ((d >> 2) & 1)) * B1 + l[1] + ((d >> 1) & 1)) * B1 + l[0] + (d & 1);
    const float tb = tsdf[m];
    const float lam = ta / (ta - tb);
    const unsigned cb = rgba[m];
    if ((long)q < capacity) {
      for (int ax = 0; ax < 3; ++ax) {
        double g = (double)(a.b[ax] * B + l[ax]);
        if ((d >> ax) & 1) g = g + (double)lam;
        xyz[3 * (size_t)q + ax] = a.o[ax] + g * a.s;
      }
      for (int ch = 0; ch < 3; ++ch) {
        const float fa = (float)((ca >> (8 * ch)) & 255u), fb = (float)((cb >> (8 * ch)) & 255u);
        const float c = rintf(fa + lam * (fb - fa));
        rgb[3 * (size_t)q + ch] = (uint8_t)fminf(255.f, fmaxf(0.f, c));
      }
    }
    ++q;
  }
}

__global__ __launch_bounds__(256) void k_mesh_emit_triangles(const MeshArgs a, const unsigned* __restrict__ cube_code,
                                                             const uint8_t* __restrict__ edge_mask,
                                                             const unsigned* __restrict__ first_vertex,
                                                             const unsigned* __restrict__ tri_offsets, unsigned vertex_base,
                                                             unsigned* __restrict__ faces, long capacity) {
  const int B = a.B, B1 = B + 1;
  const int n = blockIdx.x * MESH_TILE + threadIdx.x;
  const unsigned code = cube_code[n];
  unsigned total;
  unsigned q = tri_offsets[blockIdx.x] + block_exclusive_scan((code >> 25) & 15u, &total);
  if (!(code & 1u)) return;
  const int s0 = ((n / (B * B)) * B1 + (n / B) % B) * B1 + n % B;
  for (int t = 0; t < 6; ++t) {
    const int cs = (code >> (1 + 4 * t)) & 15;
    for (int r = 0; r < TETS.ntri[cs]; ++r) {
      if ((long)q < capacity) {
        for (int m = 0; m < 3; ++m) {
          const int k = TETS.tri[t][cs][r][m];
          const int st = TETS.edge_start[t][k], e = TETS.edge_dir[t][k];
          const int s = s0 + (st & 1) + ((st >> 1) & 1) * B1 + ((st >> 2) & 1) * B1 * B1;
          faces[3 * (size_t)q + m] = vertex_base + first_vertex[s] + (unsigned)__popc(edge_mask[s] & ((1u << e) - 1u));
        }
      }
      ++q;
    }
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
static MeshArgs mesh_args(const adamvs_mesh_brick& b) {
  MeshArgs a;
  memset(&a, 0, sizeof(a));
  for (int i = 0; i < 3; ++i) a.o[i] = b.origin[i];
  a.s = b.voxel;
  a.sf = (float)b.voxel;
  a.muf = (float)b.mu;
  a.B = b.B;
  a.b[0] = b.bx, a.b[1] = b.by, a.b[2] = b.bz;
  a.min_weight = b.min_weight;
  return a;
}

static unsigned sample_blocks(int B) { return tiles256((long)(B + 1) * (B + 1) * (B + 1)); }
static unsigned cube_blocks(int B) { return (unsigned)((long)B * B * B / MESH_TILE); }

int launch_tsdf_integrate(const adamvs_mesh_brick& b, const adamvs_mesh_view* views, int nviews, const int* list, int nlist, float* tsdf,
                          uint16_t* weight, unsigned* rgba, hipStream_t st) {
  hipLaunchKernelGGL(k_tsdf_integrate, dim3(sample_blocks(b.B)), dim3(MESH_TILE), 0, st, mesh_args(b), views, nviews, list, nlist, tsdf,
                     weight, rgba);
  ADAMVS_CHECK_LAUNCH("tsdf_integrate");
  return 0;
}

int launch_mesh_classify(const adamvs_mesh_brick& b, const float* tsdf, const uint16_t* weight, unsigned* cube_code, unsigned* block_tris,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_mesh_classify, dim3(cube_blocks(b.B)), dim3(MESH_TILE), 0, st, mesh_args(b), tsdf, weight, cube_code, block_tris);
  ADAMVS_CHECK_LAUNCH("mesh_classify");
  return 0;
}

int launch_mesh_count_vertices(const adamvs_mesh_brick& b, const float* tsdf, const unsigned* cube_code, uint8_t* edge_mask,
                               unsigned* block_verts, hipStream_t st) {
  hipLaunchKernelGGL(k_mesh_count_vertices, dim3(sample_blocks(b.B)), dim3(MESH_TILE), 0, st, mesh_args(b), tsdf, cube_code, edge_mask,
                     block_verts);
  ADAMVS_CHECK_LAUNCH("mesh_count_vertices");
  return 0;
}

int launch_mesh_emit(const adamvs_mesh_brick& b, const float* tsdf, const unsigned* rgba, const unsigned* cube_code, const uint8_t* edge_mask,
                     const unsigned* vert_offsets, const unsigned* tri_offsets, unsigned vertex_base, double* xyz, uint8_t* rgb,
                     unsigned* first_vertex, long vert_capacity, unsigned* faces, long tri_capacity, hipStream_t st) {
  const MeshArgs a = mesh_args(b);
  hipLaunchKernelGGL(k_mesh_emit_vertices, dim3(sample_blocks(b.B)), dim3(MESH_TILE), 0, st, a, tsdf, rgba, edge_mask, vert_offsets, xyz,
                     rgb, first_vertex, vert_capacity);
  ADAMVS_CHECK_LAUNCH("mesh_emit_vertices");
  hipLaunchKernelGGL(k_mesh_emit_triangles, dim3(cube_blocks(b.B)), dim3(MESH_TILE), 0, st, a, cube_code, edge_mask, first_vertex,
                     tri_offsets, vertex_base, faces, tri_capacity);
  ADAMVS_CHECK_LAUNCH("mesh_emit_triangles");
  return 0;
}

}  // namespace adamvs
