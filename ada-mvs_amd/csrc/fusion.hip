// Geometric-consistency filtering and point emission of predicted depth maps (the step after predict_whu.py; the
// reference stops at writing the maps, predict_whu.py "step1").  Three launches per reference view:
//
//   k_geo_consistency   one lane per reference pixel, every source of the view in one pass: reproject, bilinear tap of the
//                       source depth, reproject back, count the consistent sources, average their depths; per-workgroup
//                       number of kept pixels
//   k_fusion_scan       exclusive scan of those counts (one workgroup)
//   k_fusion_emit       each kept pixel to world coordinates (fp64) at  block offset + rank in the block
//
// Workgroups cover FUSION_TILE consecutive pixels of the row-major image, so block order is pixel order and the point
// buffer comes out in row-major order.  No atomics and no inter-workgroup waits: the launches are the synchronisation,
// and the output is bit-identical from run to run.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

namespace adamvs {

// Per-source constants, fp32, formed by the host in fp64 (ada-mvs_amd/fusion.py::relative_transforms):
//   fwd  = {A row-major (9), b (3)}: source pixel (homogeneous) = d * A [x y 1]^T + b, A = K_s R_sr K_r^-1, b = K_s t_sr
//   back = {B row-major (9), c (3)}: reference pixel           = d_s * B [u v 1]^T + c, B = K_r R_rs K_s^-1, c = K_r t_rs
// The third component of either is the depth in that camera (K's last row is 0 0 1).  Passed by value: the loop over
// sources reads them from the kernel-argument segment into scalar registers.
struct FusionArgs {
  const float* depth[FUSION_MAX_SOURCES];
  int H[FUSION_MAX_SOURCES], W[FUSION_MAX_SOURCES];
  float fwd[FUSION_MAX_SOURCES][12];
  float back[FUSION_MAX_SOURCES][12];
  int n;
};

__device__ __forceinline__ bool positive_finite(float v) { return v > 0.f && v <= 3.402823466e38f; }   // false for NaN / inf

__global__ __launch_bounds__(256) void k_geo_consistency(const float* __restrict__ ref_depth, const float* __restrict__ ref_conf, int H,
                                                         int W, const FusionArgs a, float prob_threshold, float pix_threshold2,
                                                         float rel_depth_threshold, int min_consistent, uint8_t* __restrict__ count,
                                                         float* __restrict__ fused, unsigned* __restrict__ block_kept) {
  const long npix = (long)H * W;
  const long p = (long)blockIdx.x * FUSION_TILE + threadIdx.x;
  const bool inside = p < npix;
  const int y = inside ? (int)(p / W) : 0, x = inside ? (int)(p - (long)y * W) : 0;
  const float d = inside ? ref_depth[p] : 0.f;
  const float conf = inside ? ref_conf[p] : 0.f;
  const bool cand = inside && positive_finite(d) && conf >= prob_threshold;      // a NaN confidence is not >=
  int n = 0;
  float sum = d;
  if (cand) {
    const float fx = (float)x, fy = (float)y;
    for (int s = 0; s < a.n; ++s) {
      const float* A = a.fwd[s];
      const float hz = d * (A[6] * fx + A[7] * fy + A[8]) + A[11];
      if (!(hz > 0.f)) continue;
      const float u = (d * (A[0] * fx + A[1] * fy + A[2]) + A[9]) / hz;
      const float v = (d * (A[3] * fx + A[4] * fy + A[5]) + A[10]) / hz;
      const int Ws = a.W[s], Hs = a.H[s];
      if (!(u >= 0.f && u < (float)(Ws - 1) && v >= 0.f && v < (float)(Hs - 1))) continue;     // NaN fails too
      const int x0 = (int)u, y0 = (int)v;                                                      // u, v >= 0: truncation = floor
      const float* row = a.depth[s] + (size_t)y0 * Ws + x0;
      const float t00 = row[0], t01 = row[1], t10 = row[Ws], t11 = row[Ws + 1];
      if (!(positive_finite(t00) && positive_finite(t01) && positive_finite(t10) && positive_finite(t11))) continue;
      const float ax = u - (float)x0, ay = v - (float)y0;
      const float ds = (1.f - ay) * ((1.f - ax) * t00 + ax * t01) + ay * ((1.f - ax) * t10 + ax * t11);
      const float* B = a.back[s];
      const float qz = ds * (B[6] * u + B[7] * v + B[8]) + B[11];
      if (!(qz > 0.f)) continue;
      const float ex = (ds * (B[0] * u + B[1] * v + B[2]) + B[9]) / qz - fx;
      const float ey = (ds * (B[3] * u + B[4] * v + B[5]) + B[10]) / qz - fy;
      if (ex * ex + ey * ey < pix_threshold2 && fabsf(qz - d) < rel_depth_threshold * d) {
        ++n;
        sum += qz;
      }
    }
  }
  const bool kept = cand && n >= min_consistent;
  if (inside) {
    count[p] = (uint8_t)n;
    fused[p] = kept ? sum / (float)(1 + n) : 0.f;
  }
  unsigned total;
  block_rank(kept, &total);
  if (threadIdx.x == 0) block_kept[blockIdx.x] = total;
}

// offsets[i] = sum of counts[0 .. i), offsets[nb] = total.  One workgroup of 1024 lanes, each a contiguous run of counts.
__global__ __launch_bounds__(1024) void k_fusion_scan(const unsigned* __restrict__ counts, unsigned* __restrict__ offsets, int nb) {
  __shared__ unsigned part[1024];
  const int per = (nb + 1023) / 1024;
  const int i0 = threadIdx.x * per, i1 = i0 + per < nb ? i0 + per : nb;
  unsigned local = 0;
  for (int i = i0; i < i1; ++i) local += counts[i];
  part[threadIdx.x] = local;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {          // Hillis-Steele inclusive scan of the 1024 run totals
    const unsigned v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned run = part[threadIdx.x] - local;
  for (int i = i0; i < i1; ++i) {
    offsets[i] = run;
    run += counts[i];
  }
  if (threadIdx.x == 1023) offsets[nb] = part[1023];
}

struct EmitCamera {
  double kinv[9];      // K_r^-1, row-major
  double rwc[9];       // camera (x right, y down, z forward) -> world rotation, row-major
  double c[3];         // camera centre in world coordinates
};

__global__ __launch_bounds__(256) void k_fusion_emit(const float* __restrict__ fused, const uint8_t* __restrict__ rgba, int H, int W,
                                                     const EmitCamera cam, const unsigned* __restrict__ offsets,
                                                     double* __restrict__ xyz, uint8_t* __restrict__ rgb, long capacity) {
  const long npix = (long)H * W;
  const long p = (long)blockIdx.x * FUSION_TILE + threadIdx.x;
  const bool inside = p < npix;
  const float d = inside ? fused[p] : 0.f;
  const bool kept = d > 0.f;
  unsigned total;
  const unsigned rank = block_rank(kept, &total);
  if (!kept) return;
  const long q = (long)offsets[blockIdx.x] + rank;
  if (q >= capacity) return;                           // cannot happen with capacity >= H W; keeps every store in bounds
  const int y = (int)(p / W), x = (int)(p - (long)y * W);
  const double dd = (double)d;
  const double rx = dd * (cam.kinv[0] * x + cam.kinv[1] * y + cam.kinv[2]);
  const double ry = dd * (cam.kinv[3] * x + cam.kinv[4] * y + cam.kinv[5]);
  const double rz = dd * (cam.kinv[6] * x + cam.kinv[7] * y + cam.kinv[8]);
  xyz[3 * q + 0] = cam.rwc[0] * rx + cam.rwc[1] * ry + cam.rwc[2] * rz + cam.c[0];
  xyz[3 * q + 1] = cam.rwc[3] * rx + cam.rwc[4] * ry + cam.rwc[5] * rz + cam.c[1];
  xyz[3 * q + 2] = cam.rwc[6] * rx + cam.rwc[7] * ry + cam.rwc[8] * rz + cam.c[2];
  const uint8_t* px = rgba + 4 * p;
  rgb[3 * q + 0] = px[0];
  rgb[3 * q + 1] = px[1];
  rgb[3 * q + 2] = px[2];
}

static unsigned fusion_blocks(int H, int W) { return tiles256((long)H * W); }

int launch_geo_consistency(const float* ref_depth, const float* ref_conf, int H, int W, const adamvs_fusion_source* srcs, int N,
                           float prob_threshold, float pix_threshold, float rel_depth_threshold, int min_consistent, uint8_t* count,
                           float* fused, unsigned* block_kept, hipStream_t st) {
  FusionArgs a;
  memset(&a, 0, sizeof(a));
  a.n = N;
  for (int s = 0; s < N; ++s) {
    a.depth[s] = srcs[s].depth;
    a.H[s] = srcs[s].H;
    a.W[s] = srcs[s].W;
    memcpy(a.fwd[s], srcs[s].fwd, sizeof(a.fwd[s]));
    memcpy(a.back[s], srcs[s].back, sizeof(a.back[s]));
  }
  hipLaunchKernelGGL(k_geo_consistency, dim3(fusion_blocks(H, W)), dim3(FUSION_TILE), 0, st, ref_depth, ref_conf, H, W, a, prob_threshold,
                     pix_threshold * pix_threshold, rel_depth_threshold, min_consistent, count, fused, block_kept);
  ADAMVS_CHECK_LAUNCH("geo_consistency");
  return 0;
}

int launch_fusion_scan(const unsigned* counts, unsigned* offsets, int nblocks, hipStream_t st) {
  hipLaunchKernelGGL(k_fusion_scan, dim3(1), dim3(1024), 0, st, counts, offsets, nblocks);
  ADAMVS_CHECK_LAUNCH("fusion_scan");
  return 0;
}

int launch_fusion_emit(const float* fused, const uint8_t* rgba, int H, int W, const double* camera, const unsigned* offsets, double* xyz,
                       uint8_t* rgb, long capacity, hipStream_t st) {
  EmitCamera cam;
  memcpy(&cam, camera, sizeof(cam));
  hipLaunchKernelGGL(k_fusion_emit, dim3(fusion_blocks(H, W)), dim3(FUSION_TILE), 0, st, fused, rgba, H, W, cam, offsets, xyz, rgb,
                     capacity);
  ADAMVS_CHECK_LAUNCH("fusion_emit");
  return 0;
}

static_assert(sizeof(EmitCamera) == 21 * sizeof(double), "adamvs_fusion_emit: camera = 21 doubles");

}  // namespace adamvs
