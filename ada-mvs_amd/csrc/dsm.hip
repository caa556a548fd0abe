// Rasterisation of a fused point cloud into a DSM (height raster) and a true orthophoto (the step after fuse_whu.py).
// Three launches, include/adamvs_hip.h "DSM" states the semantics exactly:
//
//   k_dsm_accumulate   one lane per point: grid cell in fp64, 64-bit key  o(h) << 32 | (0xFFFFFFFF - seq)  (atomicMax),
//                      count (atomicAdd u32) and, in mean mode, the integer height sum (atomicAdd s64)
//   k_dsm_claim        after its chunk's accumulate: the lane whose key equals the cell's key writes the point's colour
//   k_dsm_finalize     one lane per cell: height, saturated count and RGBA, NaN / 0 below min_count
//
// Every reduction is an integer max or sum, so the rasters do not depend on the order in which the atomics land: the output
// is bit-identical from run to run, and in mean mode under any permutation or chunking of the points.
//
// Points arrive in row-major pixel order per view, so runs of neighbouring lanes hit the same cell (at coarse GSD a run can
// span the whole wave).  Same-address atomics serialise at the memory side, so each run of equal cells inside a wave is
// combined first (max key, count, sum through __shfl_down; a segmented reduction whose step count is the log2 of the
// longest run) and only the run's first lane issues the atomics.  -DADAMVS_DSM_NO_COMBINE (tools/build_variant.py) builds
// the uncombined form, one set of atomics per used point, for A/B timing.
#include "common.h"
#include "kernels.h"

// The semantics are stated operation by operation and tests hold the kernels to an fp64 restatement bit for bit: no
// contraction of a multiply and an add into an fma in this file.
#pragma clang fp contract(off)

namespace adamvs {

// Order-preserving map of an fp32 height to uint32 (larger height -> larger value); -0 is taken as +0, so equal heights
// give equal values and the sequence number decides.  Finite heights map to values >= 0x00800000: a used point's key is
// never 0, which marks an empty cell.
__device__ __forceinline__ unsigned dsm_order(float h) {
  const unsigned b = __float_as_uint(h == 0.f ? 0.f : h);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float dsm_unorder(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// Cell of a point and its height above z_ref, in fp64 with exactly the operations of the header.  NaN / inf coordinates fail
// the range tests (a NaN comparison is false, an infinite one out of range), so "used" needs no separate finiteness test.
__device__ __forceinline__ bool dsm_cell(const adamvs_dsm_grid& g, const double* __restrict__ p, int& cell, double& dz) {
  const double fi = floor((p[0] - g.x0) / g.gsd);
  const double fj = floor((g.y_top - p[1]) / g.gsd);
  dz = p[2] - g.z_ref;
  if (!(fi >= 0.0 && fi < (double)g.W && fj >= 0.0 && fj < (double)g.H && fabs(dz) < 65536.0)) return false;
  cell = (int)fj * g.W + (int)fi;
  return true;
}

__device__ __forceinline__ unsigned long long dsm_key(double dz, unsigned seq) {
  return ((unsigned long long)dsm_order((float)dz) << 32) | (unsigned long long)(0xffffffffu - seq);
}

template <bool MEAN>
__global__ __launch_bounds__(256) void k_dsm_accumulate(const adamvs_dsm_grid g, const double* __restrict__ xyz, long n, unsigned seq0,
                                                        unsigned long long* __restrict__ key, unsigned* __restrict__ count,
                                                        unsigned long long* __restrict__ sum) {
  const long k = (long)blockIdx.x * DSM_TILE + threadIdx.x;
  int cell = -1;                                       // -1: not a used point (outside the chunk or refused)
  unsigned long long kk = 0;
  unsigned c = 0;
  long long q = 0;
  if (k < n) {
    double dz;
    if (dsm_cell(g, xyz + 3 * k, cell, dz)) {
      kk = dsm_key(dz, seq0 + (unsigned)k);
      c = 1;
      if (MEAN) q = (long long)rint(dz * 65536.0);
    } else {
      cell = -1;
    }
  }
#ifndef ADAMVS_DSM_NO_COMBINE
  // Segmented reduction over runs of equal cells (every lane of the wave takes part; refused lanes form runs of cell -1).
  // After the step of offset `off`, a lane holds the reduction of [lane, min(lane + 2 off - 1, end of its run)].
  const int lane = threadIdx.x & 63;
  const int prev = __shfl_up(cell, 1);                 // every lane takes part: not inside a short-circuit (lane 0 would drop out
  const bool head = (lane == 0) | (prev != cell);      // and lane 1 would read 0 from it)
  const unsigned long long heads = __ballot(head);
  const int end = lane + __builtin_ctzll(((heads >> 1) | (1ull << 63)) >> lane);     // last lane of this lane's run
  // cont: bit i set when lanes i .. i + off - 1 all continue the run of the lane before them, i.e. some run is longer than
  // the offsets reduced so far (bit 0 is a head, so this reaches 0 after at most the step of offset 32)
  unsigned long long cont = ~heads;
  for (int off = 1; cont; off <<= 1) {                 // wave-uniform: cont comes from a ballot
    const unsigned long long k2 = __shfl_down(kk, off);
    const unsigned c2 = __shfl_down(c, off);
    const long long q2 = MEAN ? __shfl_down(q, off) : 0;
    if (lane + off <= end) {
      kk = kk > k2 ? kk : k2;
      c += c2;
      q += q2;
    }
    cont &= cont >> off;
  }
  if (!head || cell < 0) return;
#else
  if (cell < 0) return;
#endif
  atomicMax(key + cell, kk);
  atomicAdd(count + cell, c);
  if (MEAN) atomicAdd(sum + cell, (unsigned long long)q);     // two's complement: a signed sum
}

__global__ __launch_bounds__(256) void k_dsm_claim(const adamvs_dsm_grid g, const double* __restrict__ xyz, const uint8_t* __restrict__ rgb,
                                                   long n, unsigned seq0, const unsigned long long* __restrict__ key,
                                                   unsigned* __restrict__ color) {
  const long k = (long)blockIdx.x * DSM_TILE + threadIdx.x;
  if (k >= n) return;
  int cell;
  double dz;
  if (!dsm_cell(g, xyz + 3 * k, cell, dz)) return;
  if (key[cell] != dsm_key(dz, seq0 + (unsigned)k)) return;      // keys are unique: one lane of the whole stream matches
  const uint8_t* c = rgb + 3 * k;
  color[cell] = (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16) | 0xff000000u;
}

template <bool MEAN>
__global__ __launch_bounds__(256) void k_dsm_finalize(long ncell, double z_ref, const unsigned long long* __restrict__ key,
                                                      const unsigned* __restrict__ count, const unsigned long long* __restrict__ sum,
                                                      const unsigned* __restrict__ color, unsigned min_count, float* __restrict__ dsm,
                                                      uint16_t* __restrict__ count16, unsigned* __restrict__ rgba) {
  const long c = (long)blockIdx.x * DSM_TILE + threadIdx.x;
  if (c >= ncell) return;
  const unsigned cnt = count[c];
  count16[c] = (uint16_t)(cnt < 65535u ? cnt : 65535u);
  if (cnt < min_count) {
    dsm[c] = __uint_as_float(0x7fc00000u);                    // the quiet NaN numpy writes
    rgba[c] = 0u;
    return;
  }
  if (MEAN)
    dsm[c] = (float)(z_ref + ((double)(long long)sum[c] / (double)cnt) / 65536.0);
  else
    dsm[c] = (float)(z_ref + (double)dsm_unorder((unsigned)(key[c] >> 32)));
  rgba[c] = color[c];
}

static unsigned dsm_blocks(long n) { return (unsigned)((n + DSM_TILE - 1) / DSM_TILE); }

int launch_dsm_accumulate(const adamvs_dsm_grid& g, const double* xyz, long n, long seq0, int mode, unsigned long long* key,
                          unsigned* count, long long* sum, hipStream_t st) {
  if (n == 0) return 0;
  if (mode == ADAMVS_DSM_MEAN)
    hipLaunchKernelGGL(k_dsm_accumulate<true>, dim3(dsm_blocks(n)), dim3(DSM_TILE), 0, st, g, xyz, n, (unsigned)seq0, key, count,
                       (unsigned long long*)sum);
  else
    hipLaunchKernelGGL(k_dsm_accumulate<false>, dim3(dsm_blocks(n)), dim3(DSM_TILE), 0, st, g, xyz, n, (unsigned)seq0, key, count,
                       (unsigned long long*)sum);
  ADAMVS_CHECK_LAUNCH("dsm_accumulate");
  return 0;
}

int launch_dsm_claim(const adamvs_dsm_grid& g, const double* xyz, const uint8_t* rgb, long n, long seq0, const unsigned long long* key,
                     unsigned* color, hipStream_t st) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_dsm_claim, dim3(dsm_blocks(n)), dim3(DSM_TILE), 0, st, g, xyz, rgb, n, (unsigned)seq0, key, color);
  ADAMVS_CHECK_LAUNCH("dsm_claim");
  return 0;
}

int launch_dsm_finalize(const adamvs_dsm_grid& g, const unsigned long long* key, const unsigned* count, const long long* sum,
                        const unsigned* color, int mode, int min_count, float* dsm, uint16_t* count16, unsigned* rgba, hipStream_t st) {
  const long ncell = (long)g.W * g.H;
  if (mode == ADAMVS_DSM_MEAN)
    hipLaunchKernelGGL(k_dsm_finalize<true>, dim3(dsm_blocks(ncell)), dim3(DSM_TILE), 0, st, ncell, g.z_ref, key, count,
                       (const unsigned long long*)sum, color, (unsigned)min_count, dsm, count16, rgba);
  else
    hipLaunchKernelGGL(k_dsm_finalize<false>, dim3(dsm_blocks(ncell)), dim3(DSM_TILE), 0, st, ncell, g.z_ref, key, count,
                       (const unsigned long long*)sum, color, (unsigned)min_count, dsm, count16, rgba);
  ADAMVS_CHECK_LAUNCH("dsm_finalize");
  return 0;
}

}  // namespace adamvs
