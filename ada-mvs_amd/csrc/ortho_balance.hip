// Image orthophoto, radiometric balance: one gain per view and channel from the pairwise statistics of the views over the
// cells they both see (include/adamvs_hip.h "Image orthophoto: radiometric balance" states every operation; ada_mvs_amd/ortho.py
// drives it and solves the V x V system on the host).
//
//   k_ortho_observe      per view: one lane per lattice cell, the visibility test and bilinear sample of k_ortho_compose
//                        (ortho_sample.h), the colour quantised to 1/64 level with a visibility flag: 8 bytes per cell
//   k_ortho_pair_stats   once: one workgroup per (chunk of the lattice, pair); it streams its chunk of both planes in 16-byte
//                        vectors, sums in registers, reduces over the wave and then the four waves, and adds its seven sums
//                        with one 64-bit integer atomic each
//   k_ortho_adjust_image per view: one lane per pixel, the gain applied to the 8-bit image
//   k_ortho_seam_stats   once: the squared colour steps between adjacent mosaic cells of different views
//
// Every result is an integer and every cross-workgroup sum an integer atomic: nothing depends on the order of a reduction.
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "ortho_sample.h"

// The header states the arithmetic operation by operation: no contraction into fma in this file.
#pragma clang fp contract(off)

namespace adamvs {

static_assert(ORTHO_TILE == 256, "kernels below assume workgroups of four waves");

typedef unsigned long long u64;
// two samples of a plane; a plane of an odd N_s starts on an 8-byte boundary only
typedef unsigned u32x4_a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef unsigned u32x2_a8 __attribute__((ext_vector_type(2), aligned(8)));

// Sum of NQ per-lane quantities over the workgroup, added to dst[0 .. NQ) with one atomic each (zero sums are not sent).
// Every lane must call it.
template <int NQ>
__device__ __forceinline__ void block_atomic_sums(const u64 (&v)[NQ], u64* __restrict__ dst) {
  __shared__ u64 part[4][NQ];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = 0; k < NQ; ++k) {
    const u64 s = wave_sum(v[k]);
    if (lane == 0) part[wv][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NQ) {
    const u64 s = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (s) atomicAdd(dst + threadIdx.x, s);
  }
}

__global__ __launch_bounds__(256) void k_ortho_bal_zero(u64* __restrict__ p, int n) {
  const int k = blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (k < n) p[k] = 0ull;
}

// ---- observe --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ortho_observe(const OrthoArgs a, const ViewCam c, const uint8_t* __restrict__ rgba,
                                                       const float* __restrict__ dsm, const unsigned* __restrict__ zbuf, int S, int Ws,
                                                       int Ns, float border, float tol, u32x2_a8* __restrict__ obs) {
  const int n = blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (n >= Ns) return;
  const int ia = (n % Ws) * S, ib = (n / Ws) * S;                  // the DSM cell: ia < W, ib < H by the lattice's size
  const float z = dsm[(long)ib * a.W + ia];
  u32x2_a8 o = {0u, 0u};
  Proj p;
  if (isfinite(z) && ortho_visible(c, zbuf, border, tol, a.x0 + ((double)ia + 0.5) * a.gsd, a.y_top - ((double)ib + 0.5) * a.gsd, (double)z, p)) {
    float col[3];
    ortho_bilinear(c, rgba, p, col);
    const unsigned q0 = (unsigned)floorf(64.f * col[0] + 0.5f), q1 = (unsigned)floorf(64.f * col[1] + 0.5f);
    const unsigned q2 = (unsigned)floorf(64.f * col[2] + 0.5f);
    o[0] = q0 | (q1 << 16);
    o[1] = q2 | (1u << 16);
  }
  obs[n] = o;
}

// ---- pair statistics ------------------------------------------------------------------------------------------------
constexpr int PAIR_VEC = 4;                                        // 16-byte loads in flight per lane and plane
constexpr int PAIR_ROUND = ORTHO_TILE * 2 * PAIR_VEC;              // lattice cells per workgroup and round of loads
static_assert(ORTHO_BAL_CHUNK % PAIR_ROUND == 0, "a chunk is a whole number of rounds");
// the per-lane sums are 32 bits wide: a lane sees ORTHO_BAL_CHUNK / 256 cells of at most ADAMVS_ORTHO_BAL_MAX_Q each
static_assert((long)(ORTHO_BAL_CHUNK / ORTHO_TILE) * ADAMVS_ORTHO_BAL_MAX_Q < (1L << 32), "per-lane sums would overflow");

// one lattice cell of both views: lo = q_r | q_g << 16, hi = q_b | flag << 16
__device__ __forceinline__ void pair_cell(unsigned alo, unsigned ahi, unsigned blo, unsigned bhi, int maxd, unsigned (&acc)[7]) {
  const int a0 = (int)(alo & 0xFFFFu), a1 = (int)(alo >> 16), a2 = (int)(ahi & 0xFFFFu);
  const int b0 = (int)(blo & 0xFFFFu), b1 = (int)(blo >> 16), b2 = (int)(bhi & 0xFFFFu);
  // bitwise, not short-circuit: no branch per cell
  const int ok = (int)((ahi >> 16) == 1u) & (int)((bhi >> 16) == 1u) & (int)(abs(a0 - b0) <= maxd) & (int)(abs(a1 - b1) <= maxd) &
                 (int)(abs(a2 - b2) <= maxd);
  const unsigned m = 0u - (unsigned)ok;
  acc[0] += m & 1u;
  acc[1] += m & (unsigned)a0;
  acc[2] += m & (unsigned)a1;
  acc[3] += m & (unsigned)a2;
  acc[4] += m & (unsigned)b0;
  acc[5] += m & (unsigned)b1;
  acc[6] += m & (unsigned)b2;
}

__global__ __launch_bounds__(256) void k_ortho_pair_stats(const unsigned* __restrict__ obs, int Ns, const int* __restrict__ pairs,
                                                          int maxd, u64* __restrict__ stats) {
  const int nchunk = (Ns + ORTHO_BAL_CHUNK - 1) / ORTHO_BAL_CHUNK;
  const int pr = blockIdx.x / nchunk;
  const unsigned* __restrict__ A = obs + 2l * Ns * pairs[2 * pr];          // two dwords per cell
  const unsigned* __restrict__ B = obs + 2l * Ns * pairs[2 * pr + 1];
  const int lo = (blockIdx.x - pr * nchunk) * ORTHO_BAL_CHUNK;               // even; lo < Ns by the grid's size
  const int hi = lo + ORTHO_BAL_CHUNK < Ns ? lo + ORTHO_BAL_CHUNK : Ns;
  unsigned acc[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (hi - lo == ORTHO_BAL_CHUNK) {
    // a whole chunk (uniform over the workgroup): every load is inside the planes, PAIR_VEC per plane in flight
    for (int base = lo + 2 * (int)threadIdx.x; base < hi; base += PAIR_ROUND) {
      u32x4_a8 va[PAIR_VEC], vb[PAIR_VEC];
#pragma unroll
      for (int k = 0; k < PAIR_VEC; ++k) {
        va[k] = *(const u32x4_a8*)(A + 2l * (base + k * 2 * ORTHO_TILE));
        vb[k] = *(const u32x4_a8*)(B + 2l * (base + k * 2 * ORTHO_TILE));
      }
#pragma unroll
      for (int k = 0; k < PAIR_VEC; ++k) {
        pair_cell(va[k][0], va[k][1], vb[k][0], vb[k][1], maxd, acc);
        pair_cell(va[k][2], va[k][3], vb[k][2], vb[k][3], maxd, acc);
      }
    }
  } else {
    // the last chunk of the lattice: cells n and n + 1 while both are below N_s, then the last cell of an odd N_s alone
    for (int n = lo + 2 * (int)threadIdx.x; n < hi; n += 2 * ORTHO_TILE) {
      if (n + 1 < hi) {
        const u32x4_a8 va = *(const u32x4_a8*)(A + 2l * n), vb = *(const u32x4_a8*)(B + 2l * n);
        pair_cell(va[0], va[1], vb[0], vb[1], maxd, acc);
        pair_cell(va[2], va[3], vb[2], vb[3], maxd, acc);
      } else {
        const u32x2_a8 ta = *(const u32x2_a8*)(A + 2l * n), tb = *(const u32x2_a8*)(B + 2l * n);
        pair_cell(ta[0], ta[1], tb[0], tb[1], maxd, acc);
      }
    }
  }
  u64 wide[7];
  for (int k = 0; k < 7; ++k) wide[k] = acc[k];
  block_atomic_sums<7>(wide, stats + 7l * pr);
}

// ---- adjust ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ortho_adjust_image(const unsigned* __restrict__ in, long npx, float g0, float g1, float g2,
                                                            unsigned* __restrict__ out) {
  const long n = (long)blockIdx.x * ORTHO_TILE + threadIdx.x;
  if (n >= npx) return;
  const unsigned px = in[n];
  const float g[3] = {g0, g1, g2};
  unsigned o = px & 0xFF000000u;
  for (int ch = 0; ch < 3; ++ch) {
    const float q = fminf(255.f, floorf(g[ch] * (float)((px >> (8 * ch)) & 255u) + 0.5f));
    o |= (unsigned)q << (8 * ch);
  }
  out[n] = o;
}

// ---- seam statistics ------------------------------------------------------------------------------------------------
constexpr int SEAM_CELLS = 8;                                      // mosaic cells per lane

__device__ __forceinline__ void seam_step(unsigned pa, unsigned pb, unsigned (&acc)[4]) {
  acc[0] += 1u;
  for (int ch = 0; ch < 3; ++ch) {
    const int d = (int)((pa >> (8 * ch)) & 255u) - (int)((pb >> (8 * ch)) & 255u);
    acc[1 + ch] += (unsigned)(d * d);
  }
}

__global__ __launch_bounds__(256) void k_ortho_seam_stats(int Wo, int Ho, const int* __restrict__ view, const unsigned* __restrict__ rgba,
                                                          u64* __restrict__ stats) {
  const long ncell = (long)Wo * Ho;
  unsigned acc[4] = {0u, 0u, 0u, 0u};                               // at most 2 SEAM_CELLS steps of 3 x 255^2 per lane
  for (int k = 0; k < SEAM_CELLS; ++k) {
    const long n = ((long)blockIdx.x * SEAM_CELLS + k) * ORTHO_TILE + threadIdx.x;
    if (n >= ncell) break;
    const int v = view[n];
    if (v < 0) continue;
    const int i = (int)(n % Wo), j = (int)(n / Wo);
    const unsigned px = rgba[n];
    if (i + 1 < Wo) {
      const int w = view[n + 1];
      if (w >= 0 && w != v) seam_step(px, rgba[n + 1], acc);
    }
    if (j + 1 < Ho) {
      const int w = view[n + Wo];
      if (w >= 0 && w != v) seam_step(px, rgba[n + Wo], acc);
    }
  }
  u64 wide[4];
  for (int k = 0; k < 4; ++k) wide[k] = acc[k];
  block_atomic_sums<4>(wide, stats);
}

// ---- launchers ------------------------------------------------------------------------------------------------------
static unsigned bal_blocks(long n, long per) { return (unsigned)((n + per - 1) / per); }

int launch_ortho_observe(const adamvs_ortho_grid& g, const float* dsm, const adamvs_ortho_view& v, const unsigned* zbuf, int S, float border,
                         float tol, uint16_t* obs, hipStream_t st) {
  const int Ws = (g.W + S - 1) / S, Hs = (g.H + S - 1) / S;
  const int Ns = Ws * Hs;                                           // at most 2^20: checked by the caller
  hipLaunchKernelGGL(k_ortho_observe, dim3(bal_blocks(Ns, ORTHO_TILE)), dim3(ORTHO_TILE), 0, st, ortho_args(g), view_cam(v), v.rgba, dsm,
                     zbuf, S, Ws, Ns, border, tol, (u32x2_a8*)obs);
  ADAMVS_CHECK_LAUNCH("ortho_observe");
  return 0;
}

int launch_ortho_pair_stats(const uint16_t* obs, long Ns, const int* pairs, int P, int max_diff_q, long long* stats, hipStream_t st) {
  hipLaunchKernelGGL(k_ortho_bal_zero, dim3(bal_blocks(7l * P, ORTHO_TILE)), dim3(ORTHO_TILE), 0, st, (u64*)stats, 7 * P);
  ADAMVS_CHECK_LAUNCH("ortho_pair_stats (zero)");
  hipLaunchKernelGGL(k_ortho_pair_stats, dim3(bal_blocks(Ns, ORTHO_BAL_CHUNK) * P), dim3(ORTHO_TILE), 0, st, (const unsigned*)obs, (int)Ns,
                     pairs, max_diff_q, (u64*)stats);
  ADAMVS_CHECK_LAUNCH("ortho_pair_stats");
  return 0;
}

int launch_ortho_adjust_image(const uint8_t* rgba_in, long npx, const float* gain, uint8_t* rgba_out, hipStream_t st) {
  hipLaunchKernelGGL(k_ortho_adjust_image, dim3(bal_blocks(npx, ORTHO_TILE)), dim3(ORTHO_TILE), 0, st, (const unsigned*)rgba_in, npx, gain[0],
                     gain[1], gain[2], (unsigned*)rgba_out);
  ADAMVS_CHECK_LAUNCH("ortho_adjust_image");
  return 0;
}

int launch_ortho_seam_stats(const adamvs_ortho_grid& g, const int* view_out, const uint8_t* rgba, long long* stats, hipStream_t st) {
  const int Wo = g.W * g.K, Ho = g.H * g.K;
  hipLaunchKernelGGL(k_ortho_bal_zero, dim3(1), dim3(ORTHO_TILE), 0, st, (u64*)stats, 4);
  ADAMVS_CHECK_LAUNCH("ortho_seam_stats (zero)");
  hipLaunchKernelGGL(k_ortho_seam_stats, dim3(bal_blocks((long)Wo * Ho, (long)SEAM_CELLS * ORTHO_TILE)), dim3(ORTHO_TILE), 0, st, Wo, Ho,
                     view_out, (const unsigned*)rgba, (u64*)stats);
  ADAMVS_CHECK_LAUNCH("ortho_seam_stats");
  return 0;
}

}  // namespace adamvs
