// Roof planes: link bits between adjacent cells of a building, the segments they connect, integer moments per label, the
// growth rounds into the unassigned rims and the residuals of the final planes.
// include/adamvs_hip.h "Roof planes" states the result; this file computes it with these kernels:
//
//   k_roof_links        one lane per cell: whether the cell, its east and its south neighbour are core, their gradients, and the
//                       two link tests.  The neighbours at the stride s are read straight from global memory: for the 64 cells
//                       of a wave each offset is one contiguous 256-byte piece of another row, and the rows i - s .. i + s + 1
//                       stay in L2 between the workgroups that share them.  What dsm_buildings.hip says of k_bld_flags against a
//                       tile with halo in LDS holds here unchanged (at s = 64 the halo is eight times the tile).
//   k_roof_tile /       bld_union.h: k_label_tile, k_label_pairs and launch_label over LinkEdges (a core cell is a node; the
//   k_roof_pairs        east and south bits say where two core cells are joined).  The round's hook and compress kernels and
//                       the final walk are the building stage's.
//   k_roof_moments      one lane per cell; a run of equal labels with a finite Z (raster_prims.h wave_run) is summed into its
//                       first lane, which issues the integer atomics.
//   k_roof_grow         one round: every cell of the output buffer is written (the label kept, or the best neighbouring plane).
//                       One atomicAdd per workgroup of 16 waves counts the cells labelled.
//   k_roof_residuals    the run reduction again: inlier count and the largest quantised residual per plane.
//
// Only integer atomics that commute, so every output is bit-identical from run to run.
#include <math.h>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

// ---- links ------------------------------------------------------------------------------------------------------------------
// whether (i, j) is core; its Z, gradients and building label
__device__ __forceinline__ bool roof_core(int W, int H, const float* __restrict__ dsm, const int* __restrict__ bld, int s, double tol,
                                          int i, int j, double& z, double& gx, double& gy, int& b) {
  if (i - s < 0 || i + s >= H || j - s < 0 || j + s >= W) return false;
  const long c = (long)i * W + j;
  b = bld[c];
  if (b <= 0) return false;
  const long ce = c + s, cw = c - s, cs = c + (long)s * W, cn = c - (long)s * W;
  if (bld[ce] != b || bld[cw] != b || bld[cs] != b || bld[cn] != b) return false;
  const float fz = dsm[c], fe = dsm[ce], fw = dsm[cw], fs = dsm[cs], fn = dsm[cn];
  if (!__builtin_isfinite(fz) || !__builtin_isfinite(fe) || !__builtin_isfinite(fw) || !__builtin_isfinite(fs) || !__builtin_isfinite(fn))
    return false;
  z = (double)fz;
  const double two_z = 2.0 * z;
  const double dx = fabs(((double)fe + (double)fw) - two_z), dy = fabs(((double)fs + (double)fn) - two_z);
  if (!(dx <= tol) || !(dy <= tol)) return false;
  gx = (double)fe - (double)fw;
  gy = (double)fs - (double)fn;
  return true;
}

__global__ __launch_bounds__(BLD_THREADS) void k_roof_links(int W, int H, const float* __restrict__ dsm, const int* __restrict__ bld, int s,
                                                            double smooth_tol, double g_tol, double step_tol, uint8_t* __restrict__ link) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (c >= n) return;
  int i, j;
  cell_ij(c, W, i, j);
  double za = 0.0, gxa = 0.0, gya = 0.0;
  int ba = 0;
  uint8_t out = 0;
  if (roof_core(W, H, dsm, bld, s, smooth_tol, i, j, za, gxa, gya, ba)) {
    out = 1;
    const double four_s = 4.0 * (double)s;
    double zb = 0.0, gxb = 0.0, gyb = 0.0;
    int bb = 0;
    if (j + 1 < W && roof_core(W, H, dsm, bld, s, smooth_tol, i, j + 1, zb, gxb, gyb, bb) && bb == ba) {
      if (fabs(gxa - gxb) <= g_tol && fabs(gya - gyb) <= g_tol && fabs((zb - za) - (gxa + gxb) / four_s) <= step_tol) out |= 2;
    }
    if (i + 1 < H && roof_core(W, H, dsm, bld, s, smooth_tol, i + 1, j, zb, gxb, gyb, bb) && bb == ba) {
      if (fabs(gxa - gxb) <= g_tol && fabs(gya - gyb) <= g_tol && fabs((zb - za) - (gya + gyb) / four_s) <= step_tol) out |= 4;
    }
  }
  link[c] = out;
}

// ---- moments ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_roof_moments(int W, int H, const float* __restrict__ dsm, const int* __restrict__ label,
                                                              const int* __restrict__ bld, double z_ref, long N, long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;       // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int lab = 0, i = 0, j = 0, b = 0;
  long long q = 0;
  if (c < n) {
    lab = label[c];
    if (lab < 1 || (long)lab > N) lab = 0;
  }
  if (__ballot(lab != 0) == 0ull) return;                            // wave-uniform: a wave without labels adds nothing
  if (lab) {
    const float fz = dsm[c];
    if (__builtin_isfinite(fz)) {
      cell_ij(c, W, i, j);
      q = llrint(fmin(fmax(((double)fz - z_ref) * (double)ADAMVS_ROOF_Q_SCALE, 0.0), (double)ADAMVS_ROOF_Q_MAX));
      b = bld[c];
    } else {
      lab = 0;                                                       // a cell without Z belongs to no run
    }
  }
  bool head;
  int end;
  wave_run(lab, j, lane, head, end);
  long long su = j, sq = q, suu = (long long)j * j, suq = (long long)j * q, lo = (q * q) & 0xFFFFF, hi = (q * q) >> 20, qmin = q, qmax = q;
  int bmax = b;
  for (int off = 1; off < 64; off <<= 1) {
    const long long t_su = __shfl_down(su, off, 64), t_sq = __shfl_down(sq, off, 64), t_suu = __shfl_down(suu, off, 64);
    const long long t_suq = __shfl_down(suq, off, 64), t_lo = __shfl_down(lo, off, 64), t_hi = __shfl_down(hi, off, 64);
    const long long t_min = __shfl_down(qmin, off, 64), t_max = __shfl_down(qmax, off, 64);
    const int t_b = __shfl_down(bmax, off, 64);
    if (lane + off <= end) {
      su += t_su, sq += t_sq, suu += t_suu, suq += t_suq, lo += t_lo, hi += t_hi;
      qmin = t_min < qmin ? t_min : qmin;
      qmax = t_max > qmax ? t_max : qmax;
      bmax = t_b > bmax ? t_b : bmax;
    }
  }
  if (!head) return;
  const long k = lab - 1;
  const long long len = end - lane + 1, v = i;
  add_nonzero(table + ADAMVS_ROOF_N * N + k, len);
  add_nonzero(table + ADAMVS_ROOF_SU * N + k, su);
  add_nonzero(table + ADAMVS_ROOF_SV * N + k, len * v);
  add_nonzero(table + ADAMVS_ROOF_SQ * N + k, sq);
  add_nonzero(table + ADAMVS_ROOF_SUU * N + k, suu);
  add_nonzero(table + ADAMVS_ROOF_SUV * N + k, su * v);
  add_nonzero(table + ADAMVS_ROOF_SVV * N + k, len * v * v);
  add_nonzero(table + ADAMVS_ROOF_SUQ * N + k, suq);
  add_nonzero(table + ADAMVS_ROOF_SVQ * N + k, sq * v);
  add_nonzero(table + ADAMVS_ROOF_SQQ_LO * N + k, lo);
  add_nonzero(table + ADAMVS_ROOF_SQQ_HI * N + k, hi);
  atomicMin(table + ADAMVS_ROOF_ROW_MIN * N + k, v);
  atomicMax(table + ADAMVS_ROOF_ROW_MAX * N + k, v);
  atomicMin(table + ADAMVS_ROOF_COL_MIN * N + k, (long long)j);
  atomicMax(table + ADAMVS_ROOF_COL_MAX * N + k, (long long)j + len - 1);
  atomicMin(table + ADAMVS_ROOF_Q_MIN * N + k, qmin);
  atomicMax(table + ADAMVS_ROOF_Q_MAX_COL * N + k, qmax);
  atomicMax(table + ADAMVS_ROOF_BUILDING * N + k, (long long)bmax);
}

// ---- growth -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double roof_error(const double* __restrict__ planes, int p, double zr, int i, int j) {
  const double* pl = planes + 3L * (p - 1);
  return fabs(zr - ((pl[0] * (double)j + pl[1] * (double)i) + pl[2]));
}

// 16 waves per workgroup: the cells labelled are summed in LDS and one lane adds them to the round's counter.  With one add per
// wave the rounds that label a whole rim (a few cells in each of many waves) waited on that one address.
constexpr int ROOF_GROW_THREADS = 1024;

__global__ __launch_bounds__(ROOF_GROW_THREADS) void k_roof_grow(int W, int H, const float* __restrict__ dsm, const int* __restrict__ bld,
                                                                 double z_ref, long P, const double* __restrict__ planes, double assign_tol,
                                                                 const int* __restrict__ src, int* __restrict__ dst, unsigned* count) {
  __shared__ unsigned s_taken;
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * ROOF_GROW_THREADS + threadIdx.x;
  bool taken = false;
  if (threadIdx.x == 0) s_taken = 0;
  __syncthreads();
  if (c < n) {
    int lab = src[c];
    const int b = lab == 0 ? bld[c] : 0;                             // a labelled cell is copied: 8 bytes; off the buildings: 12
    const float fz = b > 0 ? dsm[c] : 0.0f;
    if (lab == 0 && b > 0 && __builtin_isfinite(fz)) {
      int i, j;
      cell_ij(c, W, i, j);
      const double zr = (double)fz - z_ref;
      double best_e = INFINITY;
      int best_p = 0;
      const int di[4] = {-1, 0, 0, 1}, dj[4] = {0, -1, 1, 0};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int ii = i + di[d], jj = j + dj[d];
        if (ii < 0 || ii >= H || jj < 0 || jj >= W) continue;
        const long cn = (long)ii * W + jj;
        const int p = src[cn];
        if (p < 1 || (long)p > P || bld[cn] != b) continue;
        const double e = roof_error(planes, p, zr, i, j);
        if (e < best_e || (e == best_e && p < best_p)) best_e = e, best_p = p;      // a NaN e is never taken
      }
      if (best_p && best_e <= assign_tol) lab = best_p, taken = true;
    }
    dst[c] = lab;
  }
  const unsigned long long bal = __ballot(taken);                    // every lane of the workgroup arrives here
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&s_taken, (unsigned)__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0 && s_taken) atomicAdd(count, s_taken);
}

// ---- residuals --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_roof_residuals(int W, int H, const float* __restrict__ dsm, const int* __restrict__ label,
                                                                double z_ref, long R, const double* __restrict__ planes, double assign_tol,
                                                                long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;       // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int lab = 0, j = 0;
  unsigned inl = 0;
  long long worst = 0;
  if (c < n) {
    lab = label[c];
    if (lab < 1 || (long)lab > R) lab = 0;
  }
  if (__ballot(lab != 0) == 0ull) return;
  if (lab) {
    const float fz = dsm[c];
    if (__builtin_isfinite(fz)) {
      int i;
      cell_ij(c, W, i, j);
      const double e = roof_error(planes, lab, (double)fz - z_ref, i, j);
      inl = e <= assign_tol ? 1u : 0u;
      worst = e != e ? 1048576LL : llrint(fmin(e * 1024.0, 1048576.0));
    } else {
      lab = 0;
    }
  }
  bool head;
  int end;
  wave_run(lab, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t_inl = __shfl_down(inl, off, 64);
    const long long t_worst = __shfl_down(worst, off, 64);
    if (lane + off <= end) {
      inl += t_inl;
      worst = t_worst > worst ? t_worst : worst;
    }
  }
  if (!head) return;
  add_nonzero(table + (lab - 1), (long long)inl);
  atomicMax(table + R + (lab - 1), worst);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// Workspace of _roof_label: a control block (256 B), then the pairs of a round (at most W H / 32 pairs of 8 bytes).
long roof_workspace_bytes(int W, int H) { return 256 + align256(8 * bld_pairs_count(W, H, nullptr)) + 256; }

int launch_roof_links(int W, int H, const float* dsm, const int* building, int s, double smooth_tol, double g_tol, double step_tol,
                      uint8_t* link, hipStream_t st) {
  hipLaunchKernelGGL(k_roof_links, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, dsm, building, s, smooth_tol, g_tol,
                     step_tol, link);
  ADAMVS_CHECK_LAUNCH("roof_links");
  return 0;
}

int launch_roof_label(int W, int H, const uint8_t* link, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st) {
  return launch_label<LinkEdges>(W, H, link, workspace, parent, stats, st);
}

int launch_roof_moments(int W, int H, const float* dsm, const int* label, const int* building, double z_ref, long N, long long* table,
                        hipStream_t st) {
  if (N == 0) return 0;
  const TableStart start = TableStart(ADAMVS_ROOF_COLUMNS)
                               .set(TABLE_MIN_START, {ADAMVS_ROOF_ROW_MIN, ADAMVS_ROOF_COL_MIN, ADAMVS_ROOF_Q_MIN})
                               .set(-1, {ADAMVS_ROOF_ROW_MAX, ADAMVS_ROOF_COL_MAX, ADAMVS_ROOF_Q_MAX_COL, ADAMVS_ROOF_BUILDING});
  if (int rc = launch_table_init("roof_moments_init", N, start, table, st)) return rc;
  hipLaunchKernelGGL(k_roof_moments, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, dsm, label, building, z_ref, N, table);
  ADAMVS_CHECK_LAUNCH("roof_moments");
  return 0;
}

int launch_roof_grow(int W, int H, const float* dsm, const int* building, double z_ref, long P, const double* planes, double assign_tol,
                     int round0, int rounds, int* label0, int* label1, unsigned* counts, hipStream_t st) {
  if (rounds == 0) return 0;
  const hipError_t e = hipMemsetAsync(counts + round0, 0, sizeof(unsigned) * rounds, st);
  if (e != hipSuccess) return set_error((int)e, "roof_grow: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)(((long)W * H + ROOF_GROW_THREADS - 1) / ROOF_GROW_THREADS);
  for (int k = round0; k < round0 + rounds; ++k) {
    hipLaunchKernelGGL(k_roof_grow, dim3(blocks), dim3(ROOF_GROW_THREADS), 0, st, W, H, dsm, building, z_ref, P, planes, assign_tol,
                       (const int*)((k & 1) ? label1 : label0), (k & 1) ? label0 : label1, counts + k);
    ADAMVS_CHECK_LAUNCH("roof_grow");
  }
  return 0;
}

int launch_roof_residuals(int W, int H, const float* dsm, const int* label, double z_ref, long R, const double* planes, double assign_tol,
                          long long* table, hipStream_t st) {
  if (R == 0) return 0;
  const hipError_t e = hipMemsetAsync(table, 0, sizeof(long long) * 2 * R, st);
  if (e != hipSuccess) return set_error((int)e, "roof_residuals: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_roof_residuals, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, dsm, label, z_ref, R, planes, assign_tol,
                     table);
  ADAMVS_CHECK_LAUNCH("roof_residuals");
  return 0;
}

}  // namespace adamvs
