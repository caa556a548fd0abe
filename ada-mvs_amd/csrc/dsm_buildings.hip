// Building extraction on the nDSM: candidate mask, flatness flags, 4-connected component labels and the per-component table.
// include/adamvs_hip.h "Building extraction" states the result; this file computes it with these kernels:
//
//   k_bld_mask          M0 as a 0.0 / 1.0 raster (the opening of dsm_dtm.hip runs on it unchanged)
//   k_bld_flags         one lane per cell: the flag 0 .. 4.  The neighbours at the stride s are read straight from global
//                       memory: for the 64 cells of a wave each of the eight offsets is one contiguous 256-byte piece of
//                       another row, and the rows i - s .. i + s (at most 129 W floats, 1.3 MB at W = 2562) stay in L2
//                       between the workgroups that share them.  A tile with halo in LDS was not built: at s = 64 the halo of
//                       a 64 x 64 tile is eight times the tile, loaded to use nine points per cell.
//   k_bld_tile /        bld_union.h: k_label_tile, k_label_pairs and launch_label over MaskEdges (a cell with flags >= 2 is a
//   k_bld_pairs         node, adjacent nodes are always joined).
//   k_bld_hook /        one round's second and third kernel and the final walk of every cell to its root, the smallest cell
//   k_bld_compress /    index of its component.  They do not look at the cells' bytes, so both labellings launch these
//   k_bld_compress_all  (bld_union.h says why a round is three launches).
//   k_bld_table         one lane per cell.  A run of equal labels (raster_prims.h wave_run) is summed into its first lane,
//                       which issues the ten integer atomics.  A wave whose cells all lie outside the mask leaves after
//                       reading its labels.
//   k_table_init        the start values of a per-label table, for this stage, the roofs and the trees (raster_prims.h).
//
// atomicMin / atomicMax / integer atomicAdd commute, so flags, labels and the table are bit-identical from run to run.
#include <math.h>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

// ---- mask and flags ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_bld_mask(long n, const float* __restrict__ ndsm, double min_height,
                                                          float* __restrict__ m0) {
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (c >= n) return;
  const float v = ndsm[c];
  m0[c] = (__builtin_isfinite(v) && (double)v >= min_height) ? 1.0f : 0.0f;
}

__global__ __launch_bounds__(BLD_THREADS) void k_bld_flags(int W, int H, const float* __restrict__ dsm, const float* __restrict__ m0,
                                                           const float* __restrict__ m, int s, double tol,
                                                           uint8_t* __restrict__ flags) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (c >= n) return;
  if (m[c] != 1.0f) {
    flags[c] = m0[c] == 1.0f ? 1 : 0;
    return;
  }
  int i, j;
  cell_ij(c, W, i, j);
  const double two_zc = 2.0 * (double)dsm[c];
  int counting = 0;
  bool rough = false;
  const int di[4] = {0, 1, 1, 1}, dj[4] = {1, 0, 1, -1};
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int ia = i - s * di[d], ja = j - s * dj[d], ib = i + s * di[d], jb = j + s * dj[d];
    if (ia < 0 || ib >= H || ja < 0 || ja >= W || jb < 0 || jb >= W) continue;
    const long ca = (long)ia * W + ja, cb = (long)ib * W + jb;
    if (m[ca] != 1.0f || m[cb] != 1.0f) continue;
    const float za = dsm[ca], zb = dsm[cb];
    if (!__builtin_isfinite(za) || !__builtin_isfinite(zb)) continue;
    const double D = fabs(((double)za + (double)zb) - two_zc);
    ++counting;
    if (!(D <= tol)) rough = true;
  }
  flags[c] = counting == 0 ? 2 : (rough ? 4 : 3);
}

// ---- labels: what a round of either labelling launches after its pairs kernel (bld_union.h) ----------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_bld_hook(long n_pairs, long n, const int2* __restrict__ pairs, int* parent) {
  const long p = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  const int2 e = pairs[p];
  if (e.x >= 0 && e.x < e.y && (long)e.y < n) atomicMin(parent + e.y, e.x);
}

__global__ __launch_bounds__(BLD_THREADS) void k_bld_compress(int W, int H, long n_vertical, long n_pairs, int* parent) {
  const long p = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  long a, b;
  bld_pair_cells(p, W, H, n_vertical, a, b);
  compress_to_root(parent, a);
  compress_to_root(parent, b);
}

__global__ __launch_bounds__(BLD_THREADS) void k_bld_compress_all(long n, int* parent) {
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (c < n) compress_to_root(parent, c);
}

// ---- the table --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_table_init(long N, const TableStart start, long long* __restrict__ table) {
  const long k = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (k >= N) return;
  for (int col = 0; col < start.columns; ++col) table[col * N + k] = start.start[col];
}

__global__ __launch_bounds__(BLD_THREADS) void k_bld_table(int W, int H, const uint8_t* __restrict__ flags, const float* __restrict__ ndsm,
                                                           const int* __restrict__ label, long N, long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * BLD_THREADS + threadIdx.x;       // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int lab = 0, i = 0, j = 0;
  unsigned counts = 0, top = 0;                                      // smooth | rough << 8 | undetermined << 16: a run has <= 64 cells
  unsigned long long height = 0;
  if (c < n) {
    lab = label[c];
    if (lab < 1 || (long)lab > N) lab = 0;
  }
  if (__ballot(lab != 0) == 0ull) return;                            // wave-uniform: a wave over empty cells adds nothing
  if (c < n) {
    if (lab) {
      cell_ij(c, W, i, j);
      const uint8_t f = flags[c];
      counts = (f == 3 ? 1u : 0u) | (f == 4 ? 1u << 8 : 0u) | (f == 2 ? 1u << 16 : 0u);
      const float v = ndsm[c];
      top = __float_as_uint(v);
      height = (unsigned long long)llrint(fmin((double)v, 65535.0) * 1024.0);
    }
  }
  bool head;
  int end;
  wave_run(lab, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t_counts = __shfl_down(counts, off, 64);
    const unsigned t_top = __shfl_down(top, off, 64);
    const unsigned long long t_height = (unsigned long long)__shfl_down((long long)height, off, 64);
    if (lane + off <= end) {
      counts += t_counts;
      height += t_height;
      top = t_top > top ? t_top : top;
    }
  }
  if (!head) return;
  const long k = lab - 1;
  const int len = end - lane + 1;
  add_nonzero(table + ADAMVS_BLD_CELLS * N + k, len);
  add_nonzero(table + ADAMVS_BLD_SMOOTH * N + k, counts & 255u);
  add_nonzero(table + ADAMVS_BLD_ROUGH * N + k, (counts >> 8) & 255u);
  add_nonzero(table + ADAMVS_BLD_UNDETERMINED * N + k, (counts >> 16) & 255u);
  add_nonzero(table + ADAMVS_BLD_HEIGHT_SUM * N + k, (long long)height);
  atomicMin(table + ADAMVS_BLD_ROW_MIN * N + k, (long long)i);
  atomicMax(table + ADAMVS_BLD_ROW_MAX * N + k, (long long)i);
  atomicMin(table + ADAMVS_BLD_COL_MIN * N + k, (long long)j);
  atomicMax(table + ADAMVS_BLD_COL_MAX * N + k, (long long)(j + len - 1));
  atomicMax(table + ADAMVS_BLD_HEIGHT_MAX_BITS * N + k, (long long)top);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// Workspace: a control block (256 B), then either [m0 | m | the opening's workspace] (_bld_flags) or the pairs of a round
// (_bld_label: at most W H / 32 pairs of 8 bytes, far below the rasters).
long bld_workspace_bytes(int W, int H) { return 256 + 2 * align256(4L * W * H) + dtm_workspace_bytes(W, H); }

int launch_bld_flags(int W, int H, const float* dsm, const float* ndsm, double min_height, int r_open, int s, double smooth_tol,
                     void* workspace, uint8_t* flags, hipStream_t st) {
  const long n = (long)W * H;
  char* base = (char*)workspace;
  float* m0 = (float*)(base + 256);
  float* m = (float*)(base + 256 + align256(4 * n));
  void* open_ws = base + 256 + 2 * align256(4 * n);
  hipLaunchKernelGGL(k_bld_mask, dim3(bld_blocks(n)), dim3(BLD_THREADS), 0, st, n, ndsm, min_height, m0);
  ADAMVS_CHECK_LAUNCH("bld_mask");
  if (r_open > 0) {
    if (int rc = launch_dsm_open(W, H, m0, r_open, open_ws, m, st)) return rc;
  } else {
    m = m0;
  }
  hipLaunchKernelGGL(k_bld_flags, dim3(bld_blocks(n)), dim3(BLD_THREADS), 0, st, W, H, dsm, (const float*)m0, (const float*)m, s, smooth_tol,
                     flags);
  ADAMVS_CHECK_LAUNCH("bld_flags");
  return 0;
}

// one round's second and third kernel and the final walk, for both labellings (bld_union.h)
int launch_bld_hook(long n_pairs, long n, const int2* pairs, int* parent, hipStream_t st) {
  hipLaunchKernelGGL(k_bld_hook, dim3(bld_blocks(n_pairs)), dim3(BLD_THREADS), 0, st, n_pairs, n, pairs, parent);
  ADAMVS_CHECK_LAUNCH("bld_hook");
  return 0;
}

int launch_bld_compress(int W, int H, long n_vertical, long n_pairs, int* parent, hipStream_t st) {
  hipLaunchKernelGGL(k_bld_compress, dim3(bld_blocks(n_pairs)), dim3(BLD_THREADS), 0, st, W, H, n_vertical, n_pairs, parent);
  ADAMVS_CHECK_LAUNCH("bld_compress");
  return 0;
}

int launch_bld_compress_all(long n, int* parent, hipStream_t st) {
  hipLaunchKernelGGL(k_bld_compress_all, dim3(bld_blocks(n)), dim3(BLD_THREADS), 0, st, n, parent);
  ADAMVS_CHECK_LAUNCH("bld_compress_all");
  return 0;
}

int launch_bld_label(int W, int H, const uint8_t* flags, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st) {
  return launch_label<MaskEdges>(W, H, flags, workspace, parent, stats, st);
}

int launch_table_init(const char* name, long N, const TableStart& start, long long* table, hipStream_t st) {
  hipLaunchKernelGGL(k_table_init, dim3(bld_blocks(N)), dim3(BLD_THREADS), 0, st, N, start, table);
  ADAMVS_CHECK_LAUNCH(name);
  return 0;
}

int launch_bld_table(int W, int H, const uint8_t* flags, const float* ndsm, const int* label, long N, long long* table, hipStream_t st) {
  if (N == 0) return 0;
  const TableStart start = TableStart(ADAMVS_BLD_COLUMNS)
                               .set(TABLE_MIN_START, {ADAMVS_BLD_ROW_MIN, ADAMVS_BLD_COL_MIN})
                               .set(-1, {ADAMVS_BLD_ROW_MAX, ADAMVS_BLD_COL_MAX});
  if (int rc = launch_table_init("bld_table_init", N, start, table, st)) return rc;
  hipLaunchKernelGGL(k_bld_table, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, flags, ndsm, label, N, table);
  ADAMVS_CHECK_LAUNCH("bld_table");
  return 0;
}

}  // namespace adamvs
