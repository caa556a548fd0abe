// Roof planes: link bits between adjacent cells of a building, the segments they connect, integer moments per label, the
// growth rounds into the unassigned rims and the residuals of the final planes.
// include/adamvs_hip.h "Roof planes" states the result; this file computes it with these kernels:
//
//   k_roof_links        one lane per cell: whether the cell, its east and its south neighbour are core, their gradients, and the
//                       two link tests.  The neighbours at the stride s are read straight from global memory: for the 64 cells
//                       of a wave each offset is one contiguous 256-byte piece of another row, and the rows i - s .. i + s + 1
//                       stay in L2 between the workgroups that share them.  What dsm_buildings.hip says of k_bld_flags against a
//                       tile with halo in LDS holds here unchanged (at s = 64 the halo is eight times the tile).
//   k_roof_tile         k_bld_tile with edges in place of the mask.  A wave takes a row: the ballots of the core and east bits
//                       give the edges of the row (bit k: cells k and k + 1 are joined), and a lane's run starts after the
//                       nearest lane to its left whose edge is missing.  The south edges of a row are kept as one ballot word
//                       in LDS; the passes over the vertical neighbours union only where that edge exists.  The bounds of
//                       k_bld_tile hold: every pass that changes something takes a root away.
//   k_roof_pairs        one round's first kernel over the tile-border pairs: as k_bld_pairs, and only for pairs whose link bit is
//                       set.  The round's hook and compress kernels and the final walk are the building stage's (bld_union.h).
//   k_roof_moments      one lane per cell; the lanes of a wave that follow one another within a row with the same label (and a
//                       finite Z) form a run, a segmented shuffle reduction sums the run into its first lane, which issues the
//                       integer atomics.
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
  const int i = (int)((unsigned)c / (unsigned)W), j = (int)((unsigned)c - (unsigned)i * (unsigned)W);      // n <= 2^28
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

// ---- segments: the tile phase -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_roof_tile(int W, int H, int tiles_x, const uint8_t* __restrict__ link,
                                                           int* __restrict__ parent) {
  __shared__ int s_l[BLD_CELLS];
  __shared__ unsigned long long s_south[BLD_TILE_H];                 // bit k of row r: cells (r, k) and (r + 1, k) are joined
  __shared__ int s_changed;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = tx * BLD_TILE_W + lane;
  for (int r = wv; r < BLD_TILE_H; r += BLD_THREADS / 64) {          // wave-uniform: every lane takes part in the ballots
    const int i = ty * BLD_TILE_H + r;
    const bool in = i < H && j < W;
    const uint8_t f = in ? link[(long)i * W + j] : (uint8_t)0;
    const bool core = (f & 1) != 0;
    const bool below = core && (f & 4) && r + 1 < BLD_TILE_H && i + 1 < H && (link[(long)(i + 1) * W + j] & 1);
    const unsigned long long cb = __ballot(core);
    const unsigned long long edges = __ballot(core && (f & 2)) & (cb >> 1);      // bit k: cells k and k + 1 of this row are joined
    const unsigned long long sb = __ballot(below);
    const unsigned long long gaps_below = ~edges & ((1ull << lane) - 1ull);
    const int start = gaps_below ? 64 - __clzll((long long)gaps_below) : 0;      // the cell after the nearest missing edge on the left
    s_l[r * BLD_TILE_W + lane] = core ? r * BLD_TILE_W + start : -1;
    if (lane == 0) s_south[r] = sb;
  }
  __syncthreads();
  for (int pass = 0; pass < BLD_CELLS; ++pass) {                     // fewer passes than cells: see the head of dsm_buildings.hip
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
    for (int r = wv ? wv : BLD_THREADS / 64; r < BLD_TILE_H; r += BLD_THREADS / 64) {
      const int k = r * BLD_TILE_W + lane;
      if ((s_south[r - 1] >> lane) & 1ull) {                         // both cells are core
        const int a = bld_find(s_l, k), b = bld_find(s_l, k - BLD_TILE_W);
        if (a != b) {
          atomicMin(&s_l[a > b ? a : b], a > b ? b : a);
          s_changed = 1;
        }
      }
    }
    __syncthreads();
    const int changed = s_changed;
    __syncthreads();                                                 // before lane 0 clears it again
    if (!changed) break;
  }
  for (int r = wv; r < BLD_TILE_H; r += BLD_THREADS / 64) {
    const int i = ty * BLD_TILE_H + r;
    if (i >= H || j >= W) continue;
    const int k = r * BLD_TILE_W + lane;
    int out = -1;
    if (bld_lds_load(s_l + k) >= 0) {
      const int root = bld_find(s_l, k);
      out = (int)((long)(ty * BLD_TILE_H + root / BLD_TILE_W) * W + tx * BLD_TILE_W + root % BLD_TILE_W);
    }
    parent[(long)i * W + j] = out;
  }
}

// ---- segments: the border rounds --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_roof_pairs(int W, int H, long n_vertical, long n_pairs, const uint8_t* __restrict__ link,
                                                            const int* __restrict__ parent, int2* __restrict__ pairs,
                                                            unsigned* __restrict__ changed) {
  const long p = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  long a, b;
  bld_pair_cells(p, W, H, n_vertical, a, b);
  int2 out = make_int2(-1, -1);
  if (link[a] & (p < n_vertical ? 2 : 4)) {
    const int pa = parent[a], pb = parent[b];                        // both >= 0 iff both cells are core
    if (pa >= 0 && pb >= 0) {
      const int ra = bld_root(parent, pa), rb = bld_root(parent, pb);
      if (ra != rb) {
        out = make_int2(ra < rb ? ra : rb, ra < rb ? rb : ra);
        changed[0] = 1u;
      }
    }
  }
  pairs[p] = out;
}

// ---- runs of equal labels in a wave ------------------------------------------------------------------------------------------
// head: this lane starts a run; end: the last lane of this lane's run.  Every lane of the wave calls it.
__device__ __forceinline__ void roof_run(int lab, int j, int lane, bool& head, int& end) {
  const int before = __shfl_up(lab, 1, 64);
  head = lab && (lane == 0 || before != lab || j == 0);
  const unsigned long long breaks = __ballot(head || !lab);
  const unsigned long long above = lane == 63 ? 0ull : breaks & ~((2ull << lane) - 1ull);
  end = above ? __ffsll((long long)above) - 2 : 63;
}

__device__ __forceinline__ void roof_add(long long* p, long long v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// ---- moments ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_roof_moments_init(long N, long long* __restrict__ table) {
  const long k = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (k >= N) return;
  for (int col = 0; col < ADAMVS_ROOF_COLUMNS; ++col) {
    long long v = 0;
    if (col == ADAMVS_ROOF_ROW_MIN || col == ADAMVS_ROOF_COL_MIN || col == ADAMVS_ROOF_Q_MIN) v = 0x7fffffffLL;
    if (col == ADAMVS_ROOF_ROW_MAX || col == ADAMVS_ROOF_COL_MAX || col == ADAMVS_ROOF_Q_MAX_COL || col == ADAMVS_ROOF_BUILDING) v = -1;
    table[col * N + k] = v;
  }
}

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
      i = (int)((unsigned)c / (unsigned)W);                          // n <= 2^28: 32-bit division
      j = (int)((unsigned)c - (unsigned)i * (unsigned)W);
      q = llrint(fmin(fmax(((double)fz - z_ref) * (double)ADAMVS_ROOF_Q_SCALE, 0.0), (double)ADAMVS_ROOF_Q_MAX));
      b = bld[c];
    } else {
      lab = 0;                                                       // a cell without Z belongs to no run
    }
  }
  bool head;
  int end;
  roof_run(lab, j, lane, head, end);
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
  roof_add(table + ADAMVS_ROOF_N * N + k, len);
  roof_add(table + ADAMVS_ROOF_SU * N + k, su);
  roof_add(table + ADAMVS_ROOF_SV * N + k, len * v);
  roof_add(table + ADAMVS_ROOF_SQ * N + k, sq);
  roof_add(table + ADAMVS_ROOF_SUU * N + k, suu);
  roof_add(table + ADAMVS_ROOF_SUV * N + k, su * v);
  roof_add(table + ADAMVS_ROOF_SVV * N + k, len * v * v);
  roof_add(table + ADAMVS_ROOF_SUQ * N + k, suq);
  roof_add(table + ADAMVS_ROOF_SVQ * N + k, sq * v);
  roof_add(table + ADAMVS_ROOF_SQQ_LO * N + k, lo);
  roof_add(table + ADAMVS_ROOF_SQQ_HI * N + k, hi);
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
      const int i = (int)((unsigned)c / (unsigned)W), j = (int)((unsigned)c - (unsigned)i * (unsigned)W);
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
      const int i = (int)((unsigned)c / (unsigned)W);
      j = (int)((unsigned)c - (unsigned)i * (unsigned)W);
      const double e = roof_error(planes, lab, (double)fz - z_ref, i, j);
      inl = e <= assign_tol ? 1u : 0u;
      worst = e != e ? 1048576LL : llrint(fmin(e * 1024.0, 1048576.0));
    } else {
      lab = 0;
    }
  }
  bool head;
  int end;
  roof_run(lab, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned t_inl = __shfl_down(inl, off, 64);
    const long long t_worst = __shfl_down(worst, off, 64);
    if (lane + off <= end) {
      inl += t_inl;
      worst = t_worst > worst ? t_worst : worst;
    }
  }
  if (!head) return;
  roof_add(table + (lab - 1), (long long)inl);
  atomicMax(table + R + (lab - 1), worst);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// Workspace of _roof_label: a control block (256 B), then the pairs of a round (at most W H / 32 pairs of 8 bytes).
long roof_workspace_bytes(int W, int H) { return 256 + ((8 * bld_pairs_count(W, H, nullptr) + 255) & ~255L) + 256; }

int launch_roof_links(int W, int H, const float* dsm, const int* building, int s, double smooth_tol, double g_tol, double step_tol,
                      uint8_t* link, hipStream_t st) {
  hipLaunchKernelGGL(k_roof_links, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, dsm, building, s, smooth_tol, g_tol,
                     step_tol, link);
  ADAMVS_CHECK_LAUNCH("roof_links");
  return 0;
}

int launch_roof_label(int W, int H, const uint8_t* link, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st) {
  const long n = (long)W * H;
  const int tiles_x = cdiv(W, BLD_TILE_W), tiles_y = cdiv(H, BLD_TILE_H);
  long n_vertical = 0;
  const long n_pairs = bld_pairs_count(W, H, &n_vertical);
  unsigned* changed = (unsigned*)workspace;
  int2* pairs = (int2*)((char*)workspace + 256);
  memset(stats, 0, sizeof(*stats));
  stats->tiles = (long)tiles_x * tiles_y;
  stats->pairs = n_pairs;
  BldClock clock;
  clock.mark(0, st);
  hipLaunchKernelGGL(k_roof_tile, dim3((unsigned)stats->tiles), dim3(BLD_THREADS), 0, st, W, H, tiles_x, link, parent);
  ADAMVS_CHECK_LAUNCH("roof_tile");
  clock.mark(1, st);
  bool open = n_pairs > 0;                               // whether the last look found a pair with two roots
  while (open) {
    unsigned host = 0;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return set_error((int)e, "roof_label: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_roof_pairs, dim3(bld_blocks(n_pairs)), dim3(BLD_THREADS), 0, st, W, H, n_vertical, n_pairs, link, (const int*)parent,
                       pairs, changed);
    ADAMVS_CHECK_LAUNCH("roof_pairs");
    e = hipMemcpyAsync(&host, changed, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "roof_label: %s", hipGetErrorString(e));
    open = host != 0;
    if (!open || stats->rounds == ADAMVS_BLD_MAX_ROUNDS) break;
    if (int rc = launch_bld_hook(n_pairs, n, pairs, parent, st)) return rc;
    if (int rc = launch_bld_compress(W, H, n_vertical, n_pairs, parent, st)) return rc;
    ++stats->rounds;
  }
  if (open) return set_error(ADAMVS_BLD_NOT_CONVERGED, "roof_label: tile borders still open after %d rounds", ADAMVS_BLD_MAX_ROUNDS);
  clock.mark(2, st);
  if (int rc = launch_bld_compress_all(n, parent, st)) return rc;
  clock.mark(3, st);
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "roof_label: %s", hipGetErrorString(e));
  stats->ms_tile = clock.ms(0);
  stats->ms_rounds = clock.ms(1);
  stats->ms_compress = clock.ms(2);
  stats->converged = 1;
  return 0;
}

int launch_roof_moments(int W, int H, const float* dsm, const int* label, const int* building, double z_ref, long N, long long* table,
                        hipStream_t st) {
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_roof_moments_init, dim3(bld_blocks(N)), dim3(BLD_THREADS), 0, st, N, table);
  ADAMVS_CHECK_LAUNCH("roof_moments_init");
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
