// Building extraction on the nDSM: candidate mask, flatness flags, 4-connected component labels and the per-component table.
// include/adamvs_hip.h "Building extraction" states the result; this file computes it with these kernels:
//
//   k_bld_mask          M0 as a 0.0 / 1.0 raster (the opening of dsm_dtm.hip runs on it unchanged)
//   k_bld_flags         one lane per cell: the flag 0 .. 4.  The neighbours at the stride s are read straight from global
//                       memory: for the 64 cells of a wave each of the eight offsets is one contiguous 256-byte piece of
//                       another row, and the rows i - s .. i + s (at most 129 W floats, 1.3 MB at W = 2562) stay in L2
//                       between the workgroups that share them.  A tile with halo in LDS was not built: at s = 64 the halo of
//                       a 64 x 64 tile is eight times the tile, loaded to use nine points per cell.
//   k_bld_tile          one workgroup per BLD_TILE_W x BLD_TILE_H tile, all of it in LDS.  A wave takes a row: the ballot of
//                       the mask gives every lane the first cell of its run, which is its first label.  Then passes over the
//                       vertical neighbours: both cells walk to their roots, the larger root gets atomicMin(smaller) (LDS),
//                       until a pass finds no pair with two roots.  Every such pass takes a root away, so there are fewer
//                       passes than cells; the loop is bounded by that count.  A label only ever points to a smaller index
//                       of the same component, so every walk ends.  Written: the global index of the tile-local root.
//   k_bld_pairs /       one round over the pairs of adjacent cells either side of a tile border.  _pairs reads both parents
//   k_bld_hook /        (roots: the tile phase and _compress leave border cells flat) and stores (smaller, larger) where they
//   k_bld_compress      differ; _hook does atomicMin(parent[larger], smaller); _compress walks both cells of every pair to the
//                       root (block_prims.h compress_to_root).  Three launches, so that the reads of a round see the state the
//                       previous round left: the per-XCD L2s are not coherent for plain loads inside one kernel.  The host
//                       reads one word per round and stops at the first round without a differing pair, or at the cap.
//   k_bld_compress_all  every cell to its root: the smallest cell index of its component.
//   k_bld_table         one lane per cell.  The lanes of a wave that follow one another within a row and carry the same label
//                       form a run; a segmented shuffle reduction sums the run into its first lane, which issues the ten
//                       integer atomics.  A roof of 10^5 cells sends about 1600 of each instead of 10^5.  A wave whose cells
//                       all lie outside the mask leaves after reading its labels.
//
// parent[x] <= x holds throughout, a hook joins only cells of one component, and the rounds end only when every border pair
// has one root: then each component has a single root, its smallest cell.  atomicMin / atomicMax / integer atomicAdd commute,
// so flags, labels and the table are bit-identical from run to run.
#include <math.h>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"

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
  const int i = (int)((unsigned)c / (unsigned)W), j = (int)((unsigned)c - (unsigned)i * (unsigned)W);      // n <= 2^28
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

// ---- labels: the tile phase -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLD_THREADS) void k_bld_tile(int W, int H, int tiles_x, const uint8_t* __restrict__ flags,
                                                          int* __restrict__ parent) {
  __shared__ int s_l[BLD_CELLS];
  __shared__ int s_changed;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = tx * BLD_TILE_W + lane;
  for (int r = wv; r < BLD_TILE_H; r += BLD_THREADS / 64) {          // wave-uniform: every lane takes part in the ballot
    const int i = ty * BLD_TILE_H + r;
    const bool fg = i < H && j < W && flags[(long)i * W + j] >= 2;
    const unsigned long long bal = __ballot(fg);
    const unsigned long long gaps_below = ~bal & ((1ull << lane) - 1ull);
    const int start = gaps_below ? 64 - __clzll((long long)gaps_below) : 0;      // the cell after the nearest gap on the left
    s_l[r * BLD_TILE_W + lane] = fg ? r * BLD_TILE_W + start : -1;
  }
  __syncthreads();
  for (int pass = 0; pass < BLD_CELLS; ++pass) {                     // fewer passes than cells: see the head of the file
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
    for (int r = wv ? wv : BLD_THREADS / 64; r < BLD_TILE_H; r += BLD_THREADS / 64) {
      const int k = r * BLD_TILE_W + lane;
      if (bld_lds_load(s_l + k) >= 0 && bld_lds_load(s_l + k - BLD_TILE_W) >= 0) {                 // the sign of an entry never changes
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

// ---- labels: the border rounds ----------------------------------------------------------------------------------------------
// The pairs and their order, and the walk to a root: bld_union.h (shared with dsm_roofs.hip).
__global__ __launch_bounds__(BLD_THREADS) void k_bld_pairs(int W, int H, long n_vertical, long n_pairs, const int* __restrict__ parent,
                                                           int2* __restrict__ pairs, unsigned* __restrict__ changed) {
  const long p = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  long a, b;
  bld_pair_cells(p, W, H, n_vertical, a, b);
  int2 out = make_int2(-1, -1);
  const int pa = parent[a], pb = parent[b];
  if (pa >= 0 && pb >= 0) {
    const int ra = bld_root(parent, pa), rb = bld_root(parent, pb);
    if (ra != rb) {
      out = make_int2(ra < rb ? ra : rb, ra < rb ? rb : ra);
      changed[0] = 1u;
    }
  }
  pairs[p] = out;
}

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
__global__ __launch_bounds__(BLD_THREADS) void k_bld_table_init(long N, long long* __restrict__ table) {
  const long k = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (k >= N) return;
  for (int col = 0; col < ADAMVS_BLD_COLUMNS; ++col) {
    long long v = 0;
    if (col == ADAMVS_BLD_ROW_MIN || col == ADAMVS_BLD_COL_MIN) v = 0x7fffffffLL;
    if (col == ADAMVS_BLD_ROW_MAX || col == ADAMVS_BLD_COL_MAX) v = -1;
    table[col * N + k] = v;
  }
}

__device__ __forceinline__ void bld_add(long long* p, long long v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
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
      i = (int)((unsigned)c / (unsigned)W);                          // n <= 2^28: 32-bit division
      j = (int)((unsigned)c - (unsigned)i * (unsigned)W);
      const uint8_t f = flags[c];
      counts = (f == 3 ? 1u : 0u) | (f == 4 ? 1u << 8 : 0u) | (f == 2 ? 1u << 16 : 0u);
      const float v = ndsm[c];
      top = __float_as_uint(v);
      height = (unsigned long long)llrint(fmin((double)v, 65535.0) * 1024.0);
    }
  }
  const int before = __shfl_up(lab, 1, 64);
  const bool head = lab && (lane == 0 || before != lab || j == 0);
  const unsigned long long breaks = __ballot(head || !lab);
  const unsigned long long above = lane == 63 ? 0ull : breaks & ~((2ull << lane) - 1ull);
  const int end = above ? __ffsll((long long)above) - 2 : 63;         // the last lane of this lane's run
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
  bld_add(table + ADAMVS_BLD_CELLS * N + k, len);
  bld_add(table + ADAMVS_BLD_SMOOTH * N + k, counts & 255u);
  bld_add(table + ADAMVS_BLD_ROUGH * N + k, (counts >> 8) & 255u);
  bld_add(table + ADAMVS_BLD_UNDETERMINED * N + k, (counts >> 16) & 255u);
  bld_add(table + ADAMVS_BLD_HEIGHT_SUM * N + k, (long long)height);
  atomicMin(table + ADAMVS_BLD_ROW_MIN * N + k, (long long)i);
  atomicMax(table + ADAMVS_BLD_ROW_MAX * N + k, (long long)i);
  atomicMin(table + ADAMVS_BLD_COL_MIN * N + k, (long long)j);
  atomicMax(table + ADAMVS_BLD_COL_MAX * N + k, (long long)(j + len - 1));
  atomicMax(table + ADAMVS_BLD_HEIGHT_MAX_BITS * N + k, (long long)top);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static long bld_align(long b) { return (b + 255) & ~255L; }

// Workspace: a control block (256 B), then either [m0 | m | the opening's workspace] (_bld_flags) or the pairs of a round
// (_bld_label: at most W H / 32 pairs of 8 bytes, far below the rasters).
long bld_workspace_bytes(int W, int H) { return 256 + 2 * bld_align(4L * W * H) + dtm_workspace_bytes(W, H); }

int launch_bld_flags(int W, int H, const float* dsm, const float* ndsm, double min_height, int r_open, int s, double smooth_tol,
                     void* workspace, uint8_t* flags, hipStream_t st) {
  const long n = (long)W * H;
  char* base = (char*)workspace;
  float* m0 = (float*)(base + 256);
  float* m = (float*)(base + 256 + bld_align(4 * n));
  void* open_ws = base + 256 + 2 * bld_align(4 * n);
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
  hipLaunchKernelGGL(k_bld_tile, dim3((unsigned)stats->tiles), dim3(BLD_THREADS), 0, st, W, H, tiles_x, flags, parent);
  ADAMVS_CHECK_LAUNCH("bld_tile");
  clock.mark(1, st);
  bool open = n_pairs > 0;                               // whether the last look found a pair with two roots
  while (open) {
    unsigned host = 0;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return set_error((int)e, "bld_label: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_bld_pairs, dim3(bld_blocks(n_pairs)), dim3(BLD_THREADS), 0, st, W, H, n_vertical, n_pairs, (const int*)parent, pairs,
                       changed);
    ADAMVS_CHECK_LAUNCH("bld_pairs");
    e = hipMemcpyAsync(&host, changed, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "bld_label: %s", hipGetErrorString(e));
    open = host != 0;
    if (!open || stats->rounds == ADAMVS_BLD_MAX_ROUNDS) break;
    if (int rc = launch_bld_hook(n_pairs, n, pairs, parent, st)) return rc;
    if (int rc = launch_bld_compress(W, H, n_vertical, n_pairs, parent, st)) return rc;
    ++stats->rounds;
  }
  if (open) return set_error(ADAMVS_BLD_NOT_CONVERGED, "bld_label: tile borders still open after %d rounds", ADAMVS_BLD_MAX_ROUNDS);
  clock.mark(2, st);
  if (int rc = launch_bld_compress_all(n, parent, st)) return rc;
  clock.mark(3, st);
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "bld_label: %s", hipGetErrorString(e));
  stats->ms_tile = clock.ms(0);
  stats->ms_rounds = clock.ms(1);
  stats->ms_compress = clock.ms(2);
  stats->converged = 1;
  return 0;
}

int launch_bld_table(int W, int H, const uint8_t* flags, const float* ndsm, const int* label, long N, long long* table, hipStream_t st) {
  if (N == 0) return 0;
  hipLaunchKernelGGL(k_bld_table_init, dim3(bld_blocks(N)), dim3(BLD_THREADS), 0, st, N, table);
  ADAMVS_CHECK_LAUNCH("bld_table_init");
  hipLaunchKernelGGL(k_bld_table, dim3(bld_blocks((long)W * H)), dim3(BLD_THREADS), 0, st, W, H, flags, ndsm, label, N, table);
  ADAMVS_CHECK_LAUNCH("bld_table");
  return 0;
}

}  // namespace adamvs
