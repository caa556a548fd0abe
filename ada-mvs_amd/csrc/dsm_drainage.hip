// The drainage network of a height raster: the depression-free surface, D8 directions, flow accumulation with the root of every
// cell, and the stream links as ordered cell lists.  include/adamvs_hip.h "Drainage" states the result; this file computes it with
// these kernels:
//
//   k_drn_init          one lane per cell: r = s 2^(8 - 4 passes), the edge test on the eight neighbours, the start of F (r at an
//                       edge cell, INT_MAX at every other cell of V, INT_MIN outside V).
//   k_drn_relax         one workgroup per tile of DRN_T x DRN_T cells: F of the tile and a one-cell halo goes to LDS (34 x 34 words,
//                       4.6 KB); a lane owns four cells, keeps their r in registers and lowers them in place to
//                       max(r, min of the eight neighbours + 1) until a sweep of the whole workgroup lowers nothing
//                       (__syncthreads_or).  The sweeps race on purpose: the operator is monotone, every value read is one that some
//                       earlier sweep wrote and none is below the fixed point, so every schedule ends at the same integers.  The
//                       cells that fell are written back, and one word per round says whether any tile wrote.  The halo is read
//                       from global memory while other tiles of the same round may write it: a word is either the older or the
//                       newer value, both above the fixed point.  A round in which no tile writes has read a raster nobody
//                       changed: it is the fixed point.
//   k_drn_dir           one lane per cell: the steepest positive drop of F among E, SE, S, SW, W, NW, N, NE, 2 a^2 against b^2 in
//                       int64, the first of equals.
//   k_drn_acc_*         pointer doubling over the receivers, a pair (ancestor, sum) per cell, double-buffered: a round copies the
//                       sums and advances the ancestors, a second kernel adds every cell's sum to its ancestor's with an integer
//                       atomic.  ceil(log2(longest path + 1)) rounds.  A cell past its root holds ~root: the basins need no pass of
//                       their own.
//   k_drn_nd, k_raster_rank_dist, k_drn_cells, k_drn_tails, k_drn_vertices
//                       the stream cells' donors in closed form from the eight neighbours, the link heads' scan into link numbers
//                       (raster_prims.h raster_scan), the list ranking upstream (raster_prims.h, the contours' distance rounds),
//                       every cell's link and position, the tails' vertex counts and their scan, the link table and the vertices.
//
// DRN_CHUNK rounds per read-back of the changed words: a read-back is a stream synchronise (tools/drainage_bench.py: the init
// kernel, four rounds of one workgroup and one read-back take 0.101 ms, a round over 7 M cells 0.114 ms); the result does not
// depend on where the loop stops.  Integer atomics only (add),
// which commute; every other store goes to a slot that one lane owns: every output is bit-identical from run to run.  No
// workgroup waits on another.
#include <limits.h>
#include <string.h>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

constexpr int DRN_T = ADAMVS_DRAIN_TILE;
constexpr int DRN_LW = DRN_T + 2;
constexpr int DRN_THREADS = RASTER_THREADS;
constexpr int DRN_PER_LANE = DRN_T * DRN_T / DRN_THREADS;
constexpr int DRN_CHUNK = 4;
constexpr int DRN_NONE = INT_MIN;                // r, F outside V
constexpr int DRN_F_LIMIT = 1 << 30;             // |F| of a settled cell stays below
static_assert(DRN_T * DRN_T % DRN_THREADS == 0, "a lane owns whole cells");

// the control block at the head of the workspace
constexpr long DRN_OFF_CHANGED = 0;              // unsigned [RASTER_RANK_ROUNDS]: the ranking; the first DRN_CHUNK: fill, accumulation
constexpr long DRN_OFF_TOTAL = 256;              // unsigned long long: the total of the last scan
constexpr long DRN_CONTROL = 512;

// workspace: control | two (ancestor, value) buffers int2 [n + 1] (the link heads' flags lie over the second before the ranking, the
// links' vertex counts and their scan over both after it) | link numbers unsigned [n + 1] | workgroup totals and their offsets
struct DrnWs {
  int2* buf[2];
  unsigned* flag;        // over buf[1]: unsigned [n]
  unsigned* count;       // over buf[0]: unsigned [L]
  unsigned* first;       // over buf[1]: unsigned [L + 1]
  unsigned* lineno;
  unsigned* part;
  unsigned* part_off;
  long bytes;
};
static DrnWs drn_ws(void* workspace, int W, int H) {
  const long n = (long)W * H, nb = raster_blocks(n + 1);
  char* p = (char*)workspace;
  DrnWs w;
  long o = DRN_CONTROL;
  w.buf[0] = (int2*)(p + o);
  w.count = (unsigned*)(p + o);
  o += align256(8 * (n + 1));
  w.buf[1] = (int2*)(p + o);
  w.flag = (unsigned*)(p + o);
  w.first = (unsigned*)(p + o);
  o += align256(8 * (n + 1));
  w.lineno = (unsigned*)(p + o);
  o += align256(4 * (n + 1));
  w.part = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.part_off = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.bytes = o;
  return w;
}
long drain_workspace_bytes(int W, int H) { return drn_ws(nullptr, W, H).bytes; }

// ---- the eight neighbours in the order of the tie rule: E, SE, S, SW, W, NW, N, NE; neighbour k has the code 1 << k
__device__ __forceinline__ int drn_row_step(int k) { return (k >= 1 && k <= 3) ? 1 : (k >= 5) ? -1 : 0; }
__device__ __forceinline__ int drn_col_step(int k) { return (k <= 1 || k == 7) ? 1 : (k >= 3 && k <= 5) ? -1 : 0; }

// the receiver of cell c = (i, j) with the code d: -1 for an outlet, for no data and for a code that is no neighbour inside the grid
__device__ __forceinline__ long drn_receiver(int W, int H, int i, int j, unsigned d) {
  if (d == 0u || d == 255u || (d & (d - 1u))) return -1;
  const int k = __ffs((int)d) - 1;
  const int ii = i + drn_row_step(k), jj = j + drn_col_step(k);
  if (ii < 0 || ii >= H || jj < 0 || jj >= W) return -1;
  return (long)ii * W + jj;
}

// ---- the fill ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DRN_THREADS) void k_drn_init(int W, int H, const int* __restrict__ s, int unit, int* __restrict__ r, int* __restrict__ F) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= n) return;
  const int sv = s[c];
  if (sv == DRN_NONE) {
    r[c] = DRN_NONE;
    F[c] = DRN_NONE;
    return;
  }
  int i, j;
  cell_ij(c, W, i, j);
  bool edge = i == 0 || j == 0 || i == H - 1 || j == W - 1;
  if (!edge) {
#pragma unroll
    for (int k = 0; k < 8; ++k) edge = edge || s[c + (long)drn_row_step(k) * W + drn_col_step(k)] == DRN_NONE;
  }
  const int rv = sv * unit;                                          // |s| 65536 / S <= 8191 * 65536 < 2^29
  r[c] = rv;
  F[c] = edge ? rv : INT_MAX;
}

__global__ __launch_bounds__(DRN_THREADS) void k_drn_relax(int W, int H, int tiles_x, const int* __restrict__ r, int* F, unsigned* changed) {
  __shared__ int s_f[DRN_LW * DRN_LW];
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int i0 = ty * DRN_T, j0 = tx * DRN_T;
  for (int k = threadIdx.x; k < DRN_LW * DRN_LW; k += DRN_THREADS) {
    const int li = k / DRN_LW, lj = k - li * DRN_LW;
    const int gi = i0 - 1 + li, gj = j0 - 1 + lj;
    s_f[k] = (gi >= 0 && gi < H && gj >= 0 && gj < W) ? F[(long)gi * W + gj] : DRN_NONE;
  }
  __syncthreads();
  // a lane's cells: movable iff in V with all eight neighbours in V (what is outside the grid is DRN_NONE in LDS)
  int rv[DRN_PER_LANE], at[DRN_PER_LANE], was[DRN_PER_LANE];
  bool movable[DRN_PER_LANE];
#pragma unroll
  for (int m = 0; m < DRN_PER_LANE; ++m) {
    const int q = threadIdx.x + m * DRN_THREADS;
    const int li = q / DRN_T, lj = q - li * DRN_T;
    at[m] = (li + 1) * DRN_LW + lj + 1;
    was[m] = s_f[at[m]];
    bool mv = was[m] != DRN_NONE;
#pragma unroll
    for (int k = 0; k < 8; ++k) mv = mv && s_f[at[m] + drn_row_step(k) * DRN_LW + drn_col_step(k)] != DRN_NONE;
    movable[m] = mv;
    rv[m] = mv ? r[(long)(i0 + li) * W + j0 + lj] : 0;               // movable: inside the grid
  }
  volatile int* f = s_f;
  for (;;) {
    bool fell = false;
#pragma unroll
    for (int m = 0; m < DRN_PER_LANE; ++m) {
      if (!movable[m]) continue;
      int lo = INT_MAX;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int v = f[at[m] + drn_row_step(k) * DRN_LW + drn_col_step(k)];
        lo = v < lo ? v : lo;
      }
      const int cand = lo == INT_MAX ? INT_MAX : lo + 1;
      const int nv = cand > rv[m] ? cand : rv[m];
      if (nv < f[at[m]]) {
        f[at[m]] = nv;
        fell = true;
      }
    }
    if (!__syncthreads_or(fell ? 1 : 0)) break;
  }
  bool wrote = false;
#pragma unroll
  for (int m = 0; m < DRN_PER_LANE; ++m) {
    if (!movable[m]) continue;
    const int v = f[at[m]];
    if (v != was[m]) {
      const int q = threadIdx.x + m * DRN_THREADS;
      const int li = q / DRN_T, lj = q - li * DRN_T;
      F[(long)(i0 + li) * W + j0 + lj] = v;
      wrote = true;
    }
  }
  if (__syncthreads_or(wrote ? 1 : 0) && threadIdx.x == 0) changed[0] = 1u;
}

// ---- the directions ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DRN_THREADS) void k_drn_dir(int W, int H, const int* __restrict__ F, uint8_t* __restrict__ dir) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= n) return;
  const int fc = F[c];
  if (fc == DRN_NONE) {
    dir[c] = 255;
    return;
  }
  int i, j;
  cell_ij(c, W, i, j);
  unsigned out = 0u;
  if (i > 0 && j > 0 && i < H - 1 && j < W - 1 && fc < DRN_F_LIMIT && fc > -DRN_F_LIMIT) {
    bool edge = false;
    long long best = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int fn = F[c + (long)drn_row_step(k) * W + drn_col_step(k)];
      edge = edge || fn == DRN_NONE;
      const long long d = (long long)fc - fn;                        // < 2^31 wherever fn is a height: the squares fit
      if (fn == DRN_NONE || fn <= -DRN_F_LIMIT || d <= 0) continue;
      const long long key = (k & 1) ? d * d : 2 * d * d;             // orthogonal drop a against diagonal drop b: 2 a^2 against b^2
      if (key > best) {
        best = key;
        out = 1u << k;
      }
    }
    if (edge) out = 0u;
  }
  dir[c] = (uint8_t)out;
}

// ---- accumulation and roots -------------------------------------------------------------------------------------------------
// A pair (x, y): x >= 0 is the 2^k-th ancestor, x < 0 says that the path ended before, at the root ~x; y is the sum over the
// descendants nearer than 2^k.
__global__ __launch_bounds__(DRN_THREADS) void k_drn_acc_init(int W, int H, const uint8_t* __restrict__ dir, const int* __restrict__ value,
                                                              int2* __restrict__ st) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= n) return;
  const unsigned d = dir[c];
  int i, j;
  cell_ij(c, W, i, j);
  const long rc = drn_receiver(W, H, i, j, d);
  const bool up = rc >= 0 && dir[rc] != 255;                         // a receiver outside V is none
  st[c] = make_int2(up ? (int)rc : ~(int)c, d == 255u ? 0 : value ? value[c] : 1);
}

__global__ __launch_bounds__(DRN_THREADS) void k_drn_acc_copy(long N, const int2* __restrict__ cur, int2* __restrict__ nxt, unsigned* changed) {
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  bool moved = false;
  if (c < N) {
    int2 v = cur[c];
    if (v.x >= 0) {
      v.x = cur[v.x].x;                                              // 0 <= v.x < N by the init and by induction
      moved = true;
    }
    nxt[c] = v;
  }
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) changed[0] = 1u;
}

__global__ __launch_bounds__(DRN_THREADS) void k_drn_acc_add(long N, const int2* __restrict__ cur, int2* nxt) {
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= N) return;
  const int2 v = cur[c];
  if (v.x >= 0 && v.y) atomicAdd(&nxt[v.x].y, v.y);
}

__global__ __launch_bounds__(DRN_THREADS) void k_drn_acc_store(long N, const int2* __restrict__ res, const uint8_t* __restrict__ dir, int* __restrict__ acc,
                                                               int* __restrict__ root) {
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= N) return;
  const int2 v = res[c];
  acc[c] = v.y;
  root[c] = dir[c] == 255 ? -1 : v.x < 0 ? ~v.x : -1;                // v.x < 0 always, once the rounds have converged
}

// ---- the streams ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool drn_is_stream(const uint8_t* __restrict__ dir, const int* __restrict__ acc, long c, int min_cells) {
  return dir[c] != 255 && acc[c] >= min_cells;
}

// the stream donors of stream cell c among its neighbours: their number, and the last one found
__device__ __forceinline__ int drn_donors(int W, int H, const uint8_t* __restrict__ dir, const int* __restrict__ acc, int min_cells, long c, long* donor) {
  int i, j;
  cell_ij(c, W, i, j);
  int nd = 0;
  *donor = -1;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int ii = i + drn_row_step(k), jj = j + drn_col_step(k);
    if (ii < 0 || ii >= H || jj < 0 || jj >= W) continue;
    const long m = (long)ii * W + jj;
    if (dir[m] == (1u << ((k + 4) & 7)) && acc[m] >= min_cells) {    // it points back at c
      ++nd;
      *donor = m;
    }
  }
  return nd;
}

// nd (255 outside the streams), the flag of a link head (a head that has a receiver) and the start of the ranking
__global__ __launch_bounds__(DRN_THREADS) void k_drn_nd(int W, int H, const uint8_t* __restrict__ dir, const int* __restrict__ acc, int min_cells,
                                                        uint8_t* __restrict__ nd, unsigned* __restrict__ flag, int2* __restrict__ st) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= n) return;
  int count = 255;
  long donor = -1;
  if (drn_is_stream(dir, acc, c, min_cells)) count = drn_donors(W, H, dir, acc, min_cells, c, &donor);
  int i, j;
  cell_ij(c, W, i, j);
  nd[c] = (uint8_t)count;
  flag[c] = (count != 255 && count != 1 && drn_receiver(W, H, i, j, dir[c]) >= 0) ? 1u : 0u;
  st[c] = count == 1 ? make_int2((int)donor, 1) : make_int2(~(int)c, 0);
}

// every stream cell's link (-1 where its head heads none) and its position below the head
__global__ __launch_bounds__(DRN_THREADS) void k_drn_cells(long N, const int2* __restrict__ res, const uint8_t* __restrict__ nd,
                                                           const unsigned* __restrict__ lineno, int* __restrict__ link, int* __restrict__ pos) {
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= N) return;
  int l = -1, p = -1;
  const int2 v = res[c];
  if (nd[c] != 255 && v.x < 0) {
    const long h = ~v.x;
    if (h >= 0 && h < N && lineno[h + 1] != lineno[h]) {
      l = (int)lineno[h];
      p = v.y;
    }
  }
  link[c] = l;
  pos[c] = p;
}

// a link's last own cell: it is an outlet, or its receiver is a head
__device__ __forceinline__ bool drn_is_tail(long rc, const uint8_t* __restrict__ nd) { return rc < 0 || nd[rc] != 1; }

__global__ __launch_bounds__(DRN_THREADS) void k_drn_tails(int W, int H, long L, const uint8_t* __restrict__ dir, const uint8_t* __restrict__ nd,
                                                           const int* __restrict__ link, const int* __restrict__ pos, unsigned* __restrict__ count) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c >= n) return;
  const int l = link[c], p = pos[c];
  if (l < 0 || (long)l >= L || p < 0) return;
  int i, j;
  cell_ij(c, W, i, j);
  const long rc = drn_receiver(W, H, i, j, dir[c]);
  if (drn_is_tail(rc, nd)) count[l] = (unsigned)p + 1u + (rc >= 0 ? 1u : 0u);
}

__global__ __launch_bounds__(DRN_THREADS) void k_drn_vertices(int W, int H, long L, long P, const uint8_t* __restrict__ dir, const uint8_t* __restrict__ nd,
                                                              const int* __restrict__ link, const int* __restrict__ pos,
                                                              const unsigned* __restrict__ first, int* __restrict__ link_first,
                                                              int* __restrict__ link_head, int* __restrict__ link_end, int* __restrict__ link_to,
                                                              int* __restrict__ vertex) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * DRN_THREADS + threadIdx.x;
  if (c <= L) link_first[c] = (int)first[c];
  if (c >= n) return;
  const int l = link[c], p = pos[c];
  if (l < 0 || (long)l >= L || p < 0) return;
  const long at = (long)first[l] + p;
  if (at + 1 > P) return;                                            // keeps every store in bounds whatever the caller passed
  int i, j;
  cell_ij(c, W, i, j);
  const long rc = drn_receiver(W, H, i, j, dir[c]);
  vertex[at] = (int)c;
  if (p == 0) link_head[l] = (int)c;
  if (drn_is_tail(rc, nd)) {
    if (rc >= 0 && at + 2 <= P) vertex[at + 1] = (int)rc;
    link_end[l] = rc >= 0 ? (int)rc : (int)c;
    link_to[l] = rc >= 0 ? link[rc] : -1;                            // the junction's own link; -1 at an outlet
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// Rounds of `round(k, changed word)` until one changes nothing or `cap` have been launched: DRN_CHUNK per read-back.
template <typename Round>
static int drn_rounds(const char* name, int cap, unsigned* changed, Round round, adamvs_drain_stats* stats, hipStream_t st) {
  unsigned host[DRN_CHUNK];
  stats->rounds = stats->launched = 0;
  stats->converged = 0;
  while (stats->launched < cap && !stats->converged) {
    const int todo = cap - stats->launched < DRN_CHUNK ? cap - stats->launched : DRN_CHUNK;
    hipError_t e = hipMemsetAsync(changed, 0, sizeof(host), st);
    if (e != hipSuccess) return set_error((int)e, "%s: %s", name, hipGetErrorString(e));
    for (int k = 0; k < todo; ++k) {
      if (int rc = round(stats->launched, changed + k)) return rc;
      ++stats->launched;
    }
    e = hipMemcpyAsync(host, changed, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "%s: %s", name, hipGetErrorString(e));
    for (int k = 0; k < todo && !stats->converged; ++k) {
      if (host[k]) ++stats->rounds;
      else stats->converged = 1;     // a round that changes nothing leaves every later one without a change: the result stands
    }
  }
  return 0;
}

int launch_drain_fill(int W, int H, const int* s, int smooth_passes, int max_rounds, void* workspace, int* r, int* F, adamvs_drain_stats* stats,
                      hipStream_t st) {
  const long n = (long)W * H;
  unsigned* changed = (unsigned*)((char*)workspace + DRN_OFF_CHANGED);
  memset(stats, 0, sizeof(*stats));
  BldClock clock;
  clock.mark(0, st);
  hipLaunchKernelGGL(k_drn_init, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, W, H, s, 1 << (8 - 4 * smooth_passes), r, F);
  ADAMVS_CHECK_LAUNCH("drain_init");
  const int tiles_x = cdiv(W, DRN_T), tiles_y = cdiv(H, DRN_T);
  const auto round = [&](int, unsigned* word) {
    hipLaunchKernelGGL(k_drn_relax, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(DRN_THREADS), 0, st, W, H, tiles_x, (const int*)r, F, word);
    ADAMVS_CHECK_LAUNCH("drain_relax");
    return 0;
  };
  if (int rc = drn_rounds("drain_fill", max_rounds, changed, round, stats, st)) return rc;
  clock.mark(1, st);
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "drain_fill: %s", hipGetErrorString(e));
  stats->ms = clock.ms(0);
  return 0;
}

int launch_drain_direction(int W, int H, const int* F, uint8_t* dir, hipStream_t st) {
  hipLaunchKernelGGL(k_drn_dir, dim3(raster_blocks((long)W * H)), dim3(DRN_THREADS), 0, st, W, H, F, dir);
  ADAMVS_CHECK_LAUNCH("drain_direction");
  return 0;
}

int launch_drain_accumulate(int W, int H, const uint8_t* dir, const int* value, void* workspace, int* acc, int* root, adamvs_drain_stats* stats,
                            hipStream_t st) {
  const long n = (long)W * H;
  const DrnWs w = drn_ws(workspace, W, H);
  unsigned* changed = (unsigned*)((char*)workspace + DRN_OFF_CHANGED);
  memset(stats, 0, sizeof(*stats));
  BldClock clock;
  clock.mark(0, st);
  hipLaunchKernelGGL(k_drn_acc_init, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, W, H, dir, value, w.buf[0]);
  ADAMVS_CHECK_LAUNCH("drain_acc_init");
  int where = 0;
  const auto round = [&](int, unsigned* word) {
    hipLaunchKernelGGL(k_drn_acc_copy, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, n, (const int2*)w.buf[where], w.buf[where ^ 1], word);
    ADAMVS_CHECK_LAUNCH("drain_acc_copy");
    hipLaunchKernelGGL(k_drn_acc_add, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, n, (const int2*)w.buf[where], w.buf[where ^ 1]);
    ADAMVS_CHECK_LAUNCH("drain_acc_add");
    where ^= 1;
    return 0;
  };
  if (int rc = drn_rounds("drain_accumulate", RASTER_RANK_ROUNDS, changed, round, stats, st)) return rc;
  if (!stats->converged) return set_error(ADAMVS_DRAIN_NOT_A_FOREST, "drain_accumulate: paths still running after %d rounds (dir holds a cycle)", RASTER_RANK_ROUNDS);
  hipLaunchKernelGGL(k_drn_acc_store, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, n, (const int2*)w.buf[where], dir, acc, root);
  ADAMVS_CHECK_LAUNCH("drain_acc_store");
  clock.mark(1, st);
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "drain_accumulate: %s", hipGetErrorString(e));
  stats->ms = clock.ms(0);
  return 0;
}

static int drn_read_total(const char* name, const unsigned long long* total64, unsigned long long* total, hipStream_t st) {
  hipError_t e = hipMemcpyAsync(total, total64, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "%s: %s", name, hipGetErrorString(e));
  return 0;
}

int launch_drain_streams(int W, int H, const uint8_t* dir, const int* acc, int min_cells, void* workspace, uint8_t* nd, int* link, int* pos,
                         adamvs_drain_stats* stats, hipStream_t st) {
  const long n = (long)W * H;
  const DrnWs w = drn_ws(workspace, W, H);
  unsigned* changed = (unsigned*)((char*)workspace + DRN_OFF_CHANGED);
  unsigned long long* total64 = (unsigned long long*)((char*)workspace + DRN_OFF_TOTAL);
  memset(stats, 0, sizeof(*stats));
  BldClock clock;
  hipError_t e = hipMemsetAsync(workspace, 0, DRN_CONTROL, st);
  if (e != hipSuccess) return set_error((int)e, "drain_streams: %s", hipGetErrorString(e));
  clock.mark(0, st);
  hipLaunchKernelGGL(k_drn_nd, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, W, H, dir, acc, min_cells, nd, w.flag, w.buf[0]);
  ADAMVS_CHECK_LAUNCH("drain_nd");
  if (int rc = raster_scan("drain", n, w.flag, w.lineno, w.part, w.part_off, total64, st)) return rc;
  unsigned long long L = 0;
  if (int rc = drn_read_total("drain_streams", total64, &L, st)) return rc;
  int where = 0, moved = 0;
  bool ok = false;
  if (int rc = raster_rank_phase(k_raster_rank_dist, "drain_rank", n, w.buf, &where, changed, 0, &moved, &stats->launched, &ok, st)) return rc;
  stats->rounds = moved;
  stats->converged = ok ? 1 : 0;
  if (!ok) return set_error(ADAMVS_DRAIN_NOT_A_FOREST, "drain_streams: positions still moving after %d rounds (dir holds a cycle)", RASTER_RANK_ROUNDS);
  hipLaunchKernelGGL(k_drn_cells, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, n, (const int2*)w.buf[where], (const uint8_t*)nd,
                     (const unsigned*)w.lineno, link, pos);
  ADAMVS_CHECK_LAUNCH("drain_cells");
  unsigned long long P = 0;
  if (L) {
    e = hipMemsetAsync(w.count, 0, 4 * (long)L, st);
    if (e != hipSuccess) return set_error((int)e, "drain_streams: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(k_drn_tails, dim3(raster_blocks(n)), dim3(DRN_THREADS), 0, st, W, H, (long)L, dir, (const uint8_t*)nd, (const int*)link,
                       (const int*)pos, w.count);
    ADAMVS_CHECK_LAUNCH("drain_tails");
    if (int rc = raster_scan("drain", (long)L, w.count, w.first, w.part, w.part_off, total64, st)) return rc;
    clock.mark(1, st);
    if (int rc = drn_read_total("drain_streams", total64, &P, st)) return rc;
  } else {
    clock.mark(1, st);
    e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "drain_streams: %s", hipGetErrorString(e));
  }
  stats->links = (long)L;
  stats->vertices = (long)P;
  stats->ms = clock.ms(0);
  if (P >= (1ull << 31)) return set_error(-1, "drain_streams: %llu vertices, fewer than 2^31 can be numbered", P);
  return 0;
}

int launch_drain_links(int W, int H, const uint8_t* dir, const uint8_t* nd, const int* link, const int* pos, long L, long P, void* workspace,
                       int* link_first, int* link_head, int* link_end, int* link_to, int* vertex, hipStream_t st) {
  if (L == 0) {
    const hipError_t e = hipMemsetAsync(link_first, 0, 4, st);
    if (e != hipSuccess) return set_error((int)e, "drain_links: %s", hipGetErrorString(e));
    return 0;
  }
  const long n = (long)W * H;
  const DrnWs w = drn_ws(workspace, W, H);
  unsigned total = 0;                                                // the offsets must be those of this L and P: first[L] is their total
  hipError_t e = hipMemcpyAsync(&total, w.first + L, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "drain_links: %s", hipGetErrorString(e));
  if ((long)total != P) return set_error(-1, "drain_links: P=%ld, but the workspace holds the offsets of %u vertices (_drain_streams first)", P, total);
  hipLaunchKernelGGL(k_drn_vertices, dim3(raster_blocks(n + 1)), dim3(DRN_THREADS), 0, st, W, H, L, P, dir, nd, link, pos, (const unsigned*)w.first,
                     link_first, link_head, link_end, link_to, vertex);
  ADAMVS_CHECK_LAUNCH("drain_vertices");
  return 0;
}

}  // namespace adamvs
