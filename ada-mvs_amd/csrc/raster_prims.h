// What the raster stages (dsm_buildings.hip, dsm_roofs.hip, dsm_trees.hip, dsm_contours.hip, dsm_drainage.hip) share besides the
// labelling of bld_union.h: a cell's row and column, the runs of equal labels within a wave that the per-label tables are reduced
// over, the add that skips zeros, the start values of a table, the binomial pass over an integer raster with holes, the exclusive
// scan over a raster's cells and the distance rounds of list ranking.  Integer
// work only: the includers switch fp contraction off after their includes, and a helper that multiplies and then adds floats
// would round differently from one includer to the next (block_prims.h).
#pragma once
#include <initializer_list>

#include "block_prims.h"
#include "common.h"
#include "kernels.h"

namespace adamvs {

// Cell c of a raster W wide is (row i, column j).  Every entry point refuses n = W H > 2^28, so the division is a 32-bit one.
__device__ __forceinline__ void cell_ij(long c, int W, int& i, int& j) {
  i = (int)((unsigned)c / (unsigned)W);
  j = (int)((unsigned)c - (unsigned)i * (unsigned)W);
}

// ---- runs of equal labels in a wave -------------------------------------------------------------------------------------------
// The lanes of a wave that follow one another within a row (j is the lane's column) and carry the same label lab != 0 form a
// run.  head: this lane starts a run; end: the last lane of this lane's run.  Every lane of the wave calls it.  A segmented
// shuffle reduction (`if (lane + off <= end)`) then sums a run into its head, which issues the atomics: a component of 10^5
// cells sends about 1600 of each instead of 10^5.
__device__ __forceinline__ void wave_run(int lab, int j, int lane, bool& head, int& end) {
  const int before = __shfl_up(lab, 1, 64);
  head = lab && (lane == 0 || before != lab || j == 0);
  const unsigned long long breaks = __ballot(head || !lab);
  const unsigned long long above = lane == 63 ? 0ull : breaks & ~((2ull << lane) - 1ull);
  end = above ? __ffsll((long long)above) - 2 : 63;
}

__device__ __forceinline__ void add_nonzero(long long* p, long long v) {
  if (v) atomicAdd((unsigned long long*)p, (unsigned long long)v);
}

// ---- the start of a table ---------------------------------------------------------------------------------------------------
// table[col * N + k] = start[col] for k < N: 0 for a sum, TABLE_MIN_START for a minimum, -1 for a maximum.  The kernel is in
// dsm_buildings.hip; `name` is what a failed launch is reported under.
constexpr int TABLE_MAX_COLUMNS = 18;
constexpr long long TABLE_MIN_START = 0x7fffffffLL;
static_assert(ADAMVS_BLD_COLUMNS <= TABLE_MAX_COLUMNS && ADAMVS_ROOF_COLUMNS <= TABLE_MAX_COLUMNS && ADAMVS_TREE_COLUMNS <= TABLE_MAX_COLUMNS,
              "TableStart holds every table's columns");
struct TableStart {
  int columns;
  long long start[TABLE_MAX_COLUMNS];
  explicit TableStart(int n, long long fill = 0) : columns(n) {
    for (long long& v : start) v = fill;
  }
  TableStart& set(long long v, std::initializer_list<int> cols) {
    for (int c : cols) start[c] = v;
    return *this;
  }
};
int launch_table_init(const char* name, long N, const TableStart& start, long long* table, hipStream_t st);

// ---- the binomial pass --------------------------------------------------------------------------------------------------------
// (1 2 1) x (1 2 1) around cell c of an int32 raster with holes: a neighbour outside the grid or in a hole counts as the centre,
// a hole stays a hole.  Hole::is(v) is the "no value" test and Hole::NONE what a hole holds.  The eight neighbours come straight
// from global memory: three coalesced row segments per wave, the rows above and below re-read from L1 / L2.  The caller bounds
// |v|: the sum is 16 times a weighted mean and must fit an int.
template <class Hole>
__device__ __forceinline__ int binomial3x3(int W, int H, const int* __restrict__ src, long c) {
  const int centre = src[c];
  if (Hole::is(centre)) return Hole::NONE;
  int i, j;
  cell_ij(c, W, i, j);
  int out = 0;
#pragma unroll
  for (int di = -1; di <= 1; ++di)
#pragma unroll
    for (int dj = -1; dj <= 1; ++dj) {
      const int ii = i + di, jj = j + dj;
      int v = centre;
      if (ii >= 0 && ii < H && jj >= 0 && jj < W) {
        const int t = src[(long)ii * W + jj];
        if (!Hole::is(t)) v = t;
      }
      out += (2 - (di ? 1 : 0)) * (2 - (dj ? 1 : 0)) * v;
    }
  return out;
}

// ---- the scan -----------------------------------------------------------------------------------------------------------------
// The exclusive scan that dsm_contours.hip (block counts -> offsets, start flags -> line numbers, vertex counts -> line_first) and
// dsm_drainage.hip (link heads -> link numbers, vertex counts -> link_first) share: workgroups of 256 scan their elements with
// block_exclusive_scan, k_fusion_scan scans the workgroup totals, a third kernel adds them.  The total is also summed in 64 bits,
// so an overflow of the 32-bit offsets is seen on the host before anything reads them.
constexpr int RASTER_THREADS = 256;
static inline unsigned raster_blocks(long n) { return (unsigned)((n + RASTER_THREADS - 1) / RASTER_THREADS); }

// exclusive scan of a workgroup's 256 elements into `out`, its total into part[blockIdx.x] and into the 64-bit total
static __global__ __launch_bounds__(RASTER_THREADS) void k_raster_scan_local(long n, const unsigned* __restrict__ in, unsigned* __restrict__ out,
                                                                             unsigned* __restrict__ part, unsigned long long* total64) {
  const long c = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  const unsigned v = c < n ? in[c] : 0u;
  unsigned total;
  const unsigned ex = block_exclusive_scan(v, &total);
  if (c < n) out[c] = ex;
  if (threadIdx.x == 0) {
    part[blockIdx.x] = total;
    if (total) atomicAdd(total64, (unsigned long long)total);
  }
}

// out[c] += part_off[workgroup of c]; out[n] = the total
static __global__ __launch_bounds__(RASTER_THREADS) void k_raster_scan_add(long n, const unsigned* __restrict__ part_off, unsigned nb,
                                                                           unsigned* __restrict__ out) {
  const long c = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  if (c < n) out[c] += part_off[blockIdx.x];
  if (c == n) out[n] = part_off[nb];
}

// in [n] -> out [n + 1] (another buffer), 1 <= n < 2^31; part and part_off hold raster_blocks(n) + 1 words each.  Enqueues only;
// *total64 (device) holds the sum afterwards, and the caller compares it with 2^31 before anything trusts the 32-bit offsets.
// `stage` is what a failure is reported under ("<stage> scan", "<stage>_scan_local", ..).
static int raster_scan(const char* stage, long n, const unsigned* in, unsigned* out, unsigned* part, unsigned* part_off, unsigned long long* total64,
                       hipStream_t st) {
  const unsigned nb = raster_blocks(n);
  const hipError_t e = hipMemsetAsync(total64, 0, 8, st);
  if (e != hipSuccess) return set_error((int)e, "%s scan: %s", stage, hipGetErrorString(e));
  hipLaunchKernelGGL(k_raster_scan_local, dim3(nb), dim3(RASTER_THREADS), 0, st, n, in, out, part, total64);
  hipError_t l = hipGetLastError();
  if (l != hipSuccess) return set_error((int)l, "%s_scan_local: %s", stage, hipGetErrorString(l));
  if (int rc = launch_fusion_scan(part, part_off, (int)nb, st)) return rc;
  hipLaunchKernelGGL(k_raster_scan_add, dim3(raster_blocks(n + 1)), dim3(RASTER_THREADS), 0, st, n, part_off, nb, out);
  l = hipGetLastError();
  if (l != hipSuccess) return set_error((int)l, "%s_scan_add: %s", stage, hipGetErrorString(l));
  return 0;
}

// ---- list ranking: the distance rounds ----------------------------------------------------------------------------------------
// A pair (x, y) per element of a forest of chains: x >= 0 is the ancestor reached so far and y the steps to it; x < 0 says ARRIVED,
// at the element ~x, which y steps lead to.  A chain's first element starts as (~itself, 0), every other as (its predecessor, 1).
// One round of pointer doubling, double-buffered.  The contour lines rank their segments with it, the drainage stage the cells of
// a stream below their link's head.
static __global__ __launch_bounds__(RASTER_THREADS) void k_raster_rank_dist(long N, const int2* __restrict__ cur, int2* __restrict__ nxt,
                                                                            unsigned* changed) {
  const long n = (long)blockIdx.x * RASTER_THREADS + threadIdx.x;
  bool moved = false;
  if (n < N) {
    int2 v = cur[n];
    if (v.x >= 0 && (long)v.x < N) {
      const int2 a = cur[v.x];
      v = make_int2(a.x, v.y + a.y);
      moved = true;
    }
    nxt[n] = v;
  }
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) changed[0] = 1u;
}

// One phase of a ranking: up to RASTER_RANK_ROUNDS rounds of `kernel` (N, cur, nxt, changed word), RASTER_RANK_CHUNK rounds per
// read-back of the changed words changed[base ..], which the caller has zeroed; the result is in buf[*where] afterwards.  *moved:
// the rounds that changed a pair; *launched is added to; *converged: a round changed nothing (2^31 elements need 31 rounds and
// that one).
constexpr int RASTER_RANK_ROUNDS = 32;
constexpr int RASTER_RANK_CHUNK = 4;
static_assert(RASTER_RANK_ROUNDS % RASTER_RANK_CHUNK == 0, "whole chunks");
template <typename Kernel>
static int raster_rank_phase(Kernel kernel, const char* name, long N, int2* const buf[2], int* where, unsigned* changed, int base, int* moved,
                             int* launched, bool* converged, hipStream_t st) {
  unsigned host[RASTER_RANK_ROUNDS];
  *moved = 0;
  *converged = false;
  for (int done = 0; done < RASTER_RANK_ROUNDS && !*converged; done += RASTER_RANK_CHUNK) {
    for (int k = done; k < done + RASTER_RANK_CHUNK; ++k) {
      hipLaunchKernelGGL(kernel, dim3(raster_blocks(N)), dim3(RASTER_THREADS), 0, st, N, (const int2*)buf[*where], buf[*where ^ 1], changed + base + k);
      ADAMVS_CHECK_LAUNCH(name);
      *where ^= 1;
      ++*launched;
    }
    hipError_t e = hipMemcpyAsync(host, changed + base, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "%s: %s", name, hipGetErrorString(e));
    for (int k = done; k < done + RASTER_RANK_CHUNK && !*converged; ++k) {
      if (host[k]) *moved = k + 1;
      else *converged = true;        // a round that changes nothing leaves every later one without a change: the result stands
    }
  }
  return 0;
}

}  // namespace adamvs
