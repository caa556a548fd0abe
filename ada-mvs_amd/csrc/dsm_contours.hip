// Contour lines of a height raster as ordered polylines: the integer surface, the segments of marching squares with their
// successors and predecessors in closed form, the position of every segment in its line by list ranking, the line table and the
// vertices.  include/adamvs_hip.h "Contours" states the result; this file computes it with these kernels:
//
//   k_ctr_quant         one lane per cell: q, INT32_MIN outside V; the finite cells out of range are counted, summed in LDS
//                       and added once per workgroup (none, on a raster that passes).  The cells of V are NOT counted here:
//                       every workgroup would add to one word.
//   k_ctr_smooth        one binomial pass (raster_prims.h binomial3x3; a hole is INT32_MIN).  The last kernel of
//                       _contour_surface reduces the minimum and maximum of s per workgroup and issues an integer atomic only
//                       where the word it has just read would change (dsm_trees.hip records what per-wave atomics on one
//                       address cost).
//   k_ctr_count         one workgroup per tile of CTR_T x CTR_T blocks: the (CTR_T + 1)^2 samples and the level table go to LDS,
//                       a lane takes a block, two binary searches give the range of levels that cross it and two more the
//                       saddle sub-range; the count is the sum of the two lengths.
//   raster_scan         the exclusive scan of raster_prims.h, used three times (block counts -> offsets, start flags -> line
//                       numbers, vertex counts -> line_first).  The total is also summed in 64 bits, so an overflow of the
//                       32-bit offsets is seen on the host before anything reads them.
//   k_ctr_segments      one lane per SEGMENT, not per block: the lane finds its block by a binary search in the scanned offsets
//                       (23 steps for 2^23 cells, the upper ones shared by the whole wave and the lower ones a few cache lines
//                       apart), its level and entry edge from the block's two ranges.  A cliff with hundreds of levels in one
//                       block is then hundreds of lanes, not one lane's loop.  The partner across the exit edge (succ) and
//                       across the entry edge (pred) has the number  offset + levels of its range below k + saddle levels
//                       below k + entry order; the neighbour's four samples are re-read from L2.  No sort, no hash, no atomic.
//                       LDS for the tile was NOT built here: a lane's block is wherever its segment number falls, so a
//                       workgroup's blocks are no tile.
//   k_ctr_rank_*        list ranking by pointer doubling over pred, double-buffered, one kernel per round, an (ancestor, value)
//                       pair of 8 bytes per segment so that a round is one gather.  Phase 1 carries the smallest number seen;
//                       a chain's head marks its descendants as arrived.  It stops when a round brought no arrival and lowered
//                       no minimum of a segment that has not arrived (the header proves that every ring then holds its
//                       minimum).  Phase 2, the rings cut at their minimum, carries the distance.  CTR_RANK_CHUNK rounds per
//                       read-back of the changed words, as k_tree_jump.  The LDS pre-ranking of tile-local chains was not built.
//   k_ctr_line_*        flags of the starts, their scan into line numbers, the tails' scatter of the vertex counts and the line
//                       table, the scan into line_first, the vertices.
//
// Integer atomics only (min, max, add), which commute; every store of the segment and line kernels goes to a slot that exactly
// one lane owns: every output is bit-identical from run to run.  No workgroup waits on another.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

constexpr int CTR_T = ADAMVS_CONTOUR_TILE;
constexpr int CTR_LDS_W = CTR_T + 1;
constexpr int CTR_THREADS = 256;
constexpr int CTR_WAVES = CTR_THREADS / 64;
constexpr int CTR_RANK_CHUNK = 4;
constexpr int CTR_PHASE_ROUNDS = ADAMVS_CONTOUR_MAX_ROUNDS / 2;
constexpr int CTR_NONE = INT_MIN;                // s outside V
static_assert(CTR_T == 64, "a wave takes one row of a tile");
static_assert(CTR_PHASE_ROUNDS % CTR_RANK_CHUNK == 0 && CTR_PHASE_ROUNDS >= 32, "2^31 segments need 31 rounds and one that changes nothing");
static_assert(CTR_THREADS == RASTER_THREADS && CTR_PHASE_ROUNDS == RASTER_RANK_ROUNDS && CTR_RANK_CHUNK == RASTER_RANK_CHUNK,
              "the scan and the ranking phases of raster_prims.h");

// the control block at the head of either workspace
constexpr long CTR_OFF_CHANGED = 0;              // unsigned [ADAMVS_CONTOUR_MAX_ROUNDS]: phase 1, then phase 2
constexpr long CTR_OFF_TOTAL = 256;              // unsigned long long: the total of the last scan
constexpr long CTR_OFF_LINES = 264;              // unsigned long long: the starts counted by the ranking
constexpr long CTR_CONTROL = 512;

static inline unsigned ctr_blocks(long n) { return (unsigned)((n + CTR_THREADS - 1) / CTR_THREADS); }

// ---- workspaces -------------------------------------------------------------------------------------------------------------
// grid: control | level table | two int32 rasters (the surface's intermediate passes) | offsets unsigned [n + 1] | workgroup
// totals and their offsets, unsigned [nb + 1] each
struct CtrGridWs {
  int* lev;
  int* tmp[2];
  unsigned* off;
  unsigned* part;
  unsigned* part_off;
  long bytes;
};
static CtrGridWs ctr_grid_ws(void* workspace, int W, int H) {
  const long n = (long)W * H, nb = ctr_blocks(n);
  char* p = (char*)workspace;
  CtrGridWs w;
  long o = CTR_CONTROL;
  w.lev = (int*)(p + o);
  o += align256(4L * ADAMVS_CONTOUR_MAX_LEVELS);
  w.tmp[0] = (int*)(p + o);
  o += align256(4 * n);
  w.tmp[1] = (int*)(p + o);
  o += align256(4 * n);
  w.off = (unsigned*)(p + o);
  o += align256(4 * (n + 1));
  w.part = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.part_off = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.bytes = o;
  return w;
}
long contour_workspace_bytes(int W, int H) { return ctr_grid_ws(nullptr, W, H).bytes; }

// segments: control | level table | two (ancestor, value) buffers int2 [N] (the lines' vertex counts and their scan lie over them
// once the ranking is done) | line numbers unsigned [N + 1] | workgroup totals and their offsets
struct CtrSegWs {
  int* lev;
  int2* buf[2];
  unsigned* count;       // over buf[0]: unsigned [M]
  unsigned* first;       // over buf[1]: unsigned [M + 1]
  unsigned* lineno;
  unsigned* part;
  unsigned* part_off;
  long bytes;
};
static CtrSegWs ctr_seg_ws(void* workspace, long N) {
  const long nb = ctr_blocks(N + 1);
  char* p = (char*)workspace;
  CtrSegWs w;
  long o = CTR_CONTROL;
  w.lev = (int*)(p + o);
  o += align256(4L * ADAMVS_CONTOUR_MAX_LEVELS);
  w.buf[0] = (int2*)(p + o);
  w.count = (unsigned*)(p + o);
  o += align256(8 * (N + 1));
  w.buf[1] = (int2*)(p + o);
  w.first = (unsigned*)(p + o);
  o += align256(8 * (N + 1));
  w.lineno = (unsigned*)(p + o);
  o += align256(4 * (N + 1));
  w.part = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.part_off = (unsigned*)(p + o);
  o += align256(4 * (nb + 1));
  w.bytes = o;
  return w;
}
long contour_rank_workspace_bytes(long N) { return ctr_seg_ws(nullptr, N).bytes; }

// ---- the surface ------------------------------------------------------------------------------------------------------------
// info[0] = s_min, info[1] = s_max over the workgroup's cells of V (lo = INT_MAX, hi = INT_MIN for a lane without one)
__device__ __forceinline__ void ctr_block_range(int lo, int hi, int* info) {
  __shared__ int s_lo[CTR_WAVES], s_hi[CTR_WAVES];
  lo = wave_min(lo);
  hi = wave_max(hi);
  if ((threadIdx.x & 63) == 0) {
    s_lo[threadIdx.x >> 6] = lo;
    s_hi[threadIdx.x >> 6] = hi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < CTR_WAVES; ++k) {
      lo = s_lo[k] < lo ? s_lo[k] : lo;
      hi = s_hi[k] > hi ? s_hi[k] : hi;
    }
    if (lo < __hip_atomic_load(info + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(info + 0, lo);
    if (hi > __hip_atomic_load(info + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(info + 1, hi);
  }
}

__global__ void k_ctr_info_init(int* info) {
  if (threadIdx.x == 0) {
    info[0] = INT_MAX;
    info[1] = INT_MIN;
    info[2] = 0;
  }
}

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_quant(long n, const float* __restrict__ z, double z_ref, int* __restrict__ dst, int* info,
                                                           int reduce) {
  __shared__ unsigned s_bad;
  if (threadIdx.x == 0) s_bad = 0u;
  __syncthreads();
  const long c = (long)blockIdx.x * CTR_THREADS + threadIdx.x;      // no early return: every lane takes part in the shuffles
  int sv = CTR_NONE;
  bool bad = false;
  if (c < n) {
    const float v = z[c];
    if (__builtin_isfinite(v)) {
      const double d = (double)v - z_ref;
      if (fabs(d) <= 8191.0) sv = (int)llrint(d * 256.0);
      else bad = true;
    }
    dst[c] = sv;
  }
  const unsigned long long bal_bad = __ballot(bad);                  // none on a raster that passes
  if (bal_bad && (threadIdx.x & 63) == 0) atomicAdd(&s_bad, (unsigned)__popcll(bal_bad));
  __syncthreads();
  if (threadIdx.x == 0 && s_bad) atomicAdd(info + 2, (int)s_bad);   // one atomic per workgroup, as for the range
  if (reduce) ctr_block_range(sv == CTR_NONE ? INT_MAX : sv, sv, info);      // wave-uniform: a kernel argument
}

struct CtrHole {
  static constexpr int NONE = CTR_NONE;
  static __device__ __forceinline__ bool is(int v) { return v == CTR_NONE; }
};

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_smooth(int W, int H, const int* __restrict__ src, int* __restrict__ dst, int* info, int reduce) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  int out = CTR_NONE;
  if (c < n) dst[c] = out = binomial3x3<CtrHole>(W, H, src, c);      // |s| <= 8191 * 256 * 16^2 < 2^30
  if (reduce) ctr_block_range(out == CTR_NONE ? INT_MAX : out, out, info);
}

// ---- a block's levels -------------------------------------------------------------------------------------------------------
// the first k with lev[k] > v
__device__ __forceinline__ int ctr_upper(const int* lev, int K, int v) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (lev[mid] > v) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

struct CtrRange {
  int k0, k1;            // the levels that cross the block: min < lev[k] <= max
  int s0, s1;            // those at which it is a saddle (empty: s0 == s1); inside [k0, k1)
  __device__ __forceinline__ int count() const { return (k1 - k0) + (s1 - s0); }
  // segments of the block at levels below k
  __device__ __forceinline__ int below(int k) const {
    const int t = k - s0;
    return (k - k0) + (t < 0 ? 0 : t > s1 - s0 ? s1 - s0 : t);
  }
  __device__ __forceinline__ bool saddle(int k) const { return k >= s0 && k < s1; }
};

__device__ __forceinline__ int ctr_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int ctr_max(int a, int b) { return a > b ? a : b; }

// corners A, B, C, D; a block with a corner outside V has no level
__device__ __forceinline__ CtrRange ctr_range(int a, int b, int c, int d, const int* lev, int K) {
  CtrRange r = {0, 0, 0, 0};
  if (a == CTR_NONE || b == CTR_NONE || c == CTR_NONE || d == CTR_NONE) return r;
  const int lo = ctr_min(ctr_min(a, b), ctr_min(c, d)), hi = ctr_max(ctr_max(a, b), ctr_max(c, d));
  if (lo == hi) return r;
  r.k0 = ctr_upper(lev, K, lo);
  r.k1 = ctr_upper(lev, K, hi);
  r.s0 = r.s1 = r.k0;
  // A and C up, B and D down iff max(b, d) < lev <= min(a, c); the other saddle likewise; at most one of the two is not empty
  const int ac_lo = ctr_min(a, c), ac_hi = ctr_max(a, c), bd_lo = ctr_min(b, d), bd_hi = ctr_max(b, d);
  if (r.k1 > r.k0) {
    if (bd_hi < ac_lo) {
      r.s0 = ctr_upper(lev, K, bd_hi);
      r.s1 = ctr_upper(lev, K, ac_lo);
    } else if (ac_hi < bd_lo) {
      r.s0 = ctr_upper(lev, K, ac_hi);
      r.s1 = ctr_upper(lev, K, bd_lo);
    }
  }
  return r;
}

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_count(int W, int H, int tiles_x, const int* __restrict__ s, const int* __restrict__ lev, int K,
                                                           int* __restrict__ count) {
  __shared__ int s_t[CTR_LDS_W * CTR_LDS_W];
  __shared__ int s_lev[ADAMVS_CONTOUR_MAX_LEVELS];
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int i0 = ty * CTR_T, j0 = tx * CTR_T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < CTR_LDS_W * CTR_LDS_W; k += CTR_THREADS) {
    const int li = k / CTR_LDS_W, lj = k - li * CTR_LDS_W;
    const int gi = i0 + li, gj = j0 + lj;
    s_t[k] = (gi < H && gj < W) ? s[(long)gi * W + gj] : CTR_NONE;
  }
  for (int k = threadIdx.x; k < K; k += CTR_THREADS) s_lev[k] = lev[k];
  __syncthreads();
  for (int r = wv; r < CTR_T; r += CTR_WAVES) {
    const int i = i0 + r, j = j0 + lane;
    if (i >= H || j >= W) continue;
    // the last row and column of cells head no block; the samples past the grid are CTR_NONE in LDS: no level there
    const CtrRange g = ctr_range(s_t[r * CTR_LDS_W + lane], s_t[r * CTR_LDS_W + lane + 1], s_t[(r + 1) * CTR_LDS_W + lane + 1],
                                 s_t[(r + 1) * CTR_LDS_W + lane], s_lev, K);
    count[(long)i * W + j] = g.count();
  }
}

// ---- the scan: raster_prims.h raster_scan ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_widen(long n, const unsigned* __restrict__ in, long long* __restrict__ out) {
  const long c = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (c < n) out[c] = (long long)in[c];
}

// ---- the segments -----------------------------------------------------------------------------------------------------------
// the code of edge e of block (i, j): AB and CD run east from A and D, BC and DA south from B and A
__device__ __forceinline__ int ctr_edge_code(int W, int i, int j, int e) {
  const int ci = i + (e == 2 ? 1 : 0), cj = j + (e == 1 ? 1 : 0);
  return 2 * (ci * W + cj) + (e & 1);                                // W H <= 2^28: below 2^30
}

// centre up iff 2 (a + b + c + d) >= 4 (2 lev - 1)
__device__ __forceinline__ bool ctr_centre_up(int a, int b, int c, int d, int level) {
  return 2LL * ((long long)a + b + c + d) >= 4LL * (2LL * level - 1);
}

struct CtrBlock {
  int a, b, c, d;
  CtrRange g;
  unsigned off;
};

// the block (i, j), which may lie outside the grid: no level then
__device__ __forceinline__ CtrBlock ctr_block(int W, int H, int i, int j, const int* __restrict__ s, const unsigned* __restrict__ off,
                                              const int* __restrict__ lev, int K) {
  CtrBlock B;
  B.g = {0, 0, 0, 0};
  B.off = 0u;
  B.a = B.b = B.c = B.d = CTR_NONE;
  if (i < 0 || j < 0 || i >= H - 1 || j >= W - 1) return B;
  const long c0 = (long)i * W + j;
  B.a = s[c0];
  B.b = s[c0 + 1];
  B.c = s[c0 + W + 1];
  B.d = s[c0 + W];
  B.g = ctr_range(B.a, B.b, B.c, B.d, lev, K);
  B.off = off[c0];
  return B;
}

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_segments(int W, int H, long N, const int* __restrict__ s, const unsigned* __restrict__ off,
                                                              const int* __restrict__ lev, int K, int* __restrict__ seg_entry,
                                                              int* __restrict__ seg_exit, int* __restrict__ seg_level, int* __restrict__ succ,
                                                              int* __restrict__ pred) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n >= N) return;
  // the block: the largest index with off <= n; the blocks without a segment share their offset with the next one
  long lo = 0, hi = (long)W * H;                                     // off[lo] <= n < off[hi]; off[W H] = N
  while (hi - lo > 1) {
    const long mid = (lo + hi) >> 1;
    if ((long)off[mid] <= n) lo = mid;
    else hi = mid;
  }
  int i, j;
  cell_ij(lo, W, i, j);
  const CtrBlock B = ctr_block(W, H, i, j, s, off, lev, K);
  const int r = (int)(n - (long)B.off);
  int out_entry = -1, out_exit = -1, out_level = -1, out_succ = -1, out_pred = -1;
  if (r >= 0 && r < B.g.count()) {                                   // always, for the offsets of _contour_count and the same s and table
    const CtrRange g = B.g;
    const int single = g.s0 - g.k0, twice = 2 * (g.s1 - g.s0);
    int k, which = 0;
    if (r < single) k = g.k0 + r;
    else if (r < single + twice) {
      k = g.s0 + ((r - single) >> 1);
      which = (r - single) & 1;
    } else k = g.s1 + (r - single - twice);
    const int level = lev[k];
    const bool up[4] = {B.a >= level, B.b >= level, B.c >= level, B.d >= level};
    int e = 0, x = 0;
    if (g.saddle(k)) {
      e = (up[0] ? 1 : 0) + 2 * which;                               // A and C up: entries BC, DA; B and D up: AB, CD
      x = ctr_centre_up(B.a, B.b, B.c, B.d, level) ? (e + 3) & 3 : (e + 1) & 3;
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (!up[t] && up[(t + 1) & 3]) e = t;
        if (up[t] && !up[(t + 1) & 3]) x = t;
      }
    }
    out_entry = ctr_edge_code(W, i, j, e);
    out_exit = ctr_edge_code(W, i, j, x);
    out_level = k;
    // across edge 0 lies (i - 1, j), across 1 (i, j + 1), across 2 (i + 1, j), across 3 (i, j - 1); it sees the edge as (e + 2) % 4
    {
      const CtrBlock Q = ctr_block(W, H, i + (x == 2) - (x == 0), j + (x == 1) - (x == 3), s, off, lev, K);
      if (k >= Q.g.k0 && k < Q.g.k1) {                               // it has all four samples, hence this crossing as an entry
        const int qe = (x + 2) & 3;
        out_succ = (int)(Q.off + (unsigned)Q.g.below(k) + (Q.g.saddle(k) && qe >= 2 ? 1u : 0u));
      }
    }
    {
      const CtrBlock Q = ctr_block(W, H, i + (e == 2) - (e == 0), j + (e == 1) - (e == 3), s, off, lev, K);
      if (k >= Q.g.k0 && k < Q.g.k1) {
        const int qx = (e + 2) & 3;
        int second = 0;
        if (Q.g.saddle(k)) second = ((ctr_centre_up(Q.a, Q.b, Q.c, Q.d, level) ? qx + 1 : qx + 3) & 3) >= 2;
        out_pred = (int)(Q.off + (unsigned)Q.g.below(k) + (unsigned)second);
      }
    }
  }
  seg_entry[n] = out_entry;
  seg_exit[n] = out_exit;
  seg_level[n] = out_level;
  succ[n] = out_succ;
  pred[n] = out_pred;
}

// ---- list ranking -----------------------------------------------------------------------------------------------------------
// A pair (x, y): x >= 0 is the ancestor reached so far; x < 0 says ARRIVED, at the segment ~x.
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_rank_init(long N, const int* __restrict__ pred, int2* __restrict__ st) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n >= N) return;
  const int p = pred[n];
  st[n] = (p >= 0 && (long)p < N) ? make_int2(p, (int)n) : make_int2(~(int)n, (int)n);       // a head has arrived at itself
}

// phase 1: y = the smallest number among the segment and the predecessors passed
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_rank_min(long N, const int2* __restrict__ cur, int2* __restrict__ nxt, unsigned* changed) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  bool moved = false;
  if (n < N) {
    int2 v = cur[n];
    if (v.x >= 0) {
      const int2 a = cur[v.x];                                       // 0 <= v.x < N by the init and by induction
      const int m = a.y < v.y ? a.y : v.y;
      moved = a.x < 0 || m != v.y;
      v = make_int2(a.x, m);
    }
    nxt[n] = v;
  }
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) changed[0] = 1u;
}

// between the phases: start and closed of every segment; the rings are cut at their smallest segment; the starts are counted
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_rank_cut(long N, const int2* __restrict__ res, const int* __restrict__ pred, int2* __restrict__ st,
                                                              int* __restrict__ start, uint8_t* __restrict__ closed, unsigned long long* lines) {
  __shared__ unsigned s_n;
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  bool is_start = false;
  if (n < N) {
    const int2 v = res[n];
    const int b = v.x < 0 ? ~v.x : v.y;
    start[n] = b;
    closed[n] = v.x < 0 ? 0 : 1;
    is_start = (long)b == n;
    st[n] = is_start ? make_int2(~(int)n, 0) : make_int2(pred[n], 1);           // not a start: it has a predecessor inside 0 .. N - 1
  }
  const unsigned long long bal = __ballot(is_start);
  if (bal && (threadIdx.x & 63) == 0) atomicAdd(&s_n, (unsigned)__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(lines, (unsigned long long)s_n);
}

// phase 2, y = the succ steps from the ancestor to the segment: raster_prims.h k_raster_rank_dist

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_rank_store(long N, const int2* __restrict__ res, int* __restrict__ rank) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n < N) rank[n] = res[n].y;
}

// ---- the lines --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_line_flag(long N, const int* __restrict__ start, unsigned* __restrict__ flag) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n < N) flag[n] = (long)start[n] == n ? 1u : 0u;
}

__device__ __forceinline__ bool ctr_is_tail(int succ_n, int start_n) { return succ_n < 0 || succ_n == start_n; }

// the tail of a line knows its length: vertex count, start, level and closed of line m
__global__ __launch_bounds__(CTR_THREADS) void k_ctr_line_tails(long N, long M, const int* __restrict__ succ, const int* __restrict__ start,
                                                                const int* __restrict__ rank, const uint8_t* __restrict__ closed,
                                                                const int* __restrict__ seg_level, const unsigned* __restrict__ lineno,
                                                                unsigned* __restrict__ count, int* __restrict__ line_start,
                                                                int* __restrict__ line_level, uint8_t* __restrict__ line_closed) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n >= N) return;
  const int b = start[n];
  if (b < 0 || (long)b >= N || !ctr_is_tail(succ[n], b)) return;
  const long m = lineno[b];
  const int rk = rank[n];
  if (m >= M || start[b] != b || rk < 0 || (long)rk >= N) return;   // never, for the ranking's own results
  count[m] = (unsigned)rk + 2u;                                      // rank + 1 segments and one vertex more
  line_start[m] = b;
  line_level[m] = seg_level[b];
  line_closed[m] = closed[n];
}

__device__ __forceinline__ void ctr_store_vertex(long long* __restrict__ vertex, long p, int code, int W, long cells, const int* __restrict__ s, int level) {
  const long c = code >> 1;
  const long c2 = c + ((code & 1) ? W : 1);
  long long num = 0, den = 1;
  if (code >= 0 && c2 < cells) {
    const long long a = s[c], b = s[c2];
    num = 2LL * level - 1 - 2 * a;
    den = 2 * b - 2 * a;
    if (den < 0) {
      num = -num;
      den = -den;
    }
  }
  vertex[3 * p + 0] = code;
  vertex[3 * p + 1] = num;
  vertex[3 * p + 2] = den;
}

__global__ __launch_bounds__(CTR_THREADS) void k_ctr_line_vertices(int W, int H, long N, long M, const int* __restrict__ s, const int* __restrict__ lev,
                                                                   int K, const int* __restrict__ seg_entry, const int* __restrict__ seg_exit,
                                                                   const int* __restrict__ seg_level, const int* __restrict__ succ,
                                                                   const int* __restrict__ start, const int* __restrict__ rank,
                                                                   const unsigned* __restrict__ lineno, const unsigned* __restrict__ first,
                                                                   long long* __restrict__ vertex) {
  const long n = (long)blockIdx.x * CTR_THREADS + threadIdx.x;
  if (n >= N) return;
  const int b = start[n], k = seg_level[n], rk = rank[n];
  if (b < 0 || (long)b >= N || k < 0 || k >= K || rk < 0) return;
  const long m = lineno[b];
  if (m >= M) return;
  const long p = (long)first[m] + rk;
  if (p + 1 >= N + M) return;                                        // keeps every store in bounds whatever the caller passed
  const int level = lev[k];
  ctr_store_vertex(vertex, p, seg_entry[n], W, (long)W * H, s, level);
  if (ctr_is_tail(succ[n], b)) ctr_store_vertex(vertex, p + 1, seg_exit[n], W, (long)W * H, s, level);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static int ctr_upload_levels(int* dst, const int* lev, int K, const char* what, hipStream_t st) {
  if (K == 0) return 0;
  hipError_t e = hipMemcpyAsync(dst, lev, 4L * K, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);                 // `lev` is the caller's memory: gone from it before we return
  if (e != hipSuccess) return set_error((int)e, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

int launch_contour_surface(int W, int H, const float* z, double z_ref, int smooth_passes, void* workspace, int* s, int* info, hipStream_t st) {
  const long n = (long)W * H;
  const CtrGridWs w = ctr_grid_ws(workspace, W, H);
  hipLaunchKernelGGL(k_ctr_info_init, dim3(1), dim3(64), 0, st, info);
  ADAMVS_CHECK_LAUNCH("contour_info_init");
  int* dst = smooth_passes == 0 ? s : w.tmp[0];
  hipLaunchKernelGGL(k_ctr_quant, dim3(ctr_blocks(n)), dim3(CTR_THREADS), 0, st, n, z, z_ref, dst, info, smooth_passes == 0 ? 1 : 0);
  ADAMVS_CHECK_LAUNCH("contour_quant");
  for (int k = 0; k < smooth_passes; ++k) {
    const bool last = k == smooth_passes - 1;
    const int* src = dst;
    dst = last ? s : w.tmp[1];
    hipLaunchKernelGGL(k_ctr_smooth, dim3(ctr_blocks(n)), dim3(CTR_THREADS), 0, st, W, H, src, dst, info, last ? 1 : 0);
    ADAMVS_CHECK_LAUNCH("contour_smooth");
  }
  return 0;
}

int launch_contour_count(int W, int H, const int* s, int K, const int* lev, void* workspace, int* count, adamvs_contour_stats* stats,
                         hipStream_t st) {
  const long n = (long)W * H;
  const CtrGridWs w = ctr_grid_ws(workspace, W, H);
  unsigned long long* total64 = (unsigned long long*)((char*)workspace + CTR_OFF_TOTAL);
  stats->segments = 0;
  if (int rc = ctr_upload_levels(w.lev, lev, K, "contour_count", st)) return rc;
  BldClock clock;
  clock.mark(0, st);
  const int tiles_x = cdiv(W, CTR_T), tiles_y = cdiv(H, CTR_T);
  hipLaunchKernelGGL(k_ctr_count, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(CTR_THREADS), 0, st, W, H, tiles_x, s, w.lev, K, count);
  ADAMVS_CHECK_LAUNCH("contour_count");
  if (int rc = raster_scan("contour", n, (const unsigned*)count, w.off, w.part, w.part_off, total64, st)) return rc;
  clock.mark(1, st);
  unsigned long long total = 0;
  hipError_t e = hipMemcpyAsync(&total, total64, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "contour_count: %s", hipGetErrorString(e));
  stats->ms_count = clock.ms(0);
  stats->segments = (long)total;
  if (total >= (1ull << 31)) return set_error(ADAMVS_CONTOUR_TOO_MANY, "contour_count: %llu segments, fewer than 2^31 can be numbered", total);
  return 0;
}

int launch_contour_segments(int W, int H, const int* s, int K, const int* lev, long N, void* workspace, int* seg_entry, int* seg_exit,
                            int* seg_level, int* succ, int* pred, hipStream_t st) {
  if (N == 0) return 0;
  const CtrGridWs w = ctr_grid_ws(workspace, W, H);
  if (int rc = ctr_upload_levels(w.lev, lev, K, "contour_segments", st)) return rc;
  unsigned total = 0;                                                // the offsets must be those of this N: off[W H] is their total
  hipError_t e = hipMemcpyAsync(&total, w.off + (long)W * H, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "contour_segments: %s", hipGetErrorString(e));
  if ((long)total != N) return set_error(-1, "contour_segments: N=%ld, but the workspace holds the offsets of %u segments (_contour_count first)", N, total);
  hipLaunchKernelGGL(k_ctr_segments, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, W, H, N, s, w.off, w.lev, K, seg_entry, seg_exit, seg_level, succ,
                     pred);
  ADAMVS_CHECK_LAUNCH("contour_segments");
  return 0;
}

int launch_contour_rank(long N, const int* pred, void* workspace, int* start, int* rank, uint8_t* closed, adamvs_contour_stats* stats,
                        hipStream_t st) {
  stats->rounds = stats->rounds_min = stats->rounds_dist = stats->launched = 0;
  stats->converged = 1;
  stats->lines = 0;
  stats->ms_rank = 0.0f;
  if (N == 0) return 0;
  const CtrSegWs w = ctr_seg_ws(workspace, N);
  unsigned* changed = (unsigned*)((char*)workspace + CTR_OFF_CHANGED);
  unsigned long long* lines = (unsigned long long*)((char*)workspace + CTR_OFF_LINES);
  stats->converged = 0;
  BldClock clock;
  hipError_t e = hipMemsetAsync(workspace, 0, CTR_CONTROL, st);
  if (e != hipSuccess) return set_error((int)e, "contour_rank: %s", hipGetErrorString(e));
  clock.mark(0, st);
  int where = 0;
  bool ok = false;
  hipLaunchKernelGGL(k_ctr_rank_init, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, N, pred, w.buf[0]);
  ADAMVS_CHECK_LAUNCH("contour_rank_init");
  if (int rc = raster_rank_phase(k_ctr_rank_min, "contour_rank_min", N, w.buf, &where, changed, 0, &stats->rounds_min, &stats->launched, &ok, st)) return rc;
  if (!ok) return set_error(ADAMVS_CONTOUR_NOT_CONVERGED, "contour_rank: minima still moving after %d rounds", CTR_PHASE_ROUNDS);
  hipLaunchKernelGGL(k_ctr_rank_cut, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, N, (const int2*)w.buf[where], pred, w.buf[where ^ 1], start, closed,
                     lines);
  ADAMVS_CHECK_LAUNCH("contour_rank_cut");
  where ^= 1;
  if (int rc = raster_rank_phase(k_raster_rank_dist, "contour_rank_dist", N, w.buf, &where, changed, CTR_PHASE_ROUNDS, &stats->rounds_dist, &stats->launched,
                              &ok, st))
    return rc;
  if (!ok) return set_error(ADAMVS_CONTOUR_NOT_CONVERGED, "contour_rank: distances still moving after %d rounds", CTR_PHASE_ROUNDS);
  hipLaunchKernelGGL(k_ctr_rank_store, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, N, (const int2*)w.buf[where], rank);
  ADAMVS_CHECK_LAUNCH("contour_rank_store");
  clock.mark(1, st);
  unsigned long long M = 0;
  e = hipMemcpyAsync(&M, lines, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "contour_rank: %s", hipGetErrorString(e));
  stats->rounds = stats->rounds_min + stats->rounds_dist;
  stats->converged = 1;
  stats->lines = (long)M;
  stats->ms_rank = clock.ms(0);
  if ((unsigned long long)N + M >= (1ull << 31))
    return set_error(ADAMVS_CONTOUR_TOO_MANY, "contour_rank: %ld segments and %llu lines, N + M must stay below 2^31", N, M);
  return 0;
}

int launch_contour_lines(int W, int H, const int* s, int K, const int* lev, long N, long M, const int* seg_entry, const int* seg_exit,
                         const int* seg_level, const int* succ, const int* start, const int* rank, const uint8_t* closed, void* workspace,
                         long long* line_first, int* line_start, int* line_level, uint8_t* line_closed, long long* vertex, hipStream_t st) {
  if (N == 0) {
    const hipError_t e = hipMemsetAsync(line_first, 0, 8, st);
    if (e != hipSuccess) return set_error((int)e, "contour_lines: %s", hipGetErrorString(e));
    return 0;
  }
  const CtrSegWs w = ctr_seg_ws(workspace, N);
  unsigned long long* total64 = (unsigned long long*)((char*)workspace + CTR_OFF_TOTAL);
  if (int rc = ctr_upload_levels(w.lev, lev, K, "contour_lines", st)) return rc;
  unsigned* flag = (unsigned*)w.buf[0];                              // the ranking's buffers are free again
  hipLaunchKernelGGL(k_ctr_line_flag, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, N, start, flag);
  ADAMVS_CHECK_LAUNCH("contour_line_flag");
  if (int rc = raster_scan("contour", N, flag, w.lineno, w.part, w.part_off, total64, st)) return rc;
  unsigned long long total = 0;
  hipError_t e = hipMemcpyAsync(&total, total64, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "contour_lines: %s", hipGetErrorString(e));
  if ((long)total != M) return set_error(-1, "contour_lines: M=%ld, but start holds %llu starts", M, total);
  // M >= 1: a segment's start is a segment
  e = hipMemsetAsync(w.count, 0, 4 * M, st);
  if (e != hipSuccess) return set_error((int)e, "contour_lines: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_ctr_line_tails, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, N, M, succ, start, rank, closed, seg_level, (const unsigned*)w.lineno,
                     w.count, line_start, line_level, line_closed);
  ADAMVS_CHECK_LAUNCH("contour_line_tails");
  if (int rc = raster_scan("contour", M, w.count, w.first, w.part, w.part_off, total64, st)) return rc;
  e = hipMemcpyAsync(&total, total64, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "contour_lines: %s", hipGetErrorString(e));
  if ((long)total != N + M) return set_error(-1, "contour_lines: the lines hold %llu vertices, N + M = %ld (start, rank and succ must be one ranking's)", total, N + M);
  hipLaunchKernelGGL(k_ctr_widen, dim3(ctr_blocks(M + 1)), dim3(CTR_THREADS), 0, st, M + 1, (const unsigned*)w.first, line_first);
  ADAMVS_CHECK_LAUNCH("contour_widen");
  hipLaunchKernelGGL(k_ctr_line_vertices, dim3(ctr_blocks(N)), dim3(CTR_THREADS), 0, st, W, H, N, M, s, (const int*)w.lev, K, seg_entry, seg_exit, seg_level,
                     succ, start, rank, (const unsigned*)w.lineno, (const unsigned*)w.first, vertex);
  ADAMVS_CHECK_LAUNCH("contour_line_vertices");
  return 0;
}

}  // namespace adamvs
