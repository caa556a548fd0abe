// Tree detection on the nDSM: canopy mask and smoothed integer surface, the parent forest of the variable-window local-maximum
// filter, its roots by pointer jumping, the crown labels and the per-tree table.
// include/adamvs_hip.h "Trees" states the result; this file computes it with these kernels:
//
//   k_tree_mask         one lane per cell: the canopy byte, q and s0 (s is -1 outside the canopy, so that every later kernel
//                       reads one raster where it would read a surface and a mask).
//   k_tree_smooth       one binomial pass, one lane per cell (raster_prims.h binomial3x3; a hole is s < 0).  The last kernel of
//                       _tree_surface reduces the maximum of s per workgroup and issues an integer atomicMax only where the
//                       word it has just read is smaller.
//   k_tree_parents      the hot kernel; one workgroup of 16 waves per TREE_T x TREE_T tile (the candidates gather in the tiles
//                       of a rough canopy, hundreds in one and none in most; with 4 waves per tile the kernel took 0.24 ms
//                       on the bench raster, bound by those few tiles, with 16 it takes 0.14 ms).
//                       (a) s of the tile with a one-cell halo goes to LDS (66 x 66 words, 17 KB); every lane takes a cell,
//                           finds b(c) among its eight neighbours there and writes parent = b(c) where b(c) beats c.  The
//                           cells nothing beats (the 8-neighbour local maxima: about one in nine on noise, far fewer on a
//                           real canopy) are compacted into an LDS list by wave ballot.
//                       (b) the waves take candidates off the list in turn.  The 64 lanes of a wave cover the bounding box of
//                           the candidate's disc: floor(64 / (2 r + 1)) whole rows per step while a row fits into a wave (r <= 31,
//                           which is every window the defaults give below a gsd of 0.1 m), otherwise one row in pieces of
//                           64 columns.  The best key (s << 32 | ~index, so that one unsigned comparison is the order of
//                           step 3) is reduced across the wave by shuffles, and lane 0 writes parent = c for a top, the
//                           best cell of the window otherwise.
//                       LDS halo or L2 for the disc rows: L2.  A halo of TREE_MAX_RADIUS cells around a 64 x 64 tile is
//                       192 x 192 words = 147 KB of the CU's 160 KB, one workgroup per CU and nine times the tile loaded, to
//                       serve a list that holds a few percent of the tile's cells and whose windows are mostly a few cells
//                       wide; the rows a candidate's wave reads are short contiguous pieces of rows that this workgroup or a
//                       neighbouring one has just staged, so they come from L2 (k_bld_flags made the same choice for its
//                       stride reads).  There is no early exit from a sweep: a candidate that is no top needs the best
//                       cell of its whole window as its parent, so "beaten or not" is never all that is asked.
//   k_tree_jump         one round of pointer jumping, double-buffered: next(c) = the cell ADAMVS_TREE_JUMP_HOPS parents up
//                       from c in the previous round's buffer, stopping at a root.  A plain round of two hops halves the
//                       depth of the forest and costs 12 B per cell (the pointer, its gathered grandparent, the new
//                       pointer); the further hops are gathers a few cells away (a parent is a neighbour or lies within
//                       the window), taken only by the cells that have not arrived, and every round divides the depth by
//                       eight, so the bench raster settles in 3 rounds where two hops took 8 (0.25 ms, a third of the
//                       stage).  PLAIN jumping in this sense was built, not the variant that first resolves every cell
//                       to its tile exit in LDS; tools/trees_bench.py reports the rounds' share.  The host launches
//                       TREE_JUMP_CHUNK rounds, reads the rounds' changed words back once and stops at the first round
//                       that changed nothing; ADAMVS_TREE_MAX_ROUNDS bounds the loop.  A round that changes nothing
//                       leaves both buffers equal, so `root` holds the result whichever buffer the last round wrote.
//   k_tree_crowns       one lane per cell: the two tests against the cell's top, the label from the tops' numbering; the cells
//                       that fail are counted in LDS and added once per workgroup of 16 waves.
//   k_tree_table        as k_bld_table: a run of equal labels (raster_prims.h wave_run) is summed into its first lane, which
//                       issues the atomics.
//
// Every parent other than a root beats its child, so the parents are a forest whatever order the lanes ran in; integer
// atomicMin / atomicMax / atomicAdd commute: every output is bit-identical from run to run.  No workgroup waits on another;
// what one round of jumping writes is read by the next kernel.
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

constexpr int TREE_T = ADAMVS_TREE_TILE;
constexpr int TREE_LDS_W = TREE_T + 2;
constexpr int TREE_THREADS = 256;
constexpr int TREE_WAVES = TREE_THREADS / 64;
constexpr int TREE_PARENT_THREADS = 1024;    // 16 waves share a tile's candidates: the tiles inside a rough canopy hold hundreds
constexpr int TREE_PARENT_WAVES = TREE_PARENT_THREADS / 64;
constexpr int TREE_CROWN_THREADS = 1024;
constexpr int TREE_JUMP_CHUNK = 4;
static_assert(TREE_T == 64, "a wave takes one row of a tile");
static_assert(ADAMVS_TREE_MAX_RADIUS <= 64, "one ballot finds the window radius");
static_assert(ADAMVS_TREE_MAX_ROUNDS % TREE_JUMP_CHUNK == 0 && ADAMVS_TREE_MAX_ROUNDS <= 32, "the changed words fill 128 bytes");

// the control block at the head of the workspace
constexpr long TREE_OFF_CHANGED = 0;       // unsigned [ADAMVS_TREE_MAX_ROUNDS]
constexpr long TREE_OFF_TOPS = 128;        // unsigned long long
constexpr long TREE_OFF_CANDIDATES = 136;  // unsigned long long [2]: the candidates, the window cells read
constexpr long TREE_CONTROL = 256;

struct TreeThr {
  int v[ADAMVS_TREE_MAX_RADIUS];           // v[k] = thr[k + 1]; INT_MAX past r_cap
};

static inline unsigned tree_blocks(long n) { return (unsigned)((n + TREE_THREADS - 1) / TREE_THREADS); }

// The order of step 3 as one unsigned comparison: the larger key beats.  0 for a cell outside the canopy (s < 0), which
// nothing equals: idx < 2^28, so the low word of a canopy cell's key is never 0.
__device__ __forceinline__ unsigned long long tree_key(int s, unsigned idx) {
  return s < 0 ? 0ull : ((unsigned long long)(unsigned)s << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}
__device__ __forceinline__ int tree_key_cell(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// The largest v of the workgroup into *s_max.  Thousands of waves hold canopy and all their atomics would hit one address, so
// the waves are combined in LDS first, and the one lane left looks at the word before it adds: the word only grows, a stale
// look costs an atomic that changes nothing, and after the first few workgroups hardly any is issued.
__device__ __forceinline__ void tree_block_max(int v, int* s_max) {
  __shared__ int s_m[TREE_WAVES];
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < TREE_WAVES; ++k) v = s_m[k] > v ? s_m[k] : v;
    if (v > __hip_atomic_load(s_max, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(s_max, v);
  }
}

// ---- the surface ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TREE_THREADS) void k_tree_mask(long n, const float* __restrict__ ndsm, const int* __restrict__ building,
                                                            double min_height, uint8_t* __restrict__ mask, int* __restrict__ q,
                                                            int* __restrict__ s0, int* s_max) {
  const long c = (long)blockIdx.x * TREE_THREADS + threadIdx.x;      // no early return: every lane takes part in the shuffles
  int sv = -1;
  if (c < n) {
    const float v = ndsm[c];
    const bool canopy = __builtin_isfinite(v) && (double)v >= min_height && (building == nullptr || building[c] == 0);
    const int qv = canopy ? (int)llrint(fmin((double)v, 2047.0) * 256.0) : 0;
    sv = canopy ? qv : -1;
    mask[c] = canopy ? 1 : 0;
    q[c] = qv;
    s0[c] = sv;
  }
  if (s_max) tree_block_max(sv, s_max);                             // wave-uniform: a kernel argument
}

struct TreeHole {
  static constexpr int NONE = -1;
  static __device__ __forceinline__ bool is(int v) { return v < 0; }
};

__global__ __launch_bounds__(TREE_THREADS) void k_tree_smooth(int W, int H, const int* __restrict__ src, int* __restrict__ dst, int* s_max) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * TREE_THREADS + threadIdx.x;
  int out = -1;
  if (c < n) dst[c] = out = binomial3x3<TreeHole>(W, H, src, c);     // at most 16 * 2^23 = 2^27
  if (s_max) tree_block_max(out, s_max);
}

// ---- the parents ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TREE_PARENT_THREADS) void k_tree_parents(int W, int H, int tiles_x, const int* __restrict__ s, int r_cap, TreeThr thr,
                                                               int* __restrict__ parent, unsigned long long* counters) {
  __shared__ int s_t[TREE_LDS_W * TREE_LDS_W];
  __shared__ int s_list[TREE_T * TREE_T];
  __shared__ int s_thr[64];
  __shared__ int s_count;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int i0 = ty * TREE_T, j0 = tx * TREE_T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < TREE_LDS_W * TREE_LDS_W; k += TREE_PARENT_THREADS) {
    const int li = k / TREE_LDS_W, lj = k - li * TREE_LDS_W;
    const int gi = i0 + li - 1, gj = j0 + lj - 1;
    s_t[k] = (gi >= 0 && gi < H && gj >= 0 && gj < W) ? s[(long)gi * W + gj] : -1;
  }
  if (threadIdx.x < 64) s_thr[threadIdx.x] = threadIdx.x < ADAMVS_TREE_MAX_RADIUS ? thr.v[threadIdx.x] : INT_MAX;
  if (threadIdx.x == 0) s_count = 0;
  __syncthreads();
  // (a) b(c) from the tile, and the list of the cells nothing among their neighbours beats
  for (int r = wv; r < TREE_T; r += TREE_PARENT_WAVES) {                    // wave-uniform: every lane takes part in the ballot
    const int i = i0 + r, j = j0 + lane;
    const int sc = s_t[(r + 1) * TREE_LDS_W + lane + 1];
    bool cand = false;
    if (i < H && j < W) {
      const long c = (long)i * W + j;
      if (sc < 0) {
        parent[c] = -1;
      } else {
        const unsigned long long key_c = tree_key(sc, (unsigned)c);
        unsigned long long best = 0ull;
#pragma unroll
        for (int di = -1; di <= 1; ++di)
#pragma unroll
          for (int dj = -1; dj <= 1; ++dj) {
            if (di == 0 && dj == 0) continue;
            const int sn = s_t[(r + 1 + di) * TREE_LDS_W + lane + 1 + dj];    // -1 outside the grid: key 0
            const unsigned long long kn = tree_key(sn, (unsigned)(c + (long)di * W + dj));
            best = kn > best ? kn : best;
          }
        if (best > key_c) parent[c] = tree_key_cell(best);
        else cand = true;
      }
    }
    const unsigned long long bal = __ballot(cand);
    if (bal) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_count, __popcll(bal));
      base = __shfl(base, 0, 64);
      if (cand) s_list[base + __popcll(bal & ((1ull << lane) - 1ull))] = r * TREE_T + lane;
    }
  }
  __syncthreads();
  const int count = s_count;                                         // <= TREE_T * TREE_T: one entry per cell at most
  // (b) one wave per candidate: the best cell of its window
  unsigned swept = 0;
  for (int k = wv; k < count; k += TREE_PARENT_WAVES) {
    const int e = s_list[k];
    const int r = e >> 6, l = e & 63;
    const int i = i0 + r, j = j0 + l;
    const int sc = s_t[(r + 1) * TREE_LDS_W + l + 1];
    const long c = (long)i * W + j;
    const int rad = __popcll(__ballot(lane < r_cap && sc >= s_thr[lane]));     // thr ascends from 0 and sc >= 0: 1 <= rad <= r_cap
    const int rad2 = rad * rad, wb = 2 * rad + 1;
    const unsigned long long key_c = tree_key(sc, (unsigned)c);
    unsigned long long best = key_c;
    if (wb <= 64) {
      const int rpp = 64 / wb;                                       // whole rows of the bounding box per step
      const int lr = lane / wb, dj = lane - lr * wb - rad, jj = j + dj;
      const bool column = lr < rpp && jj >= 0 && jj < W;
      for (int d0 = -rad; d0 <= rad; d0 += rpp) {
        const int di = d0 + lr, ii = i + di;
        if (column && di <= rad && ii >= 0 && ii < H && di * di + dj * dj <= rad2) {
          const long cn = (long)ii * W + jj;
          const unsigned long long kn = tree_key(s[cn], (unsigned)cn);
          best = kn > best ? kn : best;
          ++swept;
        }
      }
    } else {
      for (int di = -rad; di <= rad; ++di) {
        const int ii = i + di;
        if (ii < 0 || ii >= H) continue;                             // wave-uniform
        for (int d0 = -rad; d0 <= rad; d0 += 64) {
          const int dj = d0 + lane, jj = j + dj;
          if (dj <= rad && jj >= 0 && jj < W && di * di + dj * dj <= rad2) {
            const long cn = (long)ii * W + jj;
            const unsigned long long kn = tree_key(s[cn], (unsigned)cn);
            best = kn > best ? kn : best;
            ++swept;
          }
        }
      }
    }
    for (int off = 32; off; off >>= 1) {
      const unsigned long long o = (unsigned long long)__shfl_xor((long long)best, off, 64);
      best = o > best ? o : best;
    }
    if (lane == 0) parent[c] = best == key_c ? (int)c : tree_key_cell(best);
  }
  for (int off = 32; off; off >>= 1) swept += __shfl_xor(swept, off, 64);       // a wave sweeps < 2^32 cells: 1024 lists of 2^14
  if (lane == 0 && swept) atomicAdd(counters + 1, (unsigned long long)swept);
  if (threadIdx.x == 0 && count) atomicAdd(counters, (unsigned long long)count);
}

// ---- the roots --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TREE_THREADS) void k_tree_jump(long n, const int* __restrict__ cur, int* __restrict__ nxt, unsigned* changed,
                                                            unsigned long long* tops) {
  const long c = (long)blockIdx.x * TREE_THREADS + threadIdx.x;
  bool moved = false, top = false;
  if (c < n) {
    const int p = cur[c];
    int out = -1;
    if (p >= 0 && (long)p < n) {                                     // anything else is "outside the canopy"
      out = p;
      for (int h = 1; h < ADAMVS_TREE_JUMP_HOPS; ++h) {              // `cur` is not written in this kernel
        const int g = cur[out];
        if (g == out || g < 0 || (long)g >= n) break;                // a root (or a pointer out of the forest): stay
        out = g;
      }
      top = (long)p == c;
    }
    nxt[c] = out;
    moved = out != p;
  }
  if (__ballot(moved) != 0ull && (threadIdx.x & 63) == 0) changed[0] = 1u;
  if (tops) {
    const unsigned long long bal = __ballot(top);
    if (bal && (threadIdx.x & 63) == 0) atomicAdd(tops, (unsigned long long)__popcll(bal));
  }
}

// ---- the crowns -------------------------------------------------------------------------------------------------------------
// Workgroups of 16 waves: the cells that fail a test lie in bands around every crown, a few in each of very many waves, and one
// atomicAdd per wave would send them all to one address (what the growth counter of dsm_roofs.hip met); they are summed in LDS
// and added once per workgroup.
__global__ __launch_bounds__(TREE_CROWN_THREADS) void k_tree_crowns(int W, int H, const int* __restrict__ s, const int* __restrict__ root,
                                                                    const int* __restrict__ number, int ratio_pm, long long rc2,
                                                                    int* __restrict__ label, unsigned long long* unassigned) {
  __shared__ unsigned s_failed;
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * TREE_CROWN_THREADS + threadIdx.x;
  if (threadIdx.x == 0) s_failed = 0u;
  __syncthreads();
  bool failed = false;
  if (c < n) {
    const int t = root[c];
    int lab = 0;
    if (t >= 0 && (long)t < n) {
      int i, j, it, jt;
      cell_ij(c, W, i, j);
      cell_ij(t, W, it, jt);
      const long long di = i - it, dj = j - jt;
      const bool ok = (long long)s[c] * 1000 >= (long long)ratio_pm * (long long)s[t] && di * di + dj * dj <= rc2;
      if (ok) lab = number[t];
      failed = !ok;
    }
    label[c] = lab;
  }
  const unsigned long long bal = __ballot(failed);
  if (bal && (threadIdx.x & 63) == 0) atomicAdd(&s_failed, (unsigned)__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0 && s_failed) atomicAdd(unassigned, (unsigned long long)s_failed);
}

// ---- the table --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TREE_THREADS) void k_tree_table(int W, int H, const int* __restrict__ label, const int* __restrict__ q,
                                                             const int* __restrict__ s, const int* __restrict__ root, long T, long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * TREE_THREADS + threadIdx.x;      // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int lab = 0, i = 0, j = 0, t = -1, q_max = -1;
  unsigned long long q_sum = 0;
  long long r2 = -1;
  if (c < n) {
    lab = label[c];
    if (lab < 1 || (long)lab > T) lab = 0;
    if (lab) {
      t = root[c];
      if (t < 0 || (long)t >= n) lab = 0;                            // a label without a top is no label
    }
  }
  if (__ballot(lab != 0) == 0ull) return;                            // wave-uniform
  if (lab) {
    int it, jt;
    cell_ij(c, W, i, j);
    cell_ij(t, W, it, jt);
    const long long di = i - it, dj = j - jt;
    r2 = di * di + dj * dj;
    q_max = q[c];
    q_sum = (unsigned long long)(q_max > 0 ? q_max : 0);
  }
  bool head;
  int end;
  wave_run(lab, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const int t_qmax = __shfl_down(q_max, off, 64);
    const unsigned long long t_qsum = (unsigned long long)__shfl_down((long long)q_sum, off, 64);
    const long long t_r2 = __shfl_down(r2, off, 64);
    if (lane + off <= end) {
      q_sum += t_qsum;
      q_max = t_qmax > q_max ? t_qmax : q_max;
      r2 = t_r2 > r2 ? t_r2 : r2;
    }
  }
  if (!head) return;
  const long k = lab - 1;
  const int len = end - lane + 1;
  add_nonzero(table + ADAMVS_TREE_CELLS * T + k, len);
  add_nonzero(table + ADAMVS_TREE_Q_SUM * T + k, (long long)q_sum);
  atomicMax(table + ADAMVS_TREE_Q_MAX * T + k, (long long)q_max);
  atomicMin(table + ADAMVS_TREE_ROW_MIN * T + k, (long long)i);
  atomicMax(table + ADAMVS_TREE_ROW_MAX * T + k, (long long)i);
  atomicMin(table + ADAMVS_TREE_COL_MIN * T + k, (long long)j);
  atomicMax(table + ADAMVS_TREE_COL_MAX * T + k, (long long)(j + len - 1));
  atomicMax(table + ADAMVS_TREE_R2_MAX * T + k, r2);
  atomicMax(table + ADAMVS_TREE_TOP * T + k, (long long)t);
  atomicMax(table + ADAMVS_TREE_S_TOP * T + k, (long long)s[t]);
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// Workspace: the control block, then two int32 rasters (the surface's two intermediate passes; the jumping's second buffer).
long tree_workspace_bytes(int W, int H) { return TREE_CONTROL + 2 * align256(4L * W * H); }

int launch_tree_surface(int W, int H, const float* ndsm, const int* building, double min_height, int smooth_passes, void* workspace,
                        uint8_t* mask, int* q, int* s, int* s_max, hipStream_t st) {
  const long n = (long)W * H;
  int* tmp[2] = {(int*)((char*)workspace + TREE_CONTROL), (int*)((char*)workspace + TREE_CONTROL + align256(4 * n))};
  const hipError_t e = hipMemsetAsync(s_max, 0xFF, sizeof(int), st);       // -1: no canopy
  if (e != hipSuccess) return set_error((int)e, "tree_surface: %s", hipGetErrorString(e));
  int* dst = smooth_passes == 0 ? s : tmp[0];
  hipLaunchKernelGGL(k_tree_mask, dim3(tree_blocks(n)), dim3(TREE_THREADS), 0, st, n, ndsm, building, min_height, mask, q, dst,
                     smooth_passes == 0 ? s_max : (int*)nullptr);
  ADAMVS_CHECK_LAUNCH("tree_mask");
  for (int k = 0; k < smooth_passes; ++k) {
    const bool last = k == smooth_passes - 1;
    const int* src = dst;
    dst = last ? s : tmp[1];
    hipLaunchKernelGGL(k_tree_smooth, dim3(tree_blocks(n)), dim3(TREE_THREADS), 0, st, W, H, src, dst, last ? s_max : (int*)nullptr);
    ADAMVS_CHECK_LAUNCH("tree_smooth");
  }
  return 0;
}

int launch_tree_parents(int W, int H, const int* s, int r_cap, const int* thr, void* workspace, int* parent, adamvs_tree_stats* stats,
                        hipStream_t st) {
  TreeThr t;
  for (int k = 0; k < ADAMVS_TREE_MAX_RADIUS; ++k) t.v[k] = k < r_cap ? thr[k] : INT_MAX;
  const int tiles_x = cdiv(W, TREE_T), tiles_y = cdiv(H, TREE_T);
  unsigned long long* counters = (unsigned long long*)((char*)workspace + TREE_OFF_CANDIDATES);
  unsigned long long host[2] = {0, 0};
  BldClock clock;
  hipError_t e = hipMemsetAsync(counters, 0, sizeof(host), st);
  if (e != hipSuccess) return set_error((int)e, "tree_parents: %s", hipGetErrorString(e));
  clock.mark(0, st);
  hipLaunchKernelGGL(k_tree_parents, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(TREE_PARENT_THREADS), 0, st, W, H, tiles_x, s, r_cap, t, parent,
                     counters);
  ADAMVS_CHECK_LAUNCH("tree_parents");
  clock.mark(1, st);
  e = hipMemcpyAsync(host, counters, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "tree_parents: %s", hipGetErrorString(e));
  stats->candidates = (long)host[0];
  stats->window_cells = (long)host[1];
  stats->ms_parents = clock.ms(0);
  return 0;
}

int launch_tree_roots(int W, int H, const int* parent, void* workspace, int* root, adamvs_tree_stats* stats, hipStream_t st) {
  const long n = (long)W * H;
  unsigned* changed = (unsigned*)((char*)workspace + TREE_OFF_CHANGED);
  unsigned long long* tops = (unsigned long long*)((char*)workspace + TREE_OFF_TOPS);
  int* other = (int*)((char*)workspace + TREE_CONTROL);
  struct {
    unsigned changed[ADAMVS_TREE_MAX_ROUNDS];
    unsigned long long tops;
  } host;
  static_assert(sizeof(host) == TREE_OFF_TOPS + 8, "the read-back is the head of the control block");
  stats->rounds = 0;
  stats->converged = 0;
  stats->tops = 0;
  BldClock clock;
  hipError_t e = hipMemsetAsync(workspace, 0, sizeof(host), st);
  if (e != hipSuccess) return set_error((int)e, "tree_roots: %s", hipGetErrorString(e));
  clock.mark(0, st);
  for (int done = 0; done < ADAMVS_TREE_MAX_ROUNDS && !stats->converged; done += TREE_JUMP_CHUNK) {
    for (int k = done; k < done + TREE_JUMP_CHUNK; ++k) {            // round 0: parent -> root; odd: root -> other; even: other -> root
      const int* cur = k == 0 ? parent : (k & 1) ? root : other;
      int* nxt = (k & 1) ? other : root;
      hipLaunchKernelGGL(k_tree_jump, dim3(tree_blocks(n)), dim3(TREE_THREADS), 0, st, n, cur, nxt, changed + k,
                         k == 0 ? tops : (unsigned long long*)nullptr);
      ADAMVS_CHECK_LAUNCH("tree_jump");
    }
    e = hipMemcpyAsync(&host, workspace, sizeof(host), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return set_error((int)e, "tree_roots: %s", hipGetErrorString(e));
    for (int k = done; k < done + TREE_JUMP_CHUNK && !stats->converged; ++k) {
      if (host.changed[k]) stats->rounds = k + 1;
      else stats->converged = 1;
    }
  }
  clock.mark(1, st);
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "tree_roots: %s", hipGetErrorString(e));
  stats->tops = (long)host.tops;
  stats->ms_jump = clock.ms(0);
  if (!stats->converged) return set_error(ADAMVS_TREE_NOT_CONVERGED, "tree_roots: pointers still moving after %d rounds", ADAMVS_TREE_MAX_ROUNDS);
  return 0;
}

int launch_tree_crowns(int W, int H, const int* s, const int* root, const int* number, int ratio_pm, long rc2, int* label,
                       long long* unassigned, hipStream_t st) {
  const hipError_t e = hipMemsetAsync(unassigned, 0, sizeof(long long), st);
  if (e != hipSuccess) return set_error((int)e, "tree_crowns: %s", hipGetErrorString(e));
  const long n = (long)W * H;
  hipLaunchKernelGGL(k_tree_crowns, dim3((unsigned)((n + TREE_CROWN_THREADS - 1) / TREE_CROWN_THREADS)), dim3(TREE_CROWN_THREADS), 0, st, W, H, s, root, number, ratio_pm, (long long)rc2,
                     label, (unsigned long long*)unassigned);
  ADAMVS_CHECK_LAUNCH("tree_crowns");
  return 0;
}

int launch_tree_table(int W, int H, const int* label, const int* q, const int* s, const int* root, long T, long long* table, hipStream_t st) {
  if (T == 0) return 0;
  const TableStart start = TableStart(ADAMVS_TREE_COLUMNS, -1)       // the maxima
                               .set(0, {ADAMVS_TREE_CELLS, ADAMVS_TREE_Q_SUM})
                               .set(TABLE_MIN_START, {ADAMVS_TREE_ROW_MIN, ADAMVS_TREE_COL_MIN});
  if (int rc = launch_table_init("tree_table_init", T, start, table, st)) return rc;
  hipLaunchKernelGGL(k_tree_table, dim3(tree_blocks((long)W * H)), dim3(TREE_THREADS), 0, st, W, H, label, q, s, root, T, table);
  ADAMVS_CHECK_LAUNCH("tree_table");
  return 0;
}

}  // namespace adamvs
