// LoD2 solids: the model labels (roof labels filled over the whole building), the per-building table and the boundary runs of the
// model labels with the heights of both sides at either end.  include/adamvs_hip.h "LoD2 solids" states the result; this file
// computes it with these kernels:
//
//   k_lod2_fill         one round: every cell of the output buffer is written (the label kept, the smallest neighbouring plane
//                       of the same building, or 0 off the buildings).  One atomicAdd per workgroup of 16 waves counts the
//                       cells labelled (k_roof_grow's scheme).
//   k_lod2_table        one lane per cell; a run of equal building labels in a wave (raster_prims.h wave_run) is reduced into its
//                       first lane, which issues the integer atomics.
//   k_lod2_transpose    32 x 32 tiles through LDS (33 words per row: the column read is free of bank conflicts), both sides
//                       coalesced.  With it the vertical lattice lines are rows of a raster as the horizontal ones are, and one
//                       edge kernel serves both orientations with 256-byte row segments per wave.
//   k_lod2_count /      a workgroup takes LOD2_BLOCK consecutive edges of an orientation in (line, pos) order.  Every lane reads
//   k_lod2_runs         the labels above and below its edge (two coalesced row segments) and puts the pair into LDS, the first
//                       and the last lane also the pair of the edge before and after the workgroup's.  A head is a boundary edge
//                       whose predecessor on the line is not one of the same pair, a tail likewise towards its successor.  The
//                       count kernel stores the heads per workgroup, launch_fusion_scan (fusion.hip) scans them, the emit kernel
//                       ranks heads and tails (block_prims.h block_rank): head h and the tail that closes it write the two
//                       halves of record h.  No atomics, no walk along a run, the order is the scan's.
//
// Only integer atomics that commute, so every output is bit-identical from run to run.
#include <math.h>

#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "lod2_plane.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

constexpr int LOD2_THREADS = 256;                                    // bld_union.h's BLD_THREADS: four waves
constexpr int LOD2_BLOCK = ADAMVS_LOD2_BLOCK;
static_assert(LOD2_BLOCK == LOD2_THREADS, "one lane per edge; block_rank ranks over four waves");
static_assert(ADAMVS_LOD2_COLUMNS <= TABLE_MAX_COLUMNS, "TableStart holds the building table's columns");

static inline unsigned lod2_blocks(long n) { return (unsigned)((n + LOD2_THREADS - 1) / LOD2_THREADS); }

// a label outside 1 .. P reads as 0
__device__ __forceinline__ int lod2_label(int v, long P) { return (v < 1 || (long)v > P) ? 0 : v; }

// ---- model labels -----------------------------------------------------------------------------------------------------------
constexpr int LOD2_FILL_THREADS = 1024;

__global__ __launch_bounds__(LOD2_FILL_THREADS) void k_lod2_fill(int W, int H, const int* __restrict__ bld, long P,
                                                                 const int* __restrict__ src, int* __restrict__ dst, unsigned* count) {
  __shared__ unsigned s_taken;
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * LOD2_FILL_THREADS + threadIdx.x;
  bool taken = false;
  if (threadIdx.x == 0) s_taken = 0;
  __syncthreads();
  if (c < n) {
    const int b = bld[c];
    int lab = b > 0 ? lod2_label(src[c], P) : 0;
    if (b > 0 && lab == 0) {
      int i, j;
      cell_ij(c, W, i, j);
      int best = 0;
      const int di[4] = {-1, 0, 0, 1}, dj[4] = {0, -1, 1, 0};
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int ii = i + di[d], jj = j + dj[d];
        if (ii < 0 || ii >= H || jj < 0 || jj >= W) continue;
        const long cn = (long)ii * W + jj;
        const int p = lod2_label(src[cn], P);
        if (p == 0 || bld[cn] != b) continue;
        if (best == 0 || p < best) best = p;
      }
      if (best) lab = best, taken = true;
    }
    dst[c] = lab;
  }
  const unsigned long long bal = __ballot(taken);                    // every lane of the workgroup arrives here
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&s_taken, (unsigned)__popcll(bal));
  __syncthreads();
  if (threadIdx.x == 0 && s_taken) atomicAdd(count, s_taken);
}

// ---- building table ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOD2_THREADS) void k_lod2_table(int W, int H, const float* __restrict__ dtm, const int* __restrict__ bld,
                                                             const int* __restrict__ label, double z_ref, long B, long P,
                                                             const long long* __restrict__ planes, long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * LOD2_THREADS + threadIdx.x;      // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int b = 0, j = 0;
  if (c < n) {
    b = bld[c];
    if (b < 1 || (long)b > B) b = 0;
  }
  if (__ballot(b != 0) == 0ull) return;                              // wave-uniform: a wave off the buildings adds nothing
  long long filled = 0, base = TABLE_MIN_START, roof = TABLE_MIN_START;
  if (b) {
    int i;
    cell_ij(c, W, i, j);
    const float fz = dtm[c];
    if (__builtin_isfinite(fz)) base = (long long)fmin(fmax(floor(((double)fz - z_ref) * 1024.0), -1073741824.0), 1073741824.0);
    const int lab = lod2_label(label[c], P);
    if (lab) {
      filled = 1;
      const long long* pl = planes + 3L * (lab - 1);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long long z = lod2_corner_height(pl, i + (k >> 1), j + (k & 1));
        roof = z < roof ? z : roof;
      }
    }
  }
  bool head;
  int end;
  wave_run(b, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const long long t_filled = __shfl_down(filled, off, 64), t_base = __shfl_down(base, off, 64), t_roof = __shfl_down(roof, off, 64);
    if (lane + off <= end) {
      filled += t_filled;
      base = t_base < base ? t_base : base;
      roof = t_roof < roof ? t_roof : roof;
    }
  }
  if (!head) return;
  const long k = b - 1;
  add_nonzero(table + ADAMVS_LOD2_CELLS * B + k, (long long)(end - lane + 1));
  add_nonzero(table + ADAMVS_LOD2_FILLED * B + k, filled);
  if (base < TABLE_MIN_START) atomicMin(table + ADAMVS_LOD2_BASE * B + k, base);
  if (roof < TABLE_MIN_START) atomicMin(table + ADAMVS_LOD2_ROOF_MIN * B + k, roof);
}

// ---- transpose --------------------------------------------------------------------------------------------------------------
constexpr int LOD2_TP = 32;                                          // tile side; 256 lanes take 8 rows at a time

__global__ __launch_bounds__(LOD2_THREADS) void k_lod2_transpose(int W, int H, const int* __restrict__ src, int* __restrict__ dst) {
  __shared__ int tile[LOD2_TP][LOD2_TP + 1];
  const int tx = threadIdx.x & (LOD2_TP - 1), ty = threadIdx.x / LOD2_TP;
  const int j0 = blockIdx.x * LOD2_TP, i0 = blockIdx.y * LOD2_TP;
  for (int r = ty; r < LOD2_TP; r += LOD2_THREADS / LOD2_TP) {
    const int i = i0 + r, j = j0 + tx;
    if (i < H && j < W) tile[r][tx] = src[(long)i * W + j];
  }
  __syncthreads();
  for (int r = ty; r < LOD2_TP; r += LOD2_THREADS / LOD2_TP) {
    const int j = j0 + r, i = i0 + tx;                               // dst row j (a column of src), dst column i
    if (i < H && j < W) dst[(long)j * H + i] = tile[tx][r];
  }
}

// ---- boundary runs ----------------------------------------------------------------------------------------------------------
// The edges of one orientation over a raster lab [Hh][Ww]: line k = 0 .. Hh between the rows k - 1 ("up") and k ("dn"), positions
// 0 .. Ww - 1; edge e = k Ww + pos.  (Hh + 1) Ww <= 2^28 + 2^15, so e and the division are 32-bit.
struct Lod2Edge {
  int k, pos, up, dn;
  bool head, tail, cont;                                             // cont: a boundary edge that continues its predecessor's run
};

__device__ __forceinline__ void lod2_pair(int Ww, int Hh, const int* __restrict__ lab, long P, unsigned e, int& k, int& pos, int& up,
                                          int& dn) {
  k = (int)(e / (unsigned)Ww);
  pos = (int)(e - (unsigned)k * (unsigned)Ww);
  up = k > 0 ? lod2_label(lab[(long)(k - 1) * Ww + pos], P) : 0;
  dn = k < Hh ? lod2_label(lab[(long)k * Ww + pos], P) : 0;
}

// Every lane of the workgroup calls it (LDS and a barrier inside).  block: the workgroup's number within its orientation.
__device__ __forceinline__ Lod2Edge lod2_edge(int Ww, int Hh, const int* __restrict__ lab, long P, unsigned block) {
  __shared__ int s_up[LOD2_BLOCK + 2], s_dn[LOD2_BLOCK + 2];
  const unsigned n_edges = (unsigned)(Hh + 1) * (unsigned)Ww;
  const unsigned e0 = block * (unsigned)LOD2_BLOCK, e = e0 + threadIdx.x;
  const int t = threadIdx.x;
  Lod2Edge g;
  g.k = g.pos = g.up = g.dn = 0;
  if (e < n_edges) lod2_pair(Ww, Hh, lab, P, e, g.k, g.pos, g.up, g.dn);
  s_up[t + 1] = g.up, s_dn[t + 1] = g.dn;
  if (t == 0 || t == LOD2_BLOCK - 1) {                               // the neighbours outside the workgroup's edges
    const bool before = t == 0;
    int k = 0, pos = 0, up = 0, dn = 0;
    if (before ? e0 > 0 : e0 + LOD2_BLOCK < n_edges) lod2_pair(Ww, Hh, lab, P, before ? e0 - 1 : e0 + LOD2_BLOCK, k, pos, up, dn);
    const int slot = before ? 0 : LOD2_BLOCK + 1;
    s_up[slot] = up, s_dn[slot] = dn;
  }
  __syncthreads();
  const bool boundary = e < n_edges && g.up != g.dn;                 // an equal pair next to it is then a boundary edge too
  const bool same_prev = g.pos > 0 && s_up[t] == g.up && s_dn[t] == g.dn;
  const bool same_next = g.pos < Ww - 1 && s_up[t + 2] == g.up && s_dn[t + 2] == g.dn;
  g.head = boundary && !same_prev;
  g.tail = boundary && !same_next;
  g.cont = boundary && same_prev;
  return g;
}

__global__ __launch_bounds__(LOD2_THREADS) void k_lod2_count(int Ww, int Hh, const int* __restrict__ lab, long P,
                                                             unsigned* __restrict__ counts) {
  const Lod2Edge g = lod2_edge(Ww, Hh, lab, P, blockIdx.x);
  unsigned total;
  block_rank(g.head, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// the height of side q at corner (r, c); the other side's base where q is outside
__device__ __forceinline__ int lod2_side(const long long* __restrict__ planes, const int* __restrict__ plane_base, int q, int other, int r,
                                         int c) {
  return q ? (int)lod2_corner_height(planes + 3L * (q - 1), r, c) : plane_base[other - 1];
}

template <bool VERTICAL>
__global__ __launch_bounds__(LOD2_THREADS) void k_lod2_runs(int Ww, int Hh, const int* __restrict__ lab, long P,
                                                            const long long* __restrict__ planes, const int* __restrict__ plane_base,
                                                            const unsigned* __restrict__ offsets, long N, int* __restrict__ rec) {
  __shared__ unsigned s_cont0;
  const Lod2Edge g = lod2_edge(Ww, Hh, lab, P, blockIdx.x);
  if (threadIdx.x == 0) s_cont0 = g.cont ? 1u : 0u;
  unsigned heads, tails;
  const unsigned hr = block_rank(g.head, &heads);
  __syncthreads();                                                   // block_rank's LDS words are read before they are set again
  const unsigned tr = block_rank(g.tail, &tails);
  const long first = offsets[blockIdx.x];
  const int L = VERTICAL ? g.dn : g.up, R = VERTICAL ? g.up : g.dn;  // the left of a line that runs south is the east
  if (g.head) {
    const long h = first + hr;
    const int r = VERTICAL ? g.pos : g.k, c = VERTICAL ? g.k : g.pos;
    if (h < N) {
      rec[ADAMVS_LOD2_F_ORIENTATION * N + h] = VERTICAL ? 1 : 0;
      rec[ADAMVS_LOD2_F_LINE * N + h] = g.k;
      rec[ADAMVS_LOD2_F_START * N + h] = g.pos;
      rec[ADAMVS_LOD2_F_L * N + h] = L;
      rec[ADAMVS_LOD2_F_R * N + h] = R;
      rec[ADAMVS_LOD2_F_ZL_S * N + h] = lod2_side(planes, plane_base, L, R, r, c);
      rec[ADAMVS_LOD2_F_ZR_S * N + h] = lod2_side(planes, plane_base, R, L, r, c);
    }
  }
  if (g.tail) {
    const long h = first - (long)s_cont0 + tr;                       // >= 0: a tail with tr = 0 closes the run that came in
    const int r = VERTICAL ? g.pos + 1 : g.k, c = VERTICAL ? g.k : g.pos + 1;
    if (h >= 0 && h < N) {
      rec[ADAMVS_LOD2_F_END * N + h] = g.pos + 1;
      rec[ADAMVS_LOD2_F_ZL_E * N + h] = lod2_side(planes, plane_base, L, R, r, c);
      rec[ADAMVS_LOD2_F_ZR_E * N + h] = lod2_side(planes, plane_base, R, L, r, c);
    }
  }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static inline long lod2_edges_h(int W, int H) { return (long)(H + 1) * W; }
static inline long lod2_edges_v(int W, int H) { return (long)(W + 1) * H; }

// Workspace of _lod2_count and _lod2_runs: the heads per workgroup (horizontal first), then their exclusive scan and the total.
long lod2_workspace_bytes(int W, int H) {
  const long nb = (long)lod2_blocks(lod2_edges_h(W, H)) + lod2_blocks(lod2_edges_v(W, H));
  return align256(4 * nb) + align256(4 * (nb + 1));
}

int launch_lod2_fill(int W, int H, const int* building, long P, int round0, int rounds, int* label0, int* label1, unsigned* counts,
                     hipStream_t st) {
  if (rounds == 0) return 0;
  const hipError_t e = hipMemsetAsync(counts + round0, 0, sizeof(unsigned) * rounds, st);
  if (e != hipSuccess) return set_error((int)e, "lod2_fill: %s", hipGetErrorString(e));
  const unsigned blocks = (unsigned)(((long)W * H + LOD2_FILL_THREADS - 1) / LOD2_FILL_THREADS);
  for (int k = round0; k < round0 + rounds; ++k) {
    hipLaunchKernelGGL(k_lod2_fill, dim3(blocks), dim3(LOD2_FILL_THREADS), 0, st, W, H, building, P, (const int*)((k & 1) ? label1 : label0),
                       (k & 1) ? label0 : label1, counts + k);
    ADAMVS_CHECK_LAUNCH("lod2_fill");
  }
  return 0;
}

int launch_lod2_table(int W, int H, const float* dtm, const int* building, const int* label, double z_ref, long B, long P,
                      const long long* planes, long long* table, hipStream_t st) {
  if (B == 0) return 0;
  const TableStart start = TableStart(ADAMVS_LOD2_COLUMNS).set(TABLE_MIN_START, {ADAMVS_LOD2_BASE, ADAMVS_LOD2_ROOF_MIN});
  if (int rc = launch_table_init("lod2_table_init", B, start, table, st)) return rc;
  hipLaunchKernelGGL(k_lod2_table, dim3(lod2_blocks((long)W * H)), dim3(LOD2_THREADS), 0, st, W, H, dtm, building, label, z_ref, B, P, planes,
                     table);
  ADAMVS_CHECK_LAUNCH("lod2_table");
  return 0;
}

int launch_lod2_transpose(int W, int H, const int* src, int* dst, hipStream_t st) {
  hipLaunchKernelGGL(k_lod2_transpose, dim3((unsigned)cdiv(W, LOD2_TP), (unsigned)cdiv(H, LOD2_TP)), dim3(LOD2_THREADS), 0, st, W, H, src, dst);
  ADAMVS_CHECK_LAUNCH("lod2_transpose");
  return 0;
}

int launch_lod2_count(int W, int H, const int* label, const int* label_t, long P, void* workspace, unsigned* total, hipStream_t st) {
  const unsigned nb_h = lod2_blocks(lod2_edges_h(W, H)), nb_v = lod2_blocks(lod2_edges_v(W, H));
  const long nb = (long)nb_h + nb_v;
  unsigned* counts = (unsigned*)workspace;
  unsigned* offsets = (unsigned*)((char*)workspace + align256(4 * nb));
  hipLaunchKernelGGL(k_lod2_count, dim3(nb_h), dim3(LOD2_THREADS), 0, st, W, H, label, P, counts);
  ADAMVS_CHECK_LAUNCH("lod2_count");
  hipLaunchKernelGGL(k_lod2_count, dim3(nb_v), dim3(LOD2_THREADS), 0, st, H, W, label_t, P, counts + nb_h);
  ADAMVS_CHECK_LAUNCH("lod2_count");
  if (int rc = launch_fusion_scan(counts, offsets, (int)nb, st)) return rc;
  const hipError_t e = hipMemcpyAsync(total, offsets + nb, sizeof(unsigned), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) return set_error((int)e, "lod2_count: %s", hipGetErrorString(e));
  return 0;
}

int launch_lod2_runs(int W, int H, const int* label, const int* label_t, long P, const long long* planes, const int* plane_base, long N,
                     void* workspace, int* records, hipStream_t st) {
  if (N == 0) return 0;
  const unsigned nb_h = lod2_blocks(lod2_edges_h(W, H)), nb_v = lod2_blocks(lod2_edges_v(W, H));
  const long nb = (long)nb_h + nb_v;
  const unsigned* offsets = (const unsigned*)((char*)workspace + align256(4 * nb));
  hipLaunchKernelGGL(k_lod2_runs<false>, dim3(nb_h), dim3(LOD2_THREADS), 0, st, W, H, label, P, planes, plane_base, offsets, N, records);
  ADAMVS_CHECK_LAUNCH("lod2_runs");
  hipLaunchKernelGGL(k_lod2_runs<true>, dim3(nb_v), dim3(LOD2_THREADS), 0, st, H, W, label_t, P, planes, plane_base, offsets + nb_h, N, records);
  ADAMVS_CHECK_LAUNCH("lod2_runs");
  return 0;
}

}  // namespace adamvs
