// The tiled 4-connected component labelling of the raster stages, once: the building stage labels a mask (dsm_buildings.hip),
// the roof stage a raster of link bits (dsm_roofs.hip), and a mask is a link raster with every edge present.  An edge policy
// reads a cell's byte and says whether the cell is a node and whether it is joined to its east and to its south neighbour
// (an edge needs both ends to be nodes; the labelling checks the other end).  Templated on it:
//
//   k_label_tile    one workgroup per BLD_TILE_W x BLD_TILE_H tile, all of it in LDS.  A wave takes a row: the ballots of the
//                   nodes and of the east bits give the edges of the row (bit k: cells k and k + 1 are joined), and a lane's
//                   first label is the first cell of its run, the cell after the nearest missing edge on its left.  Every lane
//                   keeps the south bits of its wave's rows in one register (none where all nodes are joined); that both ends
//                   are nodes is read from the signs of their LDS entries, so a cell's byte is read once and no other row's.
//                   Then passes over the vertical edges: both cells walk to their roots, the larger root gets atomicMin(smaller) (LDS), until a pass finds
//                   no edge with two roots.  Every such pass takes a root away, so there are fewer passes than cells; the loop
//                   is bounded by that count.  A label only ever points to a smaller index of the same component, so every
//                   walk ends.  Written: the global index of the tile-local root.
//   k_label_pairs   one round's first kernel over the pairs of adjacent cells either side of a tile border: it reads both
//                   parents (roots: the tile phase and k_bld_compress leave border cells flat) and stores (smaller, larger)
//                   where the pair is joined and the roots differ.
//   launch_label    the tile kernel, then rounds of k_label_pairs / k_bld_hook (atomicMin(parent[larger], smaller)) /
//                   k_bld_compress (both cells of every pair to the root, block_prims.h compress_to_root).  Three launches, so
//                   that the reads of a round see the state the previous round left: the per-XCD L2s are not coherent for
//                   plain loads inside one kernel.  The host reads one word per round and stops at the first round without a
//                   differing pair, or at the cap.  Then k_bld_compress_all: every cell to its root.
//
// k_bld_hook, k_bld_compress and k_bld_compress_all do not look at the cells' bytes; they live in dsm_buildings.hip once.
//
// parent[x] <= x holds throughout, a hook joins only cells of one component, and the rounds end only when every joined border
// pair has one root: then each component has a single root, its smallest cell.  That is a property of the components alone,
// so the labels do not depend on the order in which edges are united (which wave takes which vertical edge, which policy
// supplied the edge): both stages get bit for bit what their own kernels gave.
#pragma once
#include <hip/hip_runtime.h>

#include "block_prims.h"
#include "common.h"
#include "kernels.h"

namespace adamvs {

constexpr int BLD_THREADS = 256;
constexpr int BLD_CELLS = BLD_TILE_W * BLD_TILE_H;
static_assert(BLD_TILE_W == 64, "a wave takes one row of a tile");
static_assert(BLD_TILE_H % (BLD_THREADS / 64) == 0, "the waves share the rows of a tile evenly");

static inline unsigned bld_blocks(long n) { return (unsigned)((n + BLD_THREADS - 1) / BLD_THREADS); }

static inline long bld_pairs_count(int W, int H, long* n_vertical) {
  const long v = (long)H * (cdiv(W, BLD_TILE_W) - 1), h = (long)W * (cdiv(H, BLD_TILE_H) - 1);
  if (n_vertical) *n_vertical = v;
  return v + h;
}

// Pair p: first the pairs across the vertical borders (columns x - 1 | x, x a multiple of BLD_TILE_W; H per border), then
// those across the horizontal borders (W per border).
__device__ __forceinline__ void bld_pair_cells(long p, int W, int H, long n_vertical, long& a, long& b) {
  if (p < n_vertical) {
    const long border = p / H;
    const long i = p - border * H;
    b = i * W + (border + 1) * BLD_TILE_W;
    a = b - 1;
  } else {
    const long q = p - n_vertical;
    const long border = q / W;
    const long jj = q - border * W;
    b = (border + 1) * BLD_TILE_H * (long)W + jj;
    a = b - W;
  }
}

// the root of cell v in a forest nobody writes during this kernel (strictly downwards, so it ends)
__device__ __forceinline__ int bld_root(const int* __restrict__ parent, int v) {
  for (int q = parent[v]; q >= 0 && q < v; q = parent[v]) v = q;
  return v;
}

__device__ __forceinline__ int bld_lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// the root of x in LDS: labels point strictly downwards until the root, which points to itself
__device__ __forceinline__ int bld_find(const int* l, int x) {
  for (int p = bld_lds_load(l + x); p != x; p = bld_lds_load(l + x)) x = p;
  return x;
}

// ---- the edge policies ------------------------------------------------------------------------------------------------------
// a mask: flags >= 2 is a node, and every two adjacent nodes are joined (all_joined: the tile kernel then keeps no south bits)
struct MaskEdges {
  static constexpr const char* name = "bld";
  static constexpr bool all_joined = true;
  static __device__ __forceinline__ bool node(uint8_t f) { return f >= 2; }
  static __device__ __forceinline__ bool east(uint8_t) { return true; }
  static __device__ __forceinline__ bool south(uint8_t) { return true; }
};
// link bits: 1 the cell is core, 2 joined to its east neighbour, 4 to its south neighbour
struct LinkEdges {
  static constexpr const char* name = "roof";
  static constexpr bool all_joined = false;
  static __device__ __forceinline__ bool node(uint8_t f) { return (f & 1) != 0; }
  static __device__ __forceinline__ bool east(uint8_t f) { return (f & 2) != 0; }
  static __device__ __forceinline__ bool south(uint8_t f) { return (f & 4) != 0; }
};

// ---- the tile phase ---------------------------------------------------------------------------------------------------------
template <class Edges>
__global__ __launch_bounds__(BLD_THREADS) void k_label_tile(int W, int H, int tiles_x, const uint8_t* __restrict__ cells,
                                                            int* __restrict__ parent) {
  constexpr int WAVES = BLD_THREADS / 64;
  static_assert(BLD_TILE_H / WAVES <= 32, "a wave's south bits fill one register");
  __shared__ int s_l[BLD_CELLS];
  __shared__ int s_changed;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = tx * BLD_TILE_W + lane;
  unsigned south = 0;                                                // bit t: this lane's cell of row wv + t WAVES has a south edge
#pragma nounroll
  for (int t = 0; t < BLD_TILE_H / WAVES; ++t) {                     // wave-uniform: every lane takes part in the ballots
    const int r = wv + t * WAVES, i = ty * BLD_TILE_H + r;
    const uint8_t f = i < H && j < W ? cells[(long)i * W + j] : (uint8_t)0;
    const bool node = i < H && j < W && Edges::node(f);
    const unsigned long long nb = __ballot(node);
    const unsigned long long edges = __ballot(node && Edges::east(f)) & (nb >> 1);      // bit k: cells k and k + 1 of this row are joined
    const unsigned long long gaps_below = ~edges & ((1ull << lane) - 1ull);
    const int start = gaps_below ? 64 - __clzll((long long)gaps_below) : 0;      // the cell after the nearest missing edge on the left
    s_l[r * BLD_TILE_W + lane] = node ? r * BLD_TILE_W + start : -1;
    if (!Edges::all_joined && Edges::south(f)) south |= 1u << t;
  }
  __syncthreads();
  for (int pass = 0; pass < BLD_CELLS; ++pass) {                     // fewer passes than cells: see the head of the file
    if (threadIdx.x == 0) s_changed = 0;
    __syncthreads();
#pragma nounroll
    for (int t = 0; t < BLD_TILE_H / WAVES; ++t) {
      const int r = wv + t * WAVES, k = r * BLD_TILE_W + lane;       // the edge from row r to row r + 1
      if (r + 1 < BLD_TILE_H && (Edges::all_joined || ((south >> t) & 1u)) && bld_lds_load(s_l + k) >= 0 &&
          bld_lds_load(s_l + k + BLD_TILE_W) >= 0) {                 // both ends are nodes: the sign of an entry never changes
        const int a = bld_find(s_l, k + BLD_TILE_W), b = bld_find(s_l, k);
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
  for (int r = wv; r < BLD_TILE_H; r += WAVES) {
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

// ---- the border rounds ------------------------------------------------------------------------------------------------------
template <class Edges>
__global__ __launch_bounds__(BLD_THREADS) void k_label_pairs(int W, int H, long n_vertical, long n_pairs, const uint8_t* __restrict__ cells,
                                                             const int* __restrict__ parent, int2* __restrict__ pairs,
                                                             unsigned* __restrict__ changed) {
  const long p = (long)blockIdx.x * BLD_THREADS + threadIdx.x;
  if (p >= n_pairs) return;
  long a, b;
  bld_pair_cells(p, W, H, n_vertical, a, b);
  int2 out = make_int2(-1, -1);
  if (p < n_vertical ? Edges::east(cells[a]) : Edges::south(cells[a])) {      // MaskEdges: always, and the byte is not read
    const int pa = parent[a], pb = parent[b];                        // both >= 0 iff both cells are nodes
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

// dsm_buildings.hip: one round's second and third kernel, and the final walk of every cell to its root
int launch_bld_hook(long n_pairs, long n, const int2* pairs, int* parent, hipStream_t st);
int launch_bld_compress(int W, int H, long n_vertical, long n_pairs, int* parent, hipStream_t st);
int launch_bld_compress_all(long n, int* parent, hipStream_t st);

// device-side stopwatch of a labelling's three groups: four events on the stream, read after the final synchronise
struct BldClock {
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ok = true;
  BldClock() {
    for (auto& e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
  }
  ~BldClock() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  void mark(int k, hipStream_t st) { ok = ok && hipEventRecord(ev[k], st) == hipSuccess; }
  float ms(int k) {
    float t = 0.0f;
    return ok && hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess ? t : -1.0f;
  }
};

// ---- the launcher -----------------------------------------------------------------------------------------------------------
// Workspace: a control block (256 B), then the pairs of a round (at most W H / 32 pairs of 8 bytes).  Errors are reported as
// "<Edges::name>_label: ...".
template <class Edges>
int launch_label(int W, int H, const uint8_t* cells, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st) {
  const auto failed = [](const char* what, hipError_t e) { return set_error((int)e, "%s_%s: %s", Edges::name, what, hipGetErrorString(e)); };
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
  hipLaunchKernelGGL(k_label_tile<Edges>, dim3((unsigned)stats->tiles), dim3(BLD_THREADS), 0, st, W, H, tiles_x, cells, parent);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return failed("tile", e);
  clock.mark(1, st);
  bool open = n_pairs > 0;                               // whether the last look found a pair with two roots
  while (open) {
    unsigned host = 0;
    e = hipMemsetAsync(changed, 0, sizeof(unsigned), st);
    if (e != hipSuccess) return failed("label", e);
    hipLaunchKernelGGL(k_label_pairs<Edges>, dim3(bld_blocks(n_pairs)), dim3(BLD_THREADS), 0, st, W, H, n_vertical, n_pairs, cells,
                       (const int*)parent, pairs, changed);
    e = hipGetLastError();
    if (e != hipSuccess) return failed("pairs", e);
    e = hipMemcpyAsync(&host, changed, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return failed("label", e);
    open = host != 0;
    if (!open || stats->rounds == ADAMVS_BLD_MAX_ROUNDS) break;
    if (int rc = launch_bld_hook(n_pairs, n, pairs, parent, st)) return rc;
    if (int rc = launch_bld_compress(W, H, n_vertical, n_pairs, parent, st)) return rc;
    ++stats->rounds;
  }
  if (open)
    return set_error(ADAMVS_BLD_NOT_CONVERGED, "%s_label: tile borders still open after %d rounds", Edges::name, ADAMVS_BLD_MAX_ROUNDS);
  clock.mark(2, st);
  if (int rc = launch_bld_compress_all(n, parent, st)) return rc;
  clock.mark(3, st);
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return failed("label", e);
  stats->ms_tile = clock.ms(0);
  stats->ms_rounds = clock.ms(1);
  stats->ms_compress = clock.ms(2);
  stats->converged = 1;
  return 0;
}

}  // namespace adamvs
