// What the two tiled component labellings share: the building stage's (dsm_buildings.hip, over a mask) and the roof stage's
// (dsm_roofs.hip, over link bits).  The tile-border pairs and their order, the walk to a root, the stopwatch, and the launchers
// of the three kernels that do not look at the mask at all: k_bld_hook, k_bld_compress and k_bld_compress_all live in
// dsm_buildings.hip once and are launched from both files.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace adamvs
