// Shared by every launcher of a persistent kernel: tile bookkeeping, the resident capacity per device, and the launch
// whose grid is that capacity (or the work, when there is less).
#pragma once
#include <atomic>
#include "common.h"

namespace adamvs {

// Tile bookkeeping of the persistent kernels: tile t -> (tile_x, tile_y, b) with the two divisions done as
// multiply-high by constants prepared on the host (t is workgroup-uniform, so this stays on the scalar unit).
struct TileGrid {
  int tiles_x, tiles_y, ntiles;
  unsigned mx, my;       // ceil(2^32 / tiles_x), ceil(2^32 / tiles_y); unused when the divisor is 1
};
__device__ __forceinline__ void tile_coords(const TileGrid& g, int t, int& b, int& tx, int& ty) {
  unsigned r = g.tiles_x == 1 ? (unsigned)t : __umulhi((unsigned)t, g.mx);
  tx = t - (int)r * g.tiles_x;
  unsigned bb = g.tiles_y == 1 ? r : __umulhi(r, g.my);
  ty = (int)r - (int)bb * g.tiles_y;
  b = (int)bb;
}
static int make_tile_grid(TileGrid& g, int tiles_x, int tiles_y, int B) {
  long n = (long)tiles_x * tiles_y * B;
  // exactness of the multiply-high quotient needs t * divisor < 2^32
  if (n <= 0 || n * (tiles_x > tiles_y ? tiles_x : tiles_y) >= (1L << 32)) return set_error(-1, "too many tiles (%ld)", n);
  g.tiles_x = tiles_x; g.tiles_y = tiles_y; g.ntiles = (int)n;
  g.mx = (unsigned)(((1ull << 32) + tiles_x - 1) / tiles_x);
  g.my = (unsigned)(((1ull << 32) + tiles_y - 1) / tiles_y);
  return 0;
}

// workgroups of `kernel` that stay resident on the current device (raw occupancy query; resident_capacity caches it)
template <typename K>
static int resident_blocks(K kernel, int threads, size_t lds) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, lds) != hipSuccess || n < 1) n = 1;
  int cus = 256, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 256;
  return n * cus;
}

// *capacity = resident workgroups of Kernel (256 threads, `lds` bytes) on the current device.  Both the count and the
// dynamic-LDS limit above 64 KB are per-device facts (one process may drive several devices, e.g. nn.DataParallel with
// one thread per device), so the first call per (Kernel, device) raises the limit when it must, then caches the count.
// A kernel is launched with the same `lds` everywhere (a constant of its instantiation).  Later calls are one atomic load;
// two threads racing on a first call both query and set the attribute, both idempotent.  No stream operation: safe
// while a stream is being captured.  Devices past the cache are queried on every call.
template <auto Kernel>
static int resident_capacity(size_t lds, const char* name, int* capacity) {
  static std::atomic<int> cache[16];                 // per device; 0 = not yet known
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const bool cached = dev >= 0 && dev < 16;
  if (cached && (*capacity = cache[dev].load(std::memory_order_acquire))) return 0;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return set_error((int)e, "%s: hipFuncSetAttribute: %s", name, hipGetErrorString(e));
  }
  *capacity = resident_blocks(Kernel, 256, lds);
  if (cached) cache[dev].store(*capacity, std::memory_order_release);
  return 0;
}

// Launch the persistent Kernel with min(work_items, resident capacity) workgroups of 256 threads and `lds` bytes of
// dynamic LDS; args are every kernel argument.  Errors read "name: ...".
template <auto Kernel, typename... Args>
static int launch_resident(long work_items, size_t lds, hipStream_t st, const char* name, const Args&... args) {
  int capacity;
  if (int rc = resident_capacity<Kernel>(lds, name, &capacity)) return rc;
  hipLaunchKernelGGL(Kernel, dim3((unsigned)(work_items < capacity ? work_items : capacity)), dim3(256), lds, st, args...);
  ADAMVS_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace adamvs
