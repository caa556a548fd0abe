// What the raster stages (dsm_buildings.hip, dsm_roofs.hip, dsm_trees.hip, dsm_contours.hip) share besides the labelling of
// bld_union.h: a cell's row and column, the runs of equal labels within a wave that the per-label tables are reduced over,
// the add that skips zeros, the start values of a table and the binomial pass over an integer raster with holes.  Integer
// work only: the includers switch fp contraction off after their includes, and a helper that multiplies and then adds floats
// would round differently from one includer to the next (block_prims.h).
#pragma once
#include <initializer_list>

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

}  // namespace adamvs
