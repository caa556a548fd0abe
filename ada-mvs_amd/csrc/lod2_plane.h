// The one evaluation of an integer roof plane at a lattice corner (include/adamvs_hip.h "LoD2 solids", step 1): the kernels of
// dsm_lod2.hip and the host entry adamvs_lod2_corner_heights_host (api.hip) both call it, so the device and the host cannot
// round differently.
#pragma once

namespace adamvs {

// pl = {A, B, C} in 2^-20 m (per cell east, per cell south, at the centre of cell (0, 0)); corner (r, c) lies half a cell north
// and west of the centre of cell (r, c).  -> the height in 1/1024 m, rounded half up.  The caller bounds |A|, |B| < 2^40 and
// |C| < 2^50, so with r, c <= 2^15 the sum stays below 2^58.  >> of a negative int64 is an arithmetic shift on the host
// compilers and the device alike: the floor.
__host__ __device__ inline long long lod2_corner_height(const long long* pl, int r, int c) {
  const long long n = pl[0] * (2LL * c - 1) + pl[1] * (2LL * r - 1) + 2LL * pl[2];
  return (n + 1024) >> 11;
}

}  // namespace adamvs
