// One source's window of a tile, as every persistent MFMA convolution stages it (slice_roles.h, "Persistent workgroups").
//
// The window is LR x LC pixels of C channels of a channel-last map [N][hi * wi][C].  It is moved as (pixel, channel group of 4)
// items, 256 per load instruction (one per thread; the surplus lanes of the last instruction repeat the last item: the same value
// to the same place), so that the base of every instruction is workgroup-uniform: the tile enters through a buffer descriptor at
// the window's first pixel, the lane through an offset that does not depend on the tile.  An interior window is loaded without
// bounds checks; on an edge tile an item outside the map takes the offset BUF_OOB, which reads zeros: the zero padding of the
// convolution, the same rule at every site.
//
//   request(stage, src, ...)   issue the loads of a window into `stage` (N registers of four floats); nothing is waited for
//   store(stage, lds)          put them into LDS as fp32 channel planes [C / 4 groups][GP], group = four planes of pitch PLANE
//
// A kernel with two sources composes two windows (A's loads, then B's; B's groups behind A's in LDS: store<GA>).  Two sources of
// the same geometry may share one window: either call by call, or with the two-source request, which interleaves their loads.
// A kernel with a layout of its own (the bf16x3 roles) passes it to init and keeps its store.
#pragma once
#include "common.h"

namespace adamvs {

// KEEP_RC: the window coordinates of the items stay in registers (one per item) for the edge tiles; without, they are formed
// again from the thread index there: a few integer divisions on a path few tiles take, for N registers in every tile.
// PLANE, GP: the planar LDS layout of init(wi) and store (0: a layout of the kernel's own).
template <int C, int LR, int LC, bool KEEP_RC = true, int PLANE = 0, int GP = 0>
struct TileWindow {
  static_assert(C % 4 == 0, "channel groups of four");
  static constexpr int G = C / 4, GD = G ? G : 1, NPIX = LR * LC;
  static constexpr int N = (NPIX * G + 255) / 256;        // load instructions (and stage registers) per window; 0 when C == 0
  static constexpr int NR = N ? N : 1;
  unsigned goff[NR];      // byte offset of the item from the window's first pixel in its source
  unsigned lbyte[NR];     // LDS byte offset of the item (planar layout: of its first channel plane, in group 0)
  int rc[KEEP_RC ? NR : 1];   // window row | column << 16 (edge tiles only)

  // window pixel of the item that load instruction k gives this thread
  static __device__ __forceinline__ int pixel(int k) { return min((int)threadIdx.x + k * 256, NPIX * G - 1) / GD; }

  // wi: row length of the source in pixels; lds_byte(row, column, group): where the item of that window pixel goes in LDS
  template <typename Layout>
  __device__ __forceinline__ void init(int wi, Layout lds_byte) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const int j = min((int)threadIdx.x + k * 256, NPIX * G - 1);
      const int g = j % GD, pp = j / GD, r = pp / LC, c = pp % LC;
      goff[k] = (unsigned)(((r * wi + c) * C + 4 * g) * 4);
      lbyte[k] = (unsigned)lds_byte(r, c, g);
      pin(goff[k]); pin(lbyte[k]);
      if (KEEP_RC) { rc[k] = r | (c << 16); pin(rc[k]); }
    }
  }
  __device__ __forceinline__ void init(int wi) {
    static_assert(GP > 0, "the planar layout");
    init(wi, [](int r, int c, int g) { return (g * GP + r * LC + c) * 4; });
  }

  // The pieces of request, for a kernel that puts windows of different geometry under one joint interior test.
  static __device__ __forceinline__ buf_rsrc origin(const float* src, int n, int hi, int wi, int iy0, int ix0) {
    return make_rsrc((const char*)src + (((long)n * hi + iy0) * wi + ix0) * (C * 4));     // may point one row / column outside
  }
  static __device__ __forceinline__ bool interior(int hi, int wi, int iy0, int ix0) {
    return iy0 >= 0 && ix0 >= 0 && iy0 + LR <= hi && ix0 + LC <= wi;
  }
  // offset of item k on an edge tile
  __device__ __forceinline__ unsigned edge_off(int k, int hi, int wi, int iy0, int ix0) const {
    const int iy = iy0 + (KEEP_RC ? rc[KEEP_RC ? k : 0] & 0xffff : pixel(k) / LC);
    const int ix = ix0 + (KEEP_RC ? rc[KEEP_RC ? k : 0] >> 16 : pixel(k) % LC);
    return ((unsigned)iy < (unsigned)hi && (unsigned)ix < (unsigned)wi) ? goff[k] : BUF_OOB;      // zero padding
  }
  template <bool EDGE>
  __device__ __forceinline__ void load(f32x4* stage, buf_rsrc rs, int hi, int wi, int iy0, int ix0) const {
#pragma unroll
    for (int k = 0; k < N; ++k) stage[k] = buf_load4(rs, EDGE ? edge_off(k, hi, wi, iy0, ix0) : goff[k]);
  }

  // the window whose first pixel is (iy0, ix0) of sample n of src [..][hi * wi][C]
  __device__ __forceinline__ void request(f32x4* stage, const float* src, int n, int hi, int wi, int iy0, int ix0) const {
    const buf_rsrc rs = origin(src, n, hi, wi, iy0, ix0);
    if (interior(hi, wi, iy0, ix0)) load<false>(stage, rs, hi, wi, iy0, ix0);
    else load<true>(stage, rs, hi, wi, iy0, ix0);
  }
  // the same window of two sources of one geometry, on one set of offsets, their loads interleaved
  __device__ __forceinline__ void request(f32x4* sa, const float* srcA, f32x4* sb, const float* srcB, int n, int hi, int wi, int iy0,
                                          int ix0) const {
    const buf_rsrc ra = origin(srcA, n, hi, wi, iy0, ix0), rb = origin(srcB, n, hi, wi, iy0, ix0);
    if (interior(hi, wi, iy0, ix0)) {
#pragma unroll
      for (int k = 0; k < N; ++k) { sa[k] = buf_load4(ra, goff[k]); sb[k] = buf_load4(rb, goff[k]); }
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const unsigned o = edge_off(k, hi, wi, iy0, ix0);
        sa[k] = buf_load4(ra, o); sb[k] = buf_load4(rb, o);
      }
    }
  }

  // fp32 channel planes; G0: the window's first group in a tile [groups][GP] that several windows fill
  template <int G0 = 0>
  __device__ __forceinline__ void store(const f32x4* stage, float* lds) const {
    static_assert(PLANE > 0 && GP > 0, "the planar layout");
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float* dl = (float*)((char*)lds + lbyte[k]) + G0 * GP;
      const f32x4 v = stage[k];
      dl[0] = v.x; dl[PLANE] = v.y; dl[2 * PLANE] = v.z; dl[3 * PLANE] = v.w;
    }
  }
};

}  // namespace adamvs
