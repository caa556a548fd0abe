// The pieces every fp32 MFMA kernel of the CostRegNet2D family (costreg2d.hip) is made of: a block's window of ONE CHUNK of input
// channels, the A-fragment fetch, the double-buffered trip of the chunk loop and the epilogue of a lane's pixel.
//
// The window is LR x WCOLS pixels of a channel-last map [N][hi * wi][D], laid out in LDS with row pitch LC (>= WCOLS: the pair forms
// load 65 columns into rows of 68, 33 into 34).  It is moved as (pixel, channel group of 4) items, one per thread and load
// instruction (the surplus lanes of the last instruction repeat the last item: the same value to the same place).  An item outside
// the map takes the offset BUF_OOB, which reads zeros: the zero padding of the convolution, the same rule at every site.
//
//   init(hi, wi, D, iy0, ix0)      the per-lane constants of the block whose window starts at pixel (iy0, ix0), pinned
//   request(stage, rsrc, ch)       issue the loads of chunk `ch` (first input channel) into `stage`; nothing is waited for
//   request(sa, ra, sb, rb, ch, two)   the same for in + in2 on shared offsets: in's loads, then (two) in2's
//   store(stage, lds)              put them into LDS as fp32 channel planes [NG groups][GP], group = four planes of pitch PLANE
//   store(stage, stage2, two, lds) the same with the two sources summed on the way (`two`: a template flag or a uniform one)
//
// A sibling of TileWindow (tile_window.h), not a use of it, because the kernels differ where TileWindow spends its code:
//  * they are not persistent: a block has one window position, so it computes its offsets ONCE with the bounds already folded in
//    (goff[] is BUF_OOB outside the map) and there is no interior / edge split and no per-tile bounds test;
//  * the channel CHUNK enters as the scalar offset operand of the buffer load: the descriptor and the per-lane offsets are the
//    same for every chunk of the layer;
//  * a chunk holds only NG = KB / 4 channel groups of a D-channel source (TileWindow moves all C channels of a narrow map).
//
// Out of scope: costreg2d_bf16x3.hip (plain loads, a bf16 hi / lo LDS layout of its own) and costreg2d_wino.hip /
// costreg2d_wino24.hip (persistent, offsets per tile, a transformed layout).
//
// The two class-chained loops keep their own text and use the window, the fragment fetch and bias_act:
//  * conv_dd_t2_all (request the next class's first chunk in the last trip; the first wait of a later class is the compiler's).
//    On the trip helper, with a tail hook in the else of the last request's branch and a flag for the first wait, it built and
//    added no branch, but k_conv_dd<4, 4, CONV_T2, 4> came out at 236 AGPRs for 228 (170 VGPRs, one wave per SIMD either way);
//  * conv_dd_t2_pairs: peeled at both ends of a class so that every request inside the loop is unconditional; 256 registers.
// Their buffer-store epilogues are a deliberately different rule (EVERY lane issues every store, so that the number in flight
// is known) and share only bias_act.
#pragma once
#include "common.h"

namespace adamvs {

template <int LR, int WCOLS, int LC, int NG, int PLANE, int GP, int NTHR = 256>
struct ChunkWindow {
  static constexpr int NITEMS = LR * WCOLS * NG;
  static constexpr int N = (NITEMS + NTHR - 1) / NTHR;      // load instructions (and stage registers) per chunk
  unsigned goff[N];       // byte offset of the item from the window's first pixel, channel 0 of the chunk; BUF_OOB outside the map
  unsigned lbyte[N];      // LDS byte offset of the item's first channel plane

  // the item that load instruction k gives this thread: channel group, window row and column; own = not a surplus lane's repeat
  struct Item { int g, r, c; bool own; };
  static __device__ __forceinline__ Item item(int k) {
    const int j = (int)threadIdx.x + k * NTHR, i = min(j, NITEMS - 1), pp = i / NG;
    return Item{i % NG, pp / WCOLS, pp % WCOLS, j < NITEMS};
  }

  // descriptor at the window's first pixel (may point one row / column outside the map)
  static __device__ __forceinline__ buf_rsrc origin(const float* src, int n, int hi, int wi, int D, int iy0, int ix0) {
    return make_rsrc((const char*)src + (((long)n * hi + iy0) * wi + ix0) * (long)D * 4);
  }

  __device__ __forceinline__ void init(int hi, int wi, int D, int iy0, int ix0) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const Item t = item(k);
      const bool ok = (unsigned)(iy0 + t.r) < (unsigned)hi && (unsigned)(ix0 + t.c) < (unsigned)wi;
      goff[k] = ok ? (unsigned)(((t.r * wi + t.c) * D + 4 * t.g) * 4) : BUF_OOB;
      lbyte[k] = (unsigned)((t.g * GP + t.r * LC + t.c) * 4);
      pin(goff[k]); pin(lbyte[k]);
    }
  }

  __device__ __forceinline__ void request(f32x4* stage, buf_rsrc rs, int ch) const {
#pragma unroll
    for (int k = 0; k < N; ++k)
      stage[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, goff[k], (unsigned)ch * 4u, 0));
  }
  __device__ __forceinline__ void request(f32x4* sa, buf_rsrc ra, f32x4* sb, buf_rsrc rb, int ch, bool two) const {
    request(sa, ra, ch);
    if (two) request(sb, rb, ch);
  }

  __device__ __forceinline__ void store(const f32x4* stage, const f32x4* stage2, bool two, float* lds) const {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float* dl = (float*)((char*)lds + lbyte[k]);
      const f32x4 v = two ? stage[k] + stage2[k] : stage[k];
      dl[0] = v.x; dl[PLANE] = v.y; dl[2 * PLANE] = v.z; dl[3 * PLANE] = v.w;
    }
  }
  __device__ __forceinline__ void store(const f32x4* stage, float* lds) const { store(stage, stage, false, lds); }
};

// A fragment of (tap, k-step = input channel / 4, tile of 16 output channels) of a layer packed as [9][D / 4][D / 16][64 lanes]
// (KCT = D / 4, NTILES = D / 16); lane_off = lane * 4 bytes, the rest is uniform and goes into the scalar offset operand.
__device__ __forceinline__ float load_afrag(buf_rsrc rw, unsigned lane_off, int tap, int kstep, int tile, int KCT, int NTILES) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, lane_off, (unsigned)((tap * KCT + kstep) * NTILES + tile) * 256u, 0));
}

// The chunk loop: KB input channels per chunk, two chunks per trip (D / KB is even for every supported D), two named register
// sets A | B for the fragments.
//
// fp32 MFMA shares the vector lanes (tools/microbench/mfma_issue.hip: every extra VALU instruction per MFMA costs 3-6 cycles of
// matrix time, at any occupancy), and at these register budgets there are one or two waves per SIMD, so the loop is written to
// contain matrix instructions and nothing else that needs the vector ALU:
//  * global accesses are buffer loads: uniform descriptor, per-lane byte offset computed once (ChunkWindow), the chunk enters as
//    the scalar offset operand;
//  * LDS addresses of the tile fill and of the B-fragment reads are per-lane constants, pinned in registers;
//  * the fragments and the activation tile of chunk k+1 are requested before the MFMAs of chunk k and waited for once, after them
//    (vmcnt retires in order; a single explicit wait keeps the compiler from scheduling its own in the middle of the chain).
//
//   wfA, wfB          the two register sets (the kernel's array of fragments); they stay compile-time indexed
//   request(wf, ch)    fragments of chunk `ch` into the set `wf`, and the chunk's window into the stage registers
//   store()            the staged window into LDS
//   mfma(wf)           the chunk's MFMAs on the set `wf` and the LDS tile
// On entry chunk 0 is requested into set A.
//
// This is ONE TRIP; the kernel writes the loop statement around it,
//     for (int ch = 0; ch < D; ch += 2 * KB) chunk_trip<KB>(D, ch, wfA, wfB, request, store, mfma);
// because with the `for` inside the helper the same instructions come out in another block order (the loop's exit block behind
// the loop instead of ahead of it), and the register allocation of the widest tilings moves with it: k_conv_dd<4, 4, ..> by
// 4 AGPRs either way, k_conv_dd<3, 4, ..> by up to 10 VGPRs.
template <int KB, class WF, class Req, class Store, class Mfma>
__device__ __forceinline__ void chunk_trip(int D, int ch, WF& wfA, WF& wfB, Req&& request, Store&& store, Mfma&& mfma) {
  wait_vmem_all();
  __syncthreads();                    // previous chunk's readers are done
  store();
  __syncthreads();
  request(wfB, ch + KB);
  mfma(wfA);

  wait_vmem_all();
  __syncthreads();
  store();
  __syncthreads();
  if (ch + 2 * KB < D) request(wfA, ch + 2 * KB);
  mfma(wfB);
}

// bias, then the layer's ReLU
__device__ __forceinline__ f32x4 bias_act(f32x4 acc, f32x4 bias4, int relu) {
  f32x4 v = acc + bias4;
  if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  return v;
}

// The plain epilogue of a lane that owns channels 4 q .. 4 q + 3 of the channel tiles tile0 .. tile0 + MT - 1 of ONE output pixel
// (oy, ox) of image n: guard, bias / ReLU, + skip (added after the ReLU), store.  acc(mt): the tile's accumulator.
// a: bias, skip, out, ho, wo, relu.
//
// k_conv_dd_resident keeps its own text of this rule (and repeats it for its GroupNorm partial sums, which form the stored
// values a second time), sharing bias_act: with both passes on this function -- or on any function or lambda of the kernel's
// own -- k_conv_dd_resident<32, 4, true> came out at 176 VGPRs for 166, two waves per SIMD for three.
template <int MT, class Args, class Acc>
__device__ __forceinline__ void epilogue_pixel(const Args& a, int D, int n, int oy, int ox, int tile0, int q, Acc&& acc) {
  if (oy >= a.ho || ox >= a.wo) return;
  const size_t opix = ((size_t)n * a.ho + oy) * a.wo + ox;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int co4 = (tile0 + mt) * 16 + 4 * q;
    f32x4 v = bias_act(acc(mt), *(const f32x4*)(a.bias + co4), a.relu);
    if (a.skip) v += *(const f32x4*)(a.skip + opix * D + co4);
    *(f32x4*)(a.out + opix * D + co4) = v;
  }
}

}  // namespace adamvs
