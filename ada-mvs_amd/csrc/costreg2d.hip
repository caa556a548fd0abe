// CostRegNet2D: the depth-as-channel 2D hourglass that scores each source view
// in stage 1 (reference models/adamvs.py:198-238, blocks models/module.py:254-261),
// and the per-pixel softmax / max / expectation that turns its scores into a view
// weight and a pair depth (reference models/adamvs.py:481-486, module.py:617-625).
//
// Every layer is a D->D 3x3 convolution: an implicit GEMM with K = 9*D on the fp32
// matrix cores (v_mfma_f32_16x16x4_f32, exact fp32).  Activations are channel-last
// [N][h*w][D]; rows of the MFMA tile are output channels, columns are 16
// consecutive output pixels of one row, so a lane ends up with 4 consecutive
// channels of one pixel (one 16-byte store).  Weights are pre-packed on the host in
// A-fragment order with the eval-mode BatchNorm scale folded in and stream
// straight from L2 into VGPRs (each wave owns different output channels, so
// there is nothing to share through LDS); activations go through a planar LDS
// tile shared by the block's four waves.
#include <stdlib.h>
#include <type_traits>

#include "chunk_window.h"
#include "common.h"
#include "conv_frag.h"
#include "costreg_softmax.h"
#include "kernels.h"
#include "persistent.h"

namespace adamvs {

struct ConvDDArgs {
  const float* in;     // [N][hi*wi][D]
  const float* wpk;    // [9][D/4][D/16][64]
  const float* bias;   // [D]
  const float* skip;   // [N][ho*wo][D] or null; added after the ReLU (adamvs.py:234-236)
  float* out;          // [N][ho*wo][D]
  int D, hi, wi, ho, wo, relu;
  // softmax epilogue (the `prob` layer inside a stage, reference adamvs.py:481-486): when sm_vw != null the scores are not
  // stored; the block reduces them over D and writes view_weight = max_d softmax and pair_depth = sum_d softmax * depth_d
  float* sm_vw; float* sm_pd;   // [N][ho*wo]
  PlaneSrc sm_planes;           // image n belongs to tile n % sm_B
  int sm_B;
  const float* in2;    // [N][hi*wi][D] or null: the layer convolves in + in2, summed when the window enters LDS.  The
                       // hourglass's skip additions (x = conv4 + conv7(x), adamvs.py:234-236) run HERE, in the consumer of x:
                       // in the producer's epilogue a skip operand is a second round of loads that nothing overlaps
  // k_conv_dd_resident only (MS-REDNet's deep GRU levels): GroupNorm(1 group) partial sums of the output's channels [0, gn_n)
  // in the epilogue -- wave w of workgroup (x, y) writes (sum, sum of squares) in double to
  // gn_part[((n * gn_ngroups + gn_group) * parts + (y * gridDim.x + x) * 4 + w) * 2], parts = 4 * workgroups per map
  double* gn_part;
  int gn_n, gn_group, gn_ngroups;
  int sm_D;            // softmax epilogue: the number of hypothesis planes when the network runs wider (costreg_width); 0 = D
};

enum { CONV_S1 = 0, CONV_S2 = 1, CONV_T2 = 2 };

// window of a block of BR output rows x 16 output columns (CONV_T2: input positions)
template <int MODE, int BR = 8> struct TileGeom;
template <int BR> struct TileGeom<CONV_S1, BR> { static constexpr int LR = BR + 2, LC = 18, PLANE = plane_pitch16((BR + 2) * 18); };
template <int BR> struct TileGeom<CONV_S2, BR> { static constexpr int LR = 2 * BR + 1, LC = 33, PLANE = ((2 * BR + 1) * 33) | 1; };
template <int BR> struct TileGeom<CONV_T2, BR> { static constexpr int LR = BR + 1, LC = 17, PLANE = plane_pitch16((BR + 1) * 17); };

// KB = input channels per LDS chunk (template parameter: 8 = two MFMA k-steps, 4 = one)

// Block = 8 rows x 16 columns of output positions x all D output channels.
// Waves: WM along output channels (MT tiles of 16 each), WN = 4/WM along rows.
// PY/PX: output parity class, CONV_T2 only (ConvTranspose2d k3 s2 p1 op1).
// Window, fragment fetch, chunk loop (and why it holds one explicit wait per chunk) and epilogue: chunk_window.h.
template <int MT, int WM, int MODE, int KB, int PY, int PX, int BR = 8, bool TWO = false, bool SOFTMAX = false>
__device__ __forceinline__ void conv_dd_body(const ConvDDArgs& a, float* lds, int n, int by, int bx) {
  using TG = TileGeom<MODE, BR>;
  constexpr int LR = TG::LR, LC = TG::LC, PLANE = TG::PLANE, GP = group_pitch(PLANE, KB / 4);
  constexpr int WN = 4 / WM, NTR = BR / WN;
  static_assert(NTR >= 1, "rows per wave");
  constexpr int STR = (MODE == CONV_S2) ? 2 : 1;
  constexpr int NTY = (MODE == CONV_T2) ? 1 + PY : 3;
  constexpr int NTX = (MODE == CONV_T2) ? 1 + PX : 3;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int wm = wave % WM, wn = wave / WM;
  const int p = lane & 15, q = lane >> 4;
  const int D = a.D, KCT = D / 4, NTILES = D / 16;
  const int r0 = by * BR, c0 = bx * 16;                      // block origin (output rows/cols, or input i/j for T2)
  const int iy0 = (MODE == CONV_T2) ? r0 : r0 * STR - 1;
  const int ix0 = (MODE == CONV_T2) ? c0 : c0 * STR - 1;
  constexpr int NTAP = NTY * NTX;
  using Win = ChunkWindow<LR, LC, LC, KB / 4, PLANE, GP>;
  constexpr int NITA = Win::N;

  // ---- per-lane constants
  // activation tile: item = (pixel of the window, group of 4 channels); out-of-image pixels read as zero
  const buf_rsrc rx = Win::origin(a.in, n, a.hi, a.wi, D, iy0, ix0);
  Win win;
  win.init(a.hi, a.wi, D, iy0, ix0);
  // A fragments: [tap][D/4][D/16][64]; lane offset only, the rest is uniform
  const buf_rsrc rw = make_rsrc(a.wpk);
  unsigned woff = (unsigned)(lane * 4);
  pin(woff);
  // B fragments: lane's k-row and pixel, per k-chunk of the LDS tile
  unsigned xb[KB / 4];
#pragma unroll
  for (int kc = 0; kc < KB / 4; ++kc) {
    xb[kc] = (unsigned)((kc * GP + q * PLANE + (wn * NTR * STR) * LC + p * STR) * 4);
    pin(xb[kc]);
  }

  f32x4 acc[MT][NTR];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < NTR; ++r) acc[mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_w = [&](float (&wf)[NTAP][KB / 4][MT], int ch) {
#pragma unroll
    for (int ty = 0; ty < NTY; ++ty)
#pragma unroll
      for (int tx = 0; tx < NTX; ++tx) {
        const int ky = (MODE == CONV_T2) ? (PY ? (ty ? 0 : 2) : 1) : ty;
        const int kx = (MODE == CONV_T2) ? (PX ? (tx ? 0 : 2) : 1) : tx;
#pragma unroll
        for (int kc = 0; kc < KB / 4; ++kc)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            wf[ty * NTX + tx][kc][mt] = load_afrag(rw, woff, ky * 3 + kx, ch / 4 + kc, wm * MT + mt, KCT, NTILES);
          }
      }
  };
  constexpr bool two = TWO;          // the layer convolves in + in2 (a separate instantiation: the plain chunk loop stays as it was)
  const buf_rsrc rx2 = Win::origin(two ? a.in2 : a.in, n, a.hi, a.wi, D, iy0, ix0);
  auto mfma_chunk = [&](const float (&wf)[NTAP][KB / 4][MT]) {
#pragma unroll
    for (int ty = 0; ty < NTY; ++ty)
#pragma unroll
      for (int tx = 0; tx < NTX; ++tx)
#pragma unroll
        for (int kc = 0; kc < KB / 4; ++kc) {
          float bv[NTR];
#pragma unroll
          for (int r = 0; r < NTR; ++r) bv[r] = *(const float*)((const char*)lds + xb[kc] + ((r * STR + ty) * LC + tx) * 4);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < NTR; ++r) acc[mt][r] = mfma16(wf[ty * NTX + tx][kc][mt], bv[r], acc[mt][r]);
        }
  };

  float wfA[NTAP][KB / 4][MT], wfB[NTAP][KB / 4][MT];
  f32x4 xs[NITA], xs2[NITA];
  auto request = [&](auto& wf, int ch) { load_w(wf, ch); win.request(xs, rx, xs2, rx2, ch, two); };
  request(wfA, 0);
  auto store_x = [&] { win.store(xs, xs2, two, lds); };
  for (int ch = 0; ch < D; ch += 2 * KB) chunk_trip<KB>(D, ch, wfA, wfB, request, store_x, mfma_chunk);

  if (SOFTMAX) {
    __syncthreads();                                   // the last chunk's readers are done: the tile space is reused
    softmax_epilogue<MT, WM, NTR, BR>(acc, a.bias, a.sm_planes, a.sm_B, n, r0, c0, a.ho, a.wo, a.sm_D ? a.sm_D : D, a.sm_vw, a.sm_pd, lds);
    return;
  }
  // epilogue: lane owns channels co4..co4+3 of the pixel in column p
#pragma unroll
  for (int r = 0; r < NTR; ++r) {
    const int row = r0 + wn * NTR + r, col = c0 + p;
    epilogue_pixel<MT>(a, D, n, (MODE == CONV_T2) ? 2 * row + PY : row, (MODE == CONV_T2) ? 2 * col + PX : col, wm * MT, q,
                       [&](int mt) { return acc[mt][r]; });
  }
}

// ConvTranspose2d(k3, s2, p1, op1), all four output parity classes of one 8 x 16 block of input positions in one
// workgroup, one after the other.  A class on its own is a short block (1, 2, 2 or 4 taps against the 9 of a
// stride-1 block) whose prologue -- per-lane constants, the latency of the first fragment and window loads -- and
// epilogue weigh as much as a third of it; here the constants are shared and the first chunk of the next class is
// requested during the last chunk of the current one, so its loads and the current class's epilogue overlap.
template <int MT, int WM, int KB>
__device__ __forceinline__ void conv_dd_t2_all(const ConvDDArgs& a, float* lds, int n, int by, int bx) {
  using TG = TileGeom<CONV_T2>;
  constexpr int LR = TG::LR, LC = TG::LC, PLANE = TG::PLANE, GP = group_pitch(PLANE, KB / 4);
  constexpr int WN = 4 / WM, NTR = 8 / WN;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int wm = wave % WM, wn = wave / WM;
  const int p = lane & 15, q = lane >> 4;
  const int D = a.D, KCT = D / 4, NTILES = D / 16;
  const int r0 = by * 8, c0 = bx * 16;                       // block origin: input positions (i, j)
  using Win = ChunkWindow<LR, LC, LC, KB / 4, PLANE, GP>;
  constexpr int NITA = Win::N;

  const buf_rsrc rx = Win::origin(a.in, n, a.hi, a.wi, D, r0, c0);
  const bool two = a.in2 != nullptr;                         // uniform: the layer convolves in + in2
  const buf_rsrc rx2 = Win::origin(two ? a.in2 : a.in, n, a.hi, a.wi, D, r0, c0);
  Win win;
  win.init(a.hi, a.wi, D, r0, c0);
  const buf_rsrc rw = make_rsrc(a.wpk);
  unsigned woff = (unsigned)(lane * 4);
  pin(woff);
  unsigned xb[KB / 4];
#pragma unroll
  for (int kc = 0; kc < KB / 4; ++kc) {
    xb[kc] = (unsigned)((kc * GP + q * PLANE + (wn * NTR) * LC + p) * 4);
    pin(xb[kc]);
  }
  // epilogue: the lane's output pixel of class (0, 0) in row r of its wave, as a byte offset from the image (the class and
  // the channel tile are added as uniform terms); BUF_OOB outside the map, so that EVERY lane issues every store and
  // the number of stores in flight after an epilogue is known: the next class does not wait for them
  const buf_rsrc ro = make_rsrc((char*)a.out + (long)n * a.ho * a.wo * (long)D * 4);
  const buf_rsrc rk = make_rsrc((const char*)(a.skip ? a.skip : a.out) + (long)n * a.ho * a.wo * (long)D * 4);
  unsigned ooff[NTR];
#pragma unroll
  for (int r = 0; r < NTR; ++r) {
    const int row = r0 + wn * NTR + r, col = c0 + p;
    ooff[r] = (row < a.hi && col < a.wi) ? (unsigned)((((2 * row) * a.wo + 2 * col) * D + wm * MT * 16 + 4 * q) * 4) : BUF_OOB;
    pin(ooff[r]);
  }

  float wfA[4][KB / 4][MT], wfB[4][KB / 4][MT];              // up to 4 taps
  f32x4 xs[NITA], xs2[NITA];
  f32x4 acc[MT][NTR];

  auto load_x = [&](int ch) { win.request(xs, rx, xs2, rx2, ch, two); };
  auto store_x = [&] { win.store(xs, xs2, two, lds); };
  auto load_w = [&](auto pyc, auto pxc, float (&wf)[4][KB / 4][MT], int ch) {
    constexpr int PY = decltype(pyc)::value, PX = decltype(pxc)::value;
#pragma unroll
    for (int ty = 0; ty <= PY; ++ty)
#pragma unroll
      for (int tx = 0; tx <= PX; ++tx) {
        const int ky = PY ? (ty ? 0 : 2) : 1, kx = PX ? (tx ? 0 : 2) : 1;
#pragma unroll
        for (int kc = 0; kc < KB / 4; ++kc)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            wf[ty * (1 + PX) + tx][kc][mt] = load_afrag(rw, woff, ky * 3 + kx, ch / 4 + kc, wm * MT + mt, KCT, NTILES);
          }
      }
  };
  auto mfma_chunk = [&](auto pyc, auto pxc, const float (&wf)[4][KB / 4][MT]) {
    constexpr int PY = decltype(pyc)::value, PX = decltype(pxc)::value;
#pragma unroll
    for (int ty = 0; ty <= PY; ++ty)
#pragma unroll
      for (int tx = 0; tx <= PX; ++tx)
#pragma unroll
        for (int kc = 0; kc < KB / 4; ++kc) {
          float bv[NTR];
#pragma unroll
          for (int r = 0; r < NTR; ++r) bv[r] = *(const float*)((const char*)lds + xb[kc] + ((r + ty) * LC + tx) * 4);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < NTR; ++r) acc[mt][r] = mfma16(wf[ty * (1 + PX) + tx][kc][mt], bv[r], acc[mt][r]);
        }
  };
  // one class; wfA and xs hold its first chunk on entry; on exit they hold the first chunk of class (nyc, nxc), if any.
  // `first`: nothing but that first chunk is in flight (block entry); otherwise the previous class's stores are, and the
  // wait for the chunk -- requested BEFORE them, vmcnt retires in order -- is left to the compiler, which counts them.
  auto run_class = [&](auto pyc, auto pxc, auto nyc, auto nxc, auto has_next, auto first) {
    constexpr int PY = decltype(pyc)::value, PX = decltype(pxc)::value;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < NTR; ++r) acc[mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < D; ch += 2 * KB) {            // chunk_trip (chunk_window.h) with the two class-chaining rules
      if (decltype(first)::value || ch > 0) wait_vmem_all();
      __syncthreads();
      store_x();
      __syncthreads();
      load_w(pyc, pxc, wfB, ch + KB);
      load_x(ch + KB);
      mfma_chunk(pyc, pxc, wfA);

      wait_vmem_all();
      __syncthreads();
      store_x();
      __syncthreads();
      if (ch + 2 * KB < D) {
        load_w(pyc, pxc, wfA, ch + 2 * KB);
        load_x(ch + 2 * KB);
      } else if (decltype(has_next)::value) {
        load_w(nyc, nxc, wfA, 0);
        load_x(0);
      }
      mfma_chunk(pyc, pxc, wfB);
    }
    const unsigned cls = (unsigned)((PY * a.wo + PX) * D * 4);           // uniform: the class's pixel offset
#pragma unroll
    for (int r = 0; r < NTR; ++r)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 v = bias_act(acc[mt][r], *(const f32x4*)(a.bias + (wm * MT + mt) * 16 + 4 * q), a.relu);
        const unsigned o = ooff[r] == BUF_OOB ? BUF_OOB : ooff[r] + cls + (unsigned)(mt * 64);
        if (a.skip) v += buf_load4(rk, o);
        buf_store4(ro, o, v);
      }
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  load_w(I1{}, I1{}, wfA, 0);
  load_x(0);
  run_class(I1{}, I1{}, I1{}, I0{}, std::true_type{}, std::true_type{});
  run_class(I1{}, I0{}, I0{}, I1{}, std::true_type{}, std::false_type{});
  run_class(I0{}, I1{}, I0{}, I0{}, std::true_type{}, std::false_type{});
  run_class(I0{}, I0{}, I0{}, I0{}, std::false_type{}, std::false_type{});
}

// ConvTranspose2d(k3, s2, p1, op1) with the four output parity classes of a block of input positions advanced TOGETHER,
// chunk by chunk of input channels.  conv_dd_t2_all above runs the classes one after the other: each loads the whole
// input window again and spends a barrier pair per channel chunk on 1, 2, 2 or 4 taps (24 ... 96 MFMAs per wave), which is
// why the transposed layers sat at 40-71 % of the matrix rate.  Here a chunk is loaded once and feeds all nine
// (input offset, class) pairs -- exactly the nine taps of the 3 x 3 kernel, each used once:
//     offset (0,0): class 00 tap (1,1) | 01 (1,2) | 10 (2,1) | 11 (2,2);  offset (0,1): 01 (1,0) | 11 (2,0);
//     offset (1,0): 10 (0,1) | 11 (0,2);  offset (1,1): 11 (0,0)          (class = output parity (py, px))
// The price is four accumulator sets: at two waves per SIMD they leave room for BR = 2 rows x 16 columns of input
// positions per block (4 x 32 outputs; 4 rows need one wave per SIMD and were 40 % slower, 8 rows spill), i.e. 54 MFMAs
// per wave and barrier pair -- the average of the class-by-class kernel, but uniformly, with the window loaded once and
// four times the workgroups: it wins on SMALL grids (the deep levels of the hourglass, few tiles per launch) and is
// chosen there (launch_conv_dd_cfg).
template <int MT, int WM, int KB, int BR>
__device__ __forceinline__ void conv_dd_t2_fused(const ConvDDArgs& a, float* lds, int n, int by, int bx) {
  constexpr int LR = BR + 1, LC = 17, PLANE = plane_pitch16(LR * LC), GP = group_pitch(PLANE, KB / 4);
  constexpr int WN = 4 / WM, NTR = BR / WN;
  static_assert(NTR >= 1, "rows per wave");
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform
  const int wm = wave % WM, wn = wave / WM;
  const int p = lane & 15, q = lane >> 4;
  const int D = a.D, KCT = D / 4, NTILES = D / 16;
  const int r0 = by * BR, c0 = bx * 16;                      // block origin: input positions (i, j)
  using Win = ChunkWindow<LR, LC, LC, KB / 4, PLANE, GP>;
  constexpr int NITA = Win::N;

  const buf_rsrc rx = Win::origin(a.in, n, a.hi, a.wi, D, r0, c0);
  Win win;
  win.init(a.hi, a.wi, D, r0, c0);
  const buf_rsrc rw = make_rsrc(a.wpk);
  unsigned woff = (unsigned)(lane * 4);
  pin(woff);
  unsigned xb[KB / 4];
#pragma unroll
  for (int kc = 0; kc < KB / 4; ++kc) {
    xb[kc] = (unsigned)((kc * GP + q * PLANE + (wn * NTR) * LC + p) * 4);
    pin(xb[kc]);
  }

  f32x4 acc[4][MT][NTR];                                     // [class = 2 py + px]
#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < NTR; ++r) acc[c][mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_w = [&](float (&wf)[9][KB / 4][MT], int ch) {    // all nine taps of the chunk, tap = ky * 3 + kx
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int kc = 0; kc < KB / 4; ++kc)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          wf[t][kc][mt] = load_afrag(rw, woff, t, ch / 4 + kc, wm * MT + mt, KCT, NTILES);
        }
  };
  const bool two = a.in2 != nullptr;                         // uniform: the layer convolves in + in2
  const buf_rsrc rx2 = Win::origin(two ? a.in2 : a.in, n, a.hi, a.wi, D, r0, c0);
  auto mfma_chunk = [&](const float (&wf)[9][KB / 4][MT]) {
#pragma unroll
    for (int ty = 0; ty < 2; ++ty)
#pragma unroll
      for (int tx = 0; tx < 2; ++tx)
#pragma unroll
        for (int kc = 0; kc < KB / 4; ++kc) {
          float bv[NTR];
#pragma unroll
          for (int r = 0; r < NTR; ++r) bv[r] = *(const float*)((const char*)lds + xb[kc] + ((r + ty) * LC + tx) * 4);
#pragma unroll
          for (int py = ty; py < 2; ++py)                    // classes that reach input offset (ty, tx)
#pragma unroll
            for (int px = tx; px < 2; ++px) {
              const int ky = py ? (ty ? 0 : 2) : 1, kx = px ? (tx ? 0 : 2) : 1;
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < NTR; ++r)
                  acc[2 * py + px][mt][r] = mfma16(wf[ky * 3 + kx][kc][mt], bv[r], acc[2 * py + px][mt][r]);
            }
        }
  };

  float wfA[9][KB / 4][MT], wfB[9][KB / 4][MT];
  f32x4 xs[NITA], xs2[NITA];
  auto request = [&](auto& wf, int ch) { load_w(wf, ch); win.request(xs, rx, xs2, rx2, ch, two); };
  request(wfA, 0);
  auto store_x = [&] { win.store(xs, xs2, two, lds); };
  for (int ch = 0; ch < D; ch += 2 * KB) chunk_trip<KB>(D, ch, wfA, wfB, request, store_x, mfma_chunk);

#pragma unroll
  for (int c = 0; c < 4; ++c)
#pragma unroll
    for (int r = 0; r < NTR; ++r)
      epilogue_pixel<MT>(a, D, n, 2 * (r0 + wn * NTR + r) + (c >> 1), 2 * (c0 + p) + (c & 1), wm * MT, q,
                         [&](int mt) { return acc[c][mt][r]; });
}

// Stride-2 layer (conv1, conv3, conv5 of the hourglass: reference models/adamvs.py:206-211, 229-232) with the minimal-filtering
// form of its polyphase decomposition along x: two neighbouring outputs of a row share the input column between them,
//     out[2m]     = W0 c[4m]   + W1 c[4m+1] + W2 c[4m+2]
//     out[2m + 1] = W0 c[4m+2] + W1 c[4m+3] + W2 c[4m+4]            (c = the window row, W = the three taps of one kernel row)
// and the two-tap filter (W0, W2) over the even columns costs three products per two outputs instead of four:
//     A0 = W1 c[4m+1] + W0 (c[4m] - c[4m+2]);  A1 = W1 c[4m+3] + W2 (c[4m+4] - c[4m+2]);  A2 = (W0 + W2) c[4m+2]
//     out[2m] = A0 + A2,  out[2m + 1] = A1 + A2
// -- five MFMAs per (kernel row, 4 input channels, channel tile, output row) for 32 output pixels where the direct form issues six
// (15 / 18 of the layer's products; the same along y would give 25 / 36 but needs nine accumulator sets).  The columns of an MFMA are
// 16 output PAIRS; a lane reads its five window values as one 16-byte and one 4-byte LDS read (row pitch 68: aligned), forms the
// two differences (2 vector instructions per 15 MFMAs) and W0 + W2 once per chunk from the fragments it streams anyway (9 adds):
// the blob keeps its nine taps.  Block = 3 output rows x 32 columns x all channels: three accumulator sets of 3 x 3 tiles = 108
// registers, two waves per SIMD as in conv_dd_body; one k-step per chunk, chunks double-buffered the same way.
//
// FOLD = F: the 16 columns of an MFMA are 16 / F output pairs of each of F row groups -- lane p holds pair
// p % (16 / F) of the output rows (p / (16 / F)) 3 + r -- so a block is 3 F output rows x 32 / F columns with the same accumulators,
// fragments and MFMAs, and per output the same sums in the same order: conv3's 24 x 48 outputs are blocks of 6 x 16 (F = 2), conv5's
// 12 x 24 blocks of 12 x 8 (F = 4), where the 32-column block pads a row by a third and the layer stayed on the direct kernel.
// The window's row pitch and plane pitch put the 16 lanes of every ds_read_b128 group on 16 different bank quadruples (row groups
// 6 LC floats apart: LC = 48 gives 8 quadruples (mod 16) for F = 2, LC = 24 gives 4 for F = 4; planes a multiple of 64 floats).
constexpr int S2P_ROWS = 3;      // output rows per block (4: 144 accumulator registers next to 63 of fragments: spills; the hourglass's 48 / 24 / 12 rows divide by 3)
template <int FOLD>
struct S2PGeom {
  static_assert(FOLD == 1 || FOLD == 2 || FOLD == 4, "16 / FOLD pairs of FOLD row groups");
  static constexpr int BR = S2P_ROWS, PPR = 16 / FOLD, BC = 2 * PPR;              // pairs per row, output columns per block
  static constexpr int LR = 2 * BR * FOLD + 1, WCOLS = 2 * BC + 1, LC = FOLD == 1 ? 68 : (FOLD == 2 ? 48 : 24);
  static constexpr int PLANE = FOLD == 1 ? ((LR * LC + 31) / 32) * 32 + 16 : ((LR * LC + 63) / 64) * 64;
  static_assert(LC >= WCOLS && LC % 4 == 0 && PLANE >= LR * LC, "16-byte reads at column 4 p of a row");
};
template <int MT, int WM, int FOLD = 1>
__device__ __forceinline__ void conv_dd_s2_pairs(const ConvDDArgs& a, float* lds, int n, int by, int bx) {
  static_assert(WM == 4, "every wave takes all rows of the block");
  using G = S2PGeom<FOLD>;
  constexpr int BR = G::BR, LR = G::LR, WCOLS = G::WCOLS, LC = G::LC, PLANE = G::PLANE;
  using Win = ChunkWindow<LR, WCOLS, LC, 1, PLANE, 4 * PLANE>;     // one channel group per chunk
  constexpr int NITA = Win::N;
  const int tid = threadIdx.x, lane = tid & 63, wm = __builtin_amdgcn_readfirstlane(tid >> 6);    // wave = channel slice
  const int p = lane & 15, q = lane >> 4;
  const int D = a.D, KCT = D / 4, NTILES = D / 16;
  const int fr = FOLD == 1 ? 0 : p / G::PPR, fp = FOLD == 1 ? p : p % G::PPR;   // the lane's row group and pair of the row
  const int r0 = by * BR * FOLD, c0 = bx * G::BC;
  const int iy0 = 2 * r0 - 1, ix0 = 2 * c0 - 1;

  const buf_rsrc rx = Win::origin(a.in, n, a.hi, a.wi, D, iy0, ix0);
  Win win;
  win.init(a.hi, a.wi, D, iy0, ix0);
  const buf_rsrc rw = make_rsrc(a.wpk);
  unsigned woff = (unsigned)(lane * 4);
  pin(woff);
  unsigned xb = (unsigned)((q * PLANE + 2 * BR * fr * LC + 4 * fp) * 4);   // the lane's k-row, first window row of its row group and first column of its pair
  pin(xb);

  f32x4 acc[3][MT][BR];                                        // A0 | A1 | A2
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < BR; ++r) acc[t][mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto load_w = [&](float (&wf)[9][MT], int ch) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        wf[t][mt] = load_afrag(rw, woff, t, ch / 4, wm * MT + mt, KCT, NTILES);
      }
  };
  auto mfma_chunk = [&](const float (&wf)[9][MT]) {
    float w02[3][MT];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) w02[ky][mt] = wf[ky * 3 + 0][mt] + wf[ky * 3 + 2][mt];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int r = 0; r < BR; ++r) {
        const char* row = (const char*)lds + xb + ((2 * r + ky) * LC) * 4;
        const f32x4 c = *(const f32x4*)row;
        const float c4 = *(const float*)(row + 16);
        const float d0 = c.x - c.z, d1 = c4 - c.z;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acc[0][mt][r] = mfma16(wf[ky * 3 + 1][mt], c.y, acc[0][mt][r]);
          acc[0][mt][r] = mfma16(wf[ky * 3 + 0][mt], d0, acc[0][mt][r]);
          acc[1][mt][r] = mfma16(wf[ky * 3 + 1][mt], c.w, acc[1][mt][r]);
          acc[1][mt][r] = mfma16(wf[ky * 3 + 2][mt], d1, acc[1][mt][r]);
          acc[2][mt][r] = mfma16(w02[ky][mt], c.z, acc[2][mt][r]);
        }
      }
  };

  float wfA[9][MT], wfB[9][MT];
  f32x4 xs[NITA];
  auto request = [&](auto& wf, int ch) { load_w(wf, ch); win.request(xs, rx, ch); };
  request(wfA, 0);
  auto store_x = [&] { win.store(xs, lds); };
  for (int ch = 0; ch < D; ch += 8) chunk_trip<4>(D, ch, wfA, wfB, request, store_x, mfma_chunk);      // one k-step per chunk
  // epilogue: lane owns channels co4 .. co4 + 3 of the output pair (c0 + 2 p, c0 + 2 p + 1) of every row
#pragma unroll
  for (int r = 0; r < BR; ++r) {
    const int oy = r0 + fr * BR + r, ox = c0 + 2 * fp;
    if (oy >= a.ho || ox >= a.wo) continue;
    const size_t opix = ((size_t)n * a.ho + oy) * a.wo + ox;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int co4 = (wm * MT + mt) * 16 + 4 * q;
      const f32x4 b = *(const f32x4*)(a.bias + co4);
      const f32x4 v0 = bias_act(acc[0][mt][r] + acc[2][mt][r], b, a.relu), v1 = bias_act(acc[1][mt][r] + acc[2][mt][r], b, a.relu);
      *(f32x4*)(a.out + opix * D + co4) = v0;
      if (ox + 1 < a.wo) *(f32x4*)(a.out + (opix + 1) * D + co4) = v1;
    }
  }
}

// grid: (ceil(wo / (32 / FOLD)), ceil(ho / (S2P_ROWS FOLD)), N); block 256
template <int MT, int WM, int FOLD = 1>
__global__ __launch_bounds__(256, 2) void k_conv_dd_s2p(ConvDDArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[4 * S2PGeom<FOLD>::PLANE];
  conv_dd_s2_pairs<MT, WM, FOLD>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
}

// Transposed layer (conv7, conv9, conv11 of the hourglass) with the same minimal-filtering form along x.  The odd output columns of a
// row are a two-tap filter over neighbouring inputs (tap names as in conv_dd_t2_all: kx = 2 meets in[j], kx = 0 meets in[j + 1]),
//     out[2j + 1] = W2 in[j] + W0 in[j + 1],          out[2j + 3] = W2 in[j + 1] + W0 in[j + 2]
// and two neighbouring ones share in[j + 1]:
//     A1 = W2 (in[j] - in[j + 1]);  A2 = (W0 + W2) in[j + 1];  A3 = W0 (in[j + 2] - in[j + 1]);  out[2j + 1] = A1 + A2,  out[2j + 3] = A3 + A2
// -- three products per two odd outputs instead of four; the even columns (out[2j] = W1 in[j]) stay direct.  Five MFMAs per (kernel
// row, 4 input channels, channel tile, input row) for an input PAIR = four output pixels where the class-by-class kernel issues six:
// 15 / 18 of the layer's products.  The columns of an MFMA are 16 input pairs; a lane reads in[2p .. 2p + 2] as one 8-byte and one
// 4-byte LDS read (row pitch 34: aligned), forms the two differences (2 vector instructions per 5 MT MFMAs) and W0 + W2 once per chunk.
// Five accumulator sets per input row; block = NR input rows x 32 input columns (2 NR x 64 outputs) x all channels, every wave all rows of
// its 48 channels.  The two row classes run one after the other as in conv_dd_t2_all, the next one's first chunk requested during the
// last chunk of the current one: py = 1 (odd output rows: kernel rows 2 and 0 on input rows i, i + 1) with KB1 input channels per chunk,
// py = 0 (kernel row 1 on row i: half the MFMAs per channel) with KB0.  What differs at the ends of a class is peeled out of its chunk
// loop (requests inside it are unconditional).  Built as NR = 2, KB1 = KB0 = 8: 120 accumulator registers, 120 / 60 MFMAs per wave and
// barrier pair, 256 registers with one dword of scratch outside the chunk loops.  KB0 = 16 (120 MFMAs in both classes) spills 13
// registers, some inside the loops; NR = 3 (180 accumulator registers) spills 170 - 340 (docs/history/tried_without_gain.md).
constexpr int T2P_COLS = 32;     // input columns per block
typedef float f32x2 __attribute__((ext_vector_type(2)));
__host__ __device__ constexpr int plane_pitch32(int n) { return ((n + 31) / 64) * 64 + 32; }   // >= n, 32 mod 64: the two k-rows of a 32-lane ds_read_b64 group on disjoint banks
template <int NR> struct T2PGeom {
  static constexpr int WCOLS = T2P_COLS + 1, LC = T2P_COLS + 2, PLANE = plane_pitch32((NR + 1) * LC);
  static constexpr int lds_floats(int KB) { return (KB / 4) * group_pitch(PLANE, KB / 4); }
};
template <int MT, int NR, int KB1, int KB0>
__device__ __forceinline__ void conv_dd_t2_pairs(const ConvDDArgs& a, float* lds, int n, int by, int bx) {
  using G = T2PGeom<NR>;
  constexpr int WCOLS = G::WCOLS, LC = G::LC, PLANE = G::PLANE;
  constexpr bool SAME = KB0 == KB1;                            // one window for both classes: py = 0 loads (and ignores) the row below its own
  using Win1 = ChunkWindow<NR + 1, WCOLS, LC, KB1 / 4, PLANE, group_pitch(PLANE, KB1 / 4)>;
  using Win0 = ChunkWindow<NR, WCOLS, LC, KB0 / 4, PLANE, group_pitch(PLANE, KB0 / 4)>;
  constexpr int NI0 = SAME ? Win1::N : Win0::N, NIM = Win1::N > NI0 ? Win1::N : NI0;
  constexpr int NW = (6 * (KB1 / 4) > 3 * (KB0 / 4) ? 6 * (KB1 / 4) : 3 * (KB0 / 4)) * MT;
  static_assert(192 % (2 * KB1) == 0 && 192 % (2 * KB0) == 0, "an even number of chunks per class at D = 192, 384");
  const int tid = threadIdx.x, lane = tid & 63, wm = __builtin_amdgcn_readfirstlane(tid >> 6);    // wave = channel slice
  const int p = lane & 15, q = lane >> 4;
  const int D = a.D, KCT = D / 4, NTILES = D / 16;
  const int r0 = by * NR, c0 = bx * T2P_COLS;                  // block origin: input positions (i, j)

  const buf_rsrc rx = Win1::origin(a.in, n, a.hi, a.wi, D, r0, c0);
  const bool two = a.in2 != nullptr;                           // uniform: the layer convolves in + in2
  const buf_rsrc rx2 = Win1::origin(two ? a.in2 : a.in, n, a.hi, a.wi, D, r0, c0);
  // window fill, per class: item = (pixel of the window, group of 4 channels); pixels outside the map read as zero
  Win1 win1;
  Win0 win0;
  win1.init(a.hi, a.wi, D, r0, c0);
  if (!SAME) win0.init(a.hi, a.wi, D, r0, c0);
  auto window = [&](auto pyc) -> const auto& {
    if constexpr (decltype(pyc)::value || SAME) return win1; else return win0;
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using K0 = std::integral_constant<int, KB0>;
  using K1 = std::integral_constant<int, KB1>;
  const buf_rsrc rw = make_rsrc(a.wpk);
  unsigned woff = (unsigned)(lane * 4);
  pin(woff);
  unsigned xb = (unsigned)((q * PLANE + 2 * p) * 4);           // the lane's k-row and the first window column of its pair
  pin(xb);
  // epilogue: the lane's four output pixels (columns 4 p' .. 4 p' + 3 of the block's 64) of class py = 0 in input row r, as a byte offset
  // from the image; BUF_OOB outside the map (the width is even: a pair is inside or outside as a whole), so that EVERY lane issues every store
  const buf_rsrc ro = make_rsrc((char*)a.out + (long)n * a.ho * a.wo * (long)D * 4);
  const buf_rsrc rk = make_rsrc((const char*)(a.skip ? a.skip : a.out) + (long)n * a.ho * a.wo * (long)D * 4);
  unsigned ooff[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const int row = r0 + r, col = c0 + 2 * p;
    ooff[r] = (row < a.hi && col < a.wi) ? (unsigned)((((2 * row) * a.wo + 2 * col) * D + wm * MT * 16 + 4 * q) * 4) : BUF_OOB;
    pin(ooff[r]);
  }

  float wfA[NW], wfB[NW];                                      // [kernel row of the class][kx][k-step][channel tile]
  f32x4 xs[NIM], xs2[NIM];
  f32x4 acc[5][MT][NR];                                        // even outputs E0 | E1, then A1 | A2 | A3

  auto load_x = [&](auto pyc, auto kbc, int ch) { window(pyc).request(xs, rx, xs2, rx2, ch, two); };
  auto store_x = [&](auto pyc) { window(pyc).store(xs, xs2, two, lds); };
  auto load_w = [&](auto pyc, auto kbc, float (&wf)[NW], int ch) {
    constexpr int PY = decltype(pyc)::value, NG = decltype(kbc)::value / 4;
#pragma unroll
    for (int ty = 0; ty <= PY; ++ty)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ky = PY ? (ty ? 0 : 2) : 1;
#pragma unroll
        for (int kc = 0; kc < NG; ++kc)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            wf[((ty * 3 + kx) * NG + kc) * MT + mt] = load_afrag(rw, woff, ky * 3 + kx, ch / 4 + kc, wm * MT + mt, KCT, NTILES);
          }
      }
  };
  auto mfma_chunk = [&](auto pyc, auto kbc, const float (&wf)[NW]) {
    constexpr int PY = decltype(pyc)::value, NG = decltype(kbc)::value / 4, GP = group_pitch(PLANE, NG);
#pragma unroll
    for (int ty = 0; ty <= PY; ++ty)
#pragma unroll
      for (int kc = 0; kc < NG; ++kc) {
        float w02[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) w02[mt] = wf[((ty * 3 + 0) * NG + kc) * MT + mt] + wf[((ty * 3 + 2) * NG + kc) * MT + mt];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const char* row = (const char*)lds + xb + (kc * GP + (r + ty) * LC) * 4;
          const f32x2 c = *(const f32x2*)row;
          const float c2 = *(const float*)(row + 8);
          const float d0 = c.x - c.y, d1 = c2 - c.y;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[0][mt][r] = mfma16(wf[((ty * 3 + 1) * NG + kc) * MT + mt], c.x, acc[0][mt][r]);
            acc[1][mt][r] = mfma16(wf[((ty * 3 + 1) * NG + kc) * MT + mt], c.y, acc[1][mt][r]);
            acc[2][mt][r] = mfma16(wf[((ty * 3 + 2) * NG + kc) * MT + mt], d0, acc[2][mt][r]);
            acc[3][mt][r] = mfma16(w02[mt], c.y, acc[3][mt][r]);
            acc[4][mt][r] = mfma16(wf[((ty * 3 + 0) * NG + kc) * MT + mt], d1, acc[4][mt][r]);
          }
        }
      }
  };
  // one chunk of a class: `cur` holds its fragments and xs its window; `req` issues the requests that follow it
  auto half = [&](auto pyc, auto kbc, const float (&cur)[NW], auto explicit_wait, auto&& req) {
    if (decltype(explicit_wait)::value) wait_vmem_all();
    __syncthreads();                    // previous chunk's readers are done
    store_x(pyc);
    __syncthreads();
    req();
    mfma_chunk(pyc, kbc, cur);
  };
  // one class; wfA and xs hold its first chunk on entry; on exit they hold the first chunk of the next class, if any.
  // `first`: nothing but that first chunk is in flight (block entry); otherwise the previous class's stores are, and the
  // wait for the chunk -- requested BEFORE them, vmcnt retires in order -- is left to the compiler, which counts them.
  auto run_class = [&](auto pyc, auto kbc, auto first, auto&& req_next) {
    constexpr int PY = decltype(pyc)::value, KB = decltype(kbc)::value;
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[t][mt][r] = f32x4{0.f, 0.f, 0.f, 0.f};
    half(pyc, kbc, wfA, first, [&] { load_w(pyc, kbc, wfB, KB); load_x(pyc, kbc, KB); });
    for (int ch = KB; ch < D - KB; ch += 2 * KB) {
      half(pyc, kbc, wfB, std::true_type{}, [&] { load_w(pyc, kbc, wfA, ch + KB); load_x(pyc, kbc, ch + KB); });
      half(pyc, kbc, wfA, std::true_type{}, [&] { load_w(pyc, kbc, wfB, ch + 2 * KB); load_x(pyc, kbc, ch + 2 * KB); });
    }
    half(pyc, kbc, wfB, std::true_type{}, req_next);
#pragma unroll
    for (int t = 0; t < 5; ++t)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < NR; ++r) drain(acc[t][mt][r]);
    const unsigned cls = (unsigned)(PY * a.wo * D * 4);                    // uniform: the class's row offset
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 b = *(const f32x4*)(a.bias + (wm * MT + mt) * 16 + 4 * q);
#pragma unroll
      for (int r = 0; r < NR; ++r) {
        const f32x4 sum[4] = {acc[0][mt][r], acc[2][mt][r] + acc[3][mt][r], acc[1][mt][r], acc[4][mt][r] + acc[3][mt][r]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          f32x4 v = bias_act(sum[k], b, a.relu);
          // BUF_OOB plus these terms (< 2^31) is still out of range.  The sum is a lane offset, not the scalar offset operand: a 16-byte
          // store with a scalar offset gets no wait state before the next write of its data registers, and the last store of the
          // class lost its fourth channel in lanes 12 - 15 to the next class's window sum
          const unsigned o = ooff[r] + (cls + (unsigned)(mt * 64) + (unsigned)(k * D * 4));
          if (a.skip) v += buf_load4(rk, o);
          buf_store4(ro, o, v);
        }
      }
    }
  };
  load_w(I1{}, K1{}, wfA, 0);
  load_x(I1{}, K1{}, 0);
  run_class(I1{}, K1{}, std::true_type{}, [&] { load_w(I0{}, K0{}, wfA, 0); load_x(I0{}, K0{}, 0); });
  run_class(I0{}, K0{}, std::false_type{}, [] {});
}

// grid: (ceil(wi/32), ceil(hi/NR), N); block 256
template <int MT, int NR, int KB1, int KB0>
__global__ __launch_bounds__(256, 2) void k_conv_dd_t2p(ConvDDArgs a) {
  constexpr int F1 = T2PGeom<NR>::lds_floats(KB1), F0 = T2PGeom<NR>::lds_floats(KB0);
  __shared__ __attribute__((aligned(16))) float lds[F1 > F0 ? F1 : F0];
  conv_dd_t2_pairs<MT, NR, KB1, KB0>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
}

// option s2_pairs = 0: the stride-2 and the transposed layers on the direct kernels, as in rounds 1-4 (A/B)
static bool s2_pairs() { return opt(OPT_S2_PAIRS) != 0; }

// grid: (ceil(cols/16), ceil(rows/BR), N); block 256; OCC = waves per SIMD the register budget is held to
template <int MT, int WM, int KB, int BR, int OCC>
__global__ __launch_bounds__(256, OCC) void k_conv_dd_t2_fused(ConvDDArgs a) {
  __shared__ float lds[(KB / 4) * group_pitch(plane_pitch16((BR + 1) * 17), KB / 4)];
  conv_dd_t2_fused<MT, WM, KB, BR>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
}

// grid: (ceil(cols/16), ceil(rows/8), N); block 256
// TWO (stride-1 layers only): the layer convolves in + in2; the transposed kernel takes in2 as a uniform run-time switch
// SM (stride-1 layers only): the softmax epilogue of the `prob` layer (conv_dd_body)
constexpr int imax(int a, int b) { return a > b ? a : b; }
template <int MT, int WM, int MODE, int KB, bool TWO = false, bool SM = false>
__global__ __launch_bounds__(256, (MT == 4 && WM == 4) ? 1 : 2) void k_conv_dd(ConvDDArgs a) {
  __shared__ float lds[imax((KB / 4) * group_pitch(TileGeom<MODE>::PLANE, KB / 4), SM ? 8 * 16 * 4 * WM * 3 : 0)];
  if (MODE == CONV_T2) {
    conv_dd_t2_all<MT, WM, KB>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
  } else {
    conv_dd_body<MT, WM, MODE, KB, 0, 0, 8, TWO, SM>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
  }
}

// Stride-1 / stride-2 layers on a SMALL grid (the deep levels of the hourglass when few maps are in flight: 12 x 24 maps
// of 16 tiles are 64 blocks of 8 x 16 on 256 CUs, a third of each block padding): blocks of 2 output rows, four times the
// workgroups, no padded rows.  54 MFMAs per wave and barrier pair instead of 216 -- it pays only while the chip is not full.
template <int MT, int WM, int MODE, int KB, bool TWO = false>
__global__ __launch_bounds__(256, 2) void k_conv_dd_rows2(ConvDDArgs a) {
  __shared__ float lds[(KB / 4) * group_pitch(TileGeom<MODE, 2>::PLANE, KB / 4)];
  conv_dd_body<MT, WM, MODE, KB, 0, 0, 2, TWO>(a, lds, blockIdx.z, blockIdx.y, blockIdx.x);
}

// Measured (cfg3, 4 / 32 tiles per step): 64 blocks of 8 rows 0.185 -> 0.073 ms, 144: 0.193 -> 0.139, 576: 0.49 -> 0.38, 512: 0.33 -> 0.25,
// 1152: 0.80 -> 0.72; at 4608 blocks it is a wash and beyond it loses (10.9 -> 11.2 ms).  Option conv_rows2 = 0 / 1 forces.
static bool small_grid_rows2(long blocks8) {
  const int forced = opt(OPT_CONV_ROWS2);
  if (forced >= 0) return forced != 0;
  return blocks8 <= 2048;
}

// Two waves per SIMD (a single wave feeding the matrix pipe from LDS reaches ~83 % of it, two reach ~92 %:
// tools/microbench/mfma_issue.hip), i.e. at most 256 registers: the widest tilings take one k-step per chunk
// (D = 256 does not fit even so and keeps one wave).
// Which transposed kernel: measured (tools/r02_t2_ab.sh), the fused form wins while the class-by-class grid is small --
// 64 ... 2048 blocks: 0.246 -> 0.080 ms, 0.267 -> 0.169, 0.646 -> 0.509, 1.57 -> 1.31 -- and loses on the large layers
// (4608 blocks: 3.61 -> 3.92 ms; 18432: 14.1 -> 15.4), where the 4-tap class alone already gives the class-by-class
// kernel 96 MFMAs per barrier pair.  Option t2_fused = 0 / 1 forces one of them (A/B timing).
static bool t2_fused(long blocks_class_by_class) {
  const int forced = opt(OPT_T2_FUSED);
  if (forced >= 0) return forced != 0;
  return blocks_class_by_class <= 2048;
}

// option t2_kb8 = 0: one k-step per chunk in the transposed kernel at D = 192, as in rounds 1-2 (A/B).  Two k-steps halve
// the barrier pairs per class (a class has at most four taps, so the fragments still fit two waves per SIMD):
// measured conv11 of cfg2 14.2 -> 13.8 ms, with the epilogue freed of the skip operand 14.5 -> 12.3.
static bool t2_kb8() { return opt(OPT_T2_KB8) != 0; }
// option costreg_defer_skips = 0: the skip additions in the producing layer's epilogue, as in rounds 1-2 (A/B)
static bool costreg_deferred_skips() { return opt(OPT_COSTREG_DEFER_SKIPS) != 0; }

static bool conv256_split() { return opt(OPT_CONV256_SPLIT) != 0; }

// Which kernel a transposed layer takes: 0 = class by class (k_conv_dd<CONV_T2>), 1 = the four classes per chunk (k_conv_dd_t2_fused,
// small grids), 2 = the pair form along x (k_conv_dd_t2p; option s2_pairs = 0: never).  The pair form exists for the 192-channel tiling
// (D = 192, and 384 as two launches; D = 256 = 2 x 128 channels stays on the direct kernel) and pads a row to blocks of 32 input columns
// where the direct kernel pads to 16: it is taken for even widths of at least one block whose padded products are fewer than the direct
// form's, 5 * 32 * ceil(wi / 32) < 6 * 16 * ceil(wi / 16) -- cfg2 / cfg3: conv11 (96 columns) yes; conv9 (48: a block and a half, 10 > 9)
// and conv7 (24: less than a block) no; cfg5: conv11 (192) and conv9 (96).  Odd widths would split a pair at the border.
constexpr int T2P_NR = 2, T2P_KB1 = 8, T2P_KB0 = 8;      // input rows per block; input channels per chunk of the odd- / even-row class
static bool t2_pairs_pay(int wi) { return wi % 2 == 0 && wi >= T2P_COLS && 5 * 2 * cdiv(wi, T2P_COLS) < 6 * cdiv(wi, 16); }
// Which blocks the stride-2 pair form takes for ho x wo outputs: 1 = 3 rows x 32 columns (where a row divides into them, or from 256
// columns), 2 / 4 = the folded blocks of 6 x 16 / 12 x 8 where the 32-column block does not fit and these tile the map exactly
// (blocks = -1, what every caller but the A/B entry points passes; 2 / 4: that fold wherever the width is a multiple of its block's,
// any height; 0: the selection of before, no folded blocks), 0 = none: the direct kernel.
static int s2_pairs_fold(int ho, int wo, int blocks) {
  if (!s2_pairs()) return 0;
  if (blocks == -1 && (opt(OPT_WINOGRAD) & 4)) blocks = 0;   // option winograd + 4: no folded blocks in any layer (A/B of the whole pipeline)
  if ((blocks == 2 || blocks == 4) && wo % (32 / blocks) == 0) return blocks;
  if (wo % 32 == 0 || wo >= 256) return 1;
  if (blocks != -1) return 0;
  if (wo % 16 == 0 && ho % (2 * S2P_ROWS) == 0) return 2;
  if (wo % 8 == 0 && ho % (4 * S2P_ROWS) == 0) return 4;
  return 0;
}
static int t2_form(int MT, int WM, int N, int hi, int wi) {
  if (WM >= 2 && t2_fused((long)cdiv(wi, 16) * cdiv(hi, 8) * N)) return 1;
  if (MT == 3 && WM == 4 && s2_pairs() && t2_pairs_pay(wi)) return 2;
  return 0;
}
// The tiling of a layer of width D: MT channel tiles per wave x WM waves along the channels = `chunk` output channels per launch,
// `parts` launches over output-channel slices.  Read by conv_t2_form (adamvs_conv_t2_form: which kernel a transposed layer takes)
// and by launch_conv_dd_z, so that the two agree.
struct WidthTiling { int D, MT, WM, parts, chunk; };
static const WidthTiling kWidthTilings[] = {
    {16, 1, 1, 1, 16}, {32, 2, 1, 1, 32}, {48, 3, 1, 1, 48}, {64, 4, 1, 1, 64}, {96, 3, 2, 1, 96}, {128, 4, 2, 1, 128}, {192, 3, 4, 1, 192},
    // 16 output tiles per block need 256 accumulator registers: one wave per SIMD, which feeds the matrix pipe at 83 % (DESIGN
    // section 4, lesson 2; measured 74.5 % of the fp32 MFMA peak for the whole network at cfg5 against 88.5 % at D = 192).  The
    // 128-channel tiling (two waves per SIMD) run twice instead: the second launch sees the weights, bias, skip and output
    // moved by 8 channel tiles and contracts over all 256 input channels like the first.  Measured at cfg5 (8 tiles): 291.9 ->
    // 279.5 ms per step.
    {256, 4, 2, 2, 128},
    // the 192-channel tiling twice (as 256 = 2 x 128 above): each launch contracts over all 384 input channels into its half
    // of the output channels
    {384, 3, 4, 2, 192},
    // the 128-channel tiling four times (round 5; the class default of the reference is num_depth = 384, adamvs.py:538, and
    // ndepths[0] is unconstrained): each launch contracts over all 512 input channels into its quarter of the output channels
    {512, 4, 2, 4, 128},
};
// D = 256 in one launch: the softmax epilogue needs all the channels of a pixel in one workgroup and keeps the wide tiling;
// ADAMVS_CONV256_SPLIT=0: the wide tiling everywhere
static const WidthTiling kWide256 = {256, 4, 4, 1, 256};
static const WidthTiling* width_tiling(int D, bool softmax_epilogue) {
  if (D == 256 && (softmax_epilogue || !conv256_split())) return &kWide256;
  for (const WidthTiling& t : kWidthTilings)
    if (t.D == D) return &t;
  return nullptr;
}
// Which kernel a stride-2 layer without skip or second input takes (adamvs_conv_s2_form): 0 a direct kernel (8-row blocks, or 2-row
// blocks on a small grid), 1 / 2 / 4 the pair form on blocks of 3 x 32, 6 x 16, 12 x 8 outputs (s2_pairs_fold)
static int conv_s2_form(int N, int D, int hi, int wi, int blocks) {
  const WidthTiling* t = width_tiling(D, false);
  if (!t) return -1;
  const int ho = hi / 2, wo = wi / 2;
  if (t->WM >= 2 && small_grid_rows2((long)cdiv(wo, 16) * cdiv(ho, 8) * N)) return 0;
  return t->MT == 3 && t->WM == 4 ? s2_pairs_fold(ho, wo, blocks) : 0;
}
static int conv_t2_form(int N, int D, int hi, int wi) {
  const WidthTiling* t = width_tiling(D, false);
  return t ? t2_form(t->MT, t->WM, N, hi, wi) : -1;
}

template <int MT, int WM>
static int launch_conv_dd_cfg(const ConvDDArgs& a_, int N, int mode, hipStream_t st, int s2_blocks) {
  const ConvDDArgs& a = a_;
  constexpr int KB = (WM == 4 || (MT == 4 && WM == 2)) ? 4 : 8;
  const bool rows2 = WM >= 2 && mode != CONV_T2 && small_grid_rows2((long)cdiv(a.wo, 16) * cdiv(a.ho, 8) * N);
  if (a.sm_vw) {                // the caller has checked cost_reg_softmax_fusable(): stride 1, no second input
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_S1, KB, false, true>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 8), N), dim3(256), 0, st, a);
    ADAMVS_CHECK_LAUNCH("conv_dd (softmax epilogue)");
    return 0;
  }
  if (mode == CONV_S1 && rows2 && a.in2)
    hipLaunchKernelGGL((k_conv_dd_rows2<MT, (WM >= 2 ? WM : 2), CONV_S1, KB, true>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 2), N), dim3(256), 0, st, a);
  else if (mode == CONV_S1 && a.in2)
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_S1, KB, true>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 8), N), dim3(256), 0, st, a);
  else if (mode == CONV_S1 && rows2)
    hipLaunchKernelGGL((k_conv_dd_rows2<MT, (WM >= 2 ? WM : 2), CONV_S1, KB>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 2), N), dim3(256), 0, st, a);
  else if (mode == CONV_S2 && rows2)
    hipLaunchKernelGGL((k_conv_dd_rows2<MT, (WM >= 2 ? WM : 2), CONV_S2, KB>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 2), N), dim3(256), 0, st, a);
  else if (mode == CONV_S1)
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_S1, KB>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 8), N), dim3(256), 0, st, a);
  // D = 192 (and 384 as two launches): 15 / 18 of the products.  Blocks are 32 output columns wide: taken where a row divides into
  // them (cfg2 at 128 tiles: conv1, 48 x 96 outputs, 11.47 -> 10.10 ms; conv3, 24 x 48 -- a block and a half per row -- 2.88 -> 3.31)
  else if (mode == CONV_S2 && MT == 3 && WM == 4 && !a.skip && !a.in2 && s2_pairs_fold(a.ho, a.wo, s2_blocks) == 1)
    hipLaunchKernelGGL((k_conv_dd_s2p<MT, (WM == 4 ? 4 : 4)>), dim3(cdiv(a.wo, 32), cdiv(a.ho, S2P_ROWS), N), dim3(256), 0, st, a);
  // ... and on the folded blocks where those tile the map and the 32-column block does not (cfg2: conv3 on 6 x 16, conv5 on 12 x 8)
  else if (mode == CONV_S2 && MT == 3 && WM == 4 && !a.skip && !a.in2 && s2_pairs_fold(a.ho, a.wo, s2_blocks) == 2)
    hipLaunchKernelGGL((k_conv_dd_s2p<MT, (WM == 4 ? 4 : 4), 2>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 2 * S2P_ROWS), N), dim3(256), 0, st, a);
  else if (mode == CONV_S2 && MT == 3 && WM == 4 && !a.skip && !a.in2 && s2_pairs_fold(a.ho, a.wo, s2_blocks) == 4)
    hipLaunchKernelGGL((k_conv_dd_s2p<MT, (WM == 4 ? 4 : 4), 4>), dim3(cdiv(a.wo, 8), cdiv(a.ho, 4 * S2P_ROWS), N), dim3(256), 0, st, a);
  else if (mode == CONV_S2)
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_S2, KB>), dim3(cdiv(a.wo, 16), cdiv(a.ho, 8), N), dim3(256), 0, st, a);
  else if (WM >= 2 && t2_form(MT, WM, N, a.hi, a.wi) == 1)      // small grids: 2-row blocks, all classes per chunk
    hipLaunchKernelGGL((k_conv_dd_t2_fused<MT, (WM >= 2 ? WM : 2), 4, 2, 2>), dim3(cdiv(a.wi, 16), cdiv(a.hi, 2), N), dim3(256), 0, st, a);
  else if (MT == 3 && WM == 4 && t2_form(MT, WM, N, a.hi, a.wi) == 2)           // 15 / 18 of the products
    hipLaunchKernelGGL((k_conv_dd_t2p<(MT == 3 ? 3 : 3), T2P_NR, T2P_KB1, T2P_KB0>), dim3(cdiv(a.wi, T2P_COLS), cdiv(a.hi, T2P_NR), N), dim3(256), 0, st, a);
  else if (WM == 4 && MT == 3 && t2_kb8())     // at most four taps per class: two k-steps per chunk fit the register budget
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_T2, 8>), dim3(cdiv(a.wi, 16), cdiv(a.hi, 8), N), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((k_conv_dd<MT, WM, CONV_T2, KB>), dim3(cdiv(a.wi, 16), cdiv(a.hi, 8), N), dim3(256), 0, st, a);
  ADAMVS_CHECK_LAUNCH("conv_dd");
  return 0;
}

bool costreg_depth_supported(int D) {
  return D == 16 || D == 32 || D == 48 || D == 64 || D == 96 || D == 128 || D == 192 || D == 256 || D == 384 || D == 512;
}

// The width CostRegNet2D runs at for D hypotheses: the next supported one.  The reference builds the network for any D
// (models/adamvs.py:198-228); here the extra channels are zero weights (packing.py::pack_reg pads to this width: a pad
// channel's activations are ReLU(0) = 0 in every layer and feed nothing), the pair-similarity volume carries zeros in them,
// and the pad channels of `prob` get a bias of -1e30: exp(-1e30 - max) = 0 exactly, so softmax, its maximum and the depth
// expectation see D hypotheses.  0 = more than 512.
int costreg_width(int D) {
  static const int widths[] = {16, 32, 48, 64, 96, 128, 192, 256, 384, 512};
  for (int w : widths)
    if (D <= w) return w;
  return 0;
}
int costreg_width_bf16x3(int D) {
  static const int widths[] = {32, 64, 96, 128, 192, 256, 384, 512};
  for (int w : widths)
    if (D <= w) return w;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Stride-1 layer on a SMALL grid (the deep GRU levels of MS-REDNet: 64 channels on 12x24 ... 48x96 maps, one
// convolution at a time in a recurrence).  An 8 x 16 output tile of k_conv_dd at D = 64 is 9.4 MFLOP = 37k cycles
// of fp32 MFMA on one CU (measured 27 us per launch whatever the map size) while a 12 x 24 map has three such tiles:
// 250 CUs idle.  Here a workgroup takes TR = 1..8 output rows x 16 columns, TR chosen at launch so that the grid
// covers the chip, and everything is requested once: each wave owns one tile of 16 output channels and keeps all its
// A fragments in registers (9 * D/4 <= 144 VGPRs), the (TR+2) x 18 window of all D input channels goes to LDS in one
// round of loads, and what follows is MFMAs fed from LDS.  Same fragment layout, planar LDS layout and epilogue as
// k_conv_dd.  D = 32: two waves per channel tile (NTR rows each, TR = 2 NTR); D = 64: one (TR = NTR).
// What the elementwise kernels between the convolutions of a ConvGRUCell2 did (reference models/module.py:72-106), folded
// into the window fill of the convolution that FOLLOWS them (MS-REDNet's deep levels at one or a few tiles are bound by the
// number of dependent launches per plane: four -> two).  Every workgroup finishes the GroupNorm reductions it needs from the
// partial sums the producing convolutions' epilogues wrote, then forms its input window on the fly:
//   GRU_PRO_GATES (the candidate convolution):  in = sigmoid(GN_r(f)) * h                       f = gate_conv's reset half
//   GRU_PRO_OUT   (the NEXT plane's gate convolutions):  in = h' = u * h + (1 - u) * tanh(GN_o(o)),   u = sigmoid(GN_u(f)),
//                 f = the previous plane's update half, o = its output_conv; the workgroup also stores h' of its own pixels
//                 (the new state, a second buffer: neighbours still read the old one) and its channels [0, hc) into R
// (halo pixels are recomputed by the neighbours: the same operands in the same order, the same bits).
// mean and 1 / sqrt(biased variance + eps) from `parts` partial sums (doubles), by the whole block, deterministic
template <int NTHR>
__device__ __forceinline__ void gru_pro_stats(const double* __restrict__ p, int parts, int count, float eps, double (*wsum)[2], float* st) {
  const int tid = threadIdx.x;
  double s_ = 0.0, q_ = 0.0;
  for (int k = tid; k < parts; k += NTHR) { s_ += p[2 * k]; q_ += p[2 * k + 1]; }
  for (int o = 32; o > 0; o >>= 1) { s_ += __shfl_down(s_, o); q_ += __shfl_down(q_, o); }
  if ((tid & 63) == 0) { wsum[tid >> 6][0] = s_; wsum[tid >> 6][1] = q_; }
  __syncthreads();
  if (tid == 0) {
    double s2 = 0.0, q2 = 0.0;
    for (int w = 0; w < NTHR / 64; ++w) { s2 += wsum[w][0]; q2 += wsum[w][1]; }
    const double mean = s2 / count, var = fmax(q2 / count - mean * mean, 0.0);
    st[0] = (float)mean;
    st[1] = (float)(1.0 / sqrt(var + (double)eps));
  }
  __syncthreads();
}

// DUAL: two layers on the same input in one launch (the reset- and the update-gate convolution of a ConvGRUCell2,
// reference models/module.py:72-92): 8 waves, waves 4-7 take the second layer's weights / bias / skip / output (`b`) over
// the window the first four staged with them; their GroupNorm partials go to group 1.
template <int D, int NTR, bool DUAL>
__global__ __launch_bounds__(DUAL ? 512 : 256) void k_conv_dd_resident(ConvDDArgs a0, ConvDDArgs a1, GruPro pro) {
  constexpr int WM = D / 16, WN = 4 / WM, TR = NTR * WN, KCT = D / 4, NTILES = D / 16;
  constexpr int LR = TR + 2, LC = 18, PLANE = plane_pitch16(LR * LC);
  constexpr int NTHR = DUAL ? 512 : 256;
  using Win = ChunkWindow<LR, LC, LC, KCT, PLANE, 4 * PLANE, NTHR>;      // one chunk: all D channels
  constexpr int NIT = Win::N;
  __shared__ float lds[D * PLANE];
  const int tid = threadIdx.x, lane = tid & 63, wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = DUAL ? wave8 >> 2 : 0, wave = wave8 & 3;
  const ConvDDArgs& a = half ? a1 : a0;
  const int wm = wave % WM, wn = wave / WM;
  const int p = lane & 15, q = lane >> 4;
  const int n = blockIdx.z, r0 = blockIdx.y * TR, c0 = blockIdx.x * 16;
  const int iy0 = r0 - 1, ix0 = c0 - 1;

  // all loads of the block, back to back: A fragments of the wave's channel tile, then the input window
  const buf_rsrc rw = make_rsrc(a.wpk);
  float wf[9][KCT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int kc = 0; kc < KCT; ++kc) wf[t][kc] = load_afrag(rw, (unsigned)(lane * 4), t, kc, wm, KCT, NTILES);
  Win win;
  win.init(a.hi, a.wi, D, iy0, ix0);
  f32x4 xs[NIT];
  win.request(xs, Win::origin(a0.in, n, a.hi, a.wi, D, iy0, ix0), 0);
  if (pro.mode != GRU_PRO_NONE) {                            // uniform: the window is formed from the previous kernels' maps
    __shared__ double wsum[NTHR / 64][2];
    __shared__ float st[2][2];
    gru_pro_stats<NTHR>(pro.part_f + ((size_t)n * 2 + pro.group_f) * pro.parts_f * 2, pro.parts_f, pro.count, pro.eps, wsum, st[0]);
    if (pro.mode == GRU_PRO_OUT) gru_pro_stats<NTHR>(pro.part_o + (size_t)n * pro.parts_o * 2, pro.parts_o, pro.count, pro.eps, wsum, st[1]);
    const buf_rsrc rf = Win::origin(pro.f, n, a.hi, a.wi, D, iy0, ix0);
    const buf_rsrc ro_ = Win::origin(pro.mode == GRU_PRO_OUT ? pro.o : pro.f, n, a.hi, a.wi, D, iy0, ix0);
    const float mf = st[0][0], rf_ = st[0][1], mo = st[1][0], ro2 = st[1][1];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const auto item = Win::item(it);
      const int g = item.g, r = item.r, c = item.c;
      const bool ok = win.goff[it] != BUF_OOB && 4 * g < pro.hc;
      const unsigned off = ok ? win.goff[it] : BUF_OOB;
      const int c4 = min(4 * g, pro.hc - 4);
      const f32x4 fv = buf_load4(rf, off);
      const f32x4 gw = *(const f32x4*)(pro.gn_f + c4), gb = *(const f32x4*)(pro.gn_f + pro.hc + c4);
      const f32x4 fn = (fv - mf) * rf_ * gw + gb;
      const f32x4 sg = {sigmoidf_(fn.x), sigmoidf_(fn.y), sigmoidf_(fn.z), sigmoidf_(fn.w)};
      f32x4 v;
      if (pro.mode == GRU_PRO_GATES) {
        v = sg * xs[it];                                     // r * h
      } else {
        const f32x4 ov = buf_load4(ro_, off);
        const f32x4 ow = *(const f32x4*)(pro.gn_o + c4), ob = *(const f32x4*)(pro.gn_o + pro.hc + c4);
        const f32x4 on = (ov - mo) * ro2 * ow + ob;
        const f32x4 y = {tanhf(on.x), tanhf(on.y), tanhf(on.z), tanhf(on.w)};
        v = sg * xs[it] + (1.0f - sg) * y;                   // h' = u h + (1 - u) y
      }
      xs[it] = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};           // zero padding / padding channels
      // the block's own pixels: the new state (and R)
      if (pro.mode == GRU_PRO_OUT && ok && item.own && r >= 1 && r <= TR && c >= 1 && c <= 16) {
        const size_t pix = ((size_t)n * a.hi + (iy0 + r)) * a.wi + (ix0 + c);
        *(f32x4*)(pro.state_out + pix * D + 4 * g) = xs[it];
        if (pro.R) *(f32x4*)(pro.R + pix * pro.RW + 4 * g) = xs[it];
      }
    }
  }
  if (a0.in2) {                                              // uniform: the layer convolves in + in2
    f32x4 xs2[NIT];
    win.request(xs2, Win::origin(a0.in2, n, a.hi, a.wi, D, iy0, ix0), 0);
#pragma unroll
    for (int it = 0; it < NIT; ++it) xs[it] += xs2[it];
  }
  win.store(xs, lds);
  __syncthreads();

  f32x4 acc[NTR];
#pragma unroll
  for (int r = 0; r < NTR; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* xb = lds + q * PLANE + (wn * NTR) * LC + p;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int kc = 0; kc < KCT; ++kc)
#pragma unroll
      for (int r = 0; r < NTR; ++r)
        acc[r] = mfma16(wf[t][kc], xb[4 * kc * PLANE + (r + t / 3) * LC + t % 3], acc[r]);

  const int co4 = wm * 16 + 4 * q;
  const f32x4 bias = *(const f32x4*)(a.bias + co4);
#pragma unroll
  for (int r = 0; r < NTR; ++r) {
    const int oy = r0 + wn * NTR + r, ox = c0 + p;
    if (oy >= a.ho || ox >= a.wo) continue;
    const size_t opix = ((size_t)n * a.ho + oy) * a.wo + ox;
    f32x4 v = bias_act(acc[r], bias, a.relu);
    if (a.skip) v += *(const f32x4*)(a.skip + opix * D + co4);
    *(f32x4*)(a.out + opix * D + co4) = v;
  }
  if (a.gn_part) {                                           // uniform: the stored values formed again (the same text: chunk_window.h says why)
    double gs = 0.0, gq = 0.0;
#pragma unroll
    for (int r = 0; r < NTR; ++r) {
      const int oy = r0 + wn * NTR + r, ox = c0 + p;
      if (oy < a.ho && ox < a.wo && co4 < a.gn_n) {
        f32x4 v = bias_act(acc[r], bias, a.relu);
        if (a.skip) v += *(const f32x4*)(a.skip + (((size_t)n * a.ho + oy) * a.wo + ox) * D + co4);
        gs += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        gq += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
      }
    }
    for (int o = 32; o > 0; o >>= 1) { gs += __shfl_down(gs, o); gq += __shfl_down(gq, o); }             // fixed tree: deterministic
    if (lane == 0) {
      const int parts = gridDim.x * gridDim.y * 4;
      double* o = a.gn_part + (((size_t)n * a.gn_ngroups + (DUAL ? half : a.gn_group)) * parts + (blockIdx.y * gridDim.x + blockIdx.x) * 4 + wave) * 2;
      o[0] = gs; o[1] = gq;
    }
  }
}

static int small_grid_limit() { return opt(OPT_CONV_SMALL_GRID); }      // workgroups up to which the resident form is used (0 disables it)

template <int D, int NTR>
static int launch_conv_dd_resident_rows(const ConvDDArgs& a, int N, hipStream_t st, const GruPro& pro = GruPro{}) {
  constexpr int TR = NTR * (4 / (D / 16));
  hipLaunchKernelGGL((k_conv_dd_resident<D, NTR, false>), dim3(cdiv(a.wo, 16), cdiv(a.ho, TR), N), dim3(256), 0, st, a, a, pro);
  ADAMVS_CHECK_LAUNCH("conv_dd (resident)");
  return 0;
}
template <int D, int NTR>
static int launch_conv_dd_resident_dual(const ConvDDArgs& a, const ConvDDArgs& b, int N, hipStream_t st, const GruPro& pro = GruPro{}) {
  constexpr int TR = NTR * (4 / (D / 16));
  hipLaunchKernelGGL((k_conv_dd_resident<D, NTR, true>), dim3(cdiv(a.wo, 16), cdiv(a.ho, TR), N), dim3(512), 0, st, a, b, pro);
  ADAMVS_CHECK_LAUNCH("conv_dd (resident, two layers)");
  return 0;
}

// the fewest rows per workgroup (most workgroups) that stays within the limit; 0: grid too large for this form
template <int D>
static int resident_rows(const ConvDDArgs& a, int N) {
  constexpr int WN = 4 / (D / 16);
  const long cols = (long)cdiv(a.wo, 16) * N, limit = small_grid_limit();
  for (int ntr = 1; ntr <= 4; ntr *= 2)
    if (cols * cdiv(a.ho, ntr * WN) <= limit) return ntr;
  return 0;
}
template <int D>
static int launch_conv_dd_resident(const ConvDDArgs& a, int N, hipStream_t st) {
  switch (resident_rows<D>(a, N)) {
    case 1: return launch_conv_dd_resident_rows<D, 1>(a, N, st);
    case 2: return launch_conv_dd_resident_rows<D, 2>(a, N, st);
    case 4: return launch_conv_dd_resident_rows<D, 4>(a, N, st);
  }
  return -1;
}

static int launch_conv_dd_z(const ConvDDArgs& a, int N, int mode, hipStream_t st, int s2_blocks);

// The kernels below take the image index from blockIdx.z (at most 65535): more images run as several launches over
// sub-batches, every pointer moved by whole images (the softmax epilogue's tile index is n % sm_B: sub-batches of whole tiles).
// s2_blocks: the blocks of the stride-2 pair form (s2_pairs_fold; -1 by the map)
static int launch_conv_dd(const ConvDDArgs& a, int N, int mode, hipStream_t st, int s2_blocks = -1) {
  constexpr int ZMAX = 65535;
  if (N <= ZMAX) return launch_conv_dd_z(a, N, mode, st, s2_blocks);
  ADAMVS_CHECK_ARG(!a.gn_part, "conv_dd: GroupNorm partials with N=%d images (at most %d)", N, ZMAX);
  const int unit = a.sm_vw ? a.sm_B : 1;
  ADAMVS_CHECK_ARG(unit <= ZMAX, "conv_dd: softmax epilogue with %d tiles per view (at most %d)", unit, ZMAX);
  const int step = ZMAX / unit * unit;
  const size_t in_img = (size_t)a.hi * a.wi * a.D, out_img = (size_t)a.ho * a.wo * a.D, map = (size_t)a.ho * a.wo;
  for (int n0 = 0; n0 < N; n0 += step) {
    ConvDDArgs b = a;
    b.in = a.in + n0 * in_img;
    if (a.in2) b.in2 = a.in2 + n0 * in_img;
    if (a.out) b.out = a.out + n0 * out_img;
    if (a.skip) b.skip = a.skip + n0 * out_img;
    if (a.sm_vw) { b.sm_vw = a.sm_vw + n0 * map; b.sm_pd = a.sm_pd + n0 * map; }
    if (int rc = launch_conv_dd_z(b, N - n0 < step ? N - n0 : step, mode, st, s2_blocks)) return rc;
  }
  return 0;
}

static int launch_conv_dd_z(const ConvDDArgs& a, int N, int mode, hipStream_t st, int s2_blocks) {
  if (mode == CONV_S1 && (a.D == 32 || a.D == 64) && !a.sm_vw) {
    const int rc = a.D == 32 ? launch_conv_dd_resident<32>(a, N, st) : launch_conv_dd_resident<64>(a, N, st);
    if (rc >= 0) return rc;
  }
  const WidthTiling* t = width_tiling(a.D, a.sm_vw != nullptr);
  if (t) {
    // No softmax epilogue where a width runs as several launches (it needs a pixel's channels in one workgroup): the scores go
    // through the score volume to k_softmax_regress.
    ADAMVS_CHECK_ARG(t->parts == 1 || !a.sm_vw, "conv_dd: no softmax epilogue at D=%d", a.D);
    ConvDDArgs h = a;
    for (int part = 0; part < t->parts; ++part) {
      h.wpk = a.wpk + (size_t)part * (t->chunk / 16) * 64;       // fragment index = (... * D/16 + tile) * 64 floats
      h.bias = a.bias + part * t->chunk;
      h.out = a.out + part * t->chunk;
      h.skip = a.skip ? a.skip + part * t->chunk : nullptr;
      int rc = -1;
      switch (t->MT * 10 + t->WM) {
        case 11: rc = launch_conv_dd_cfg<1, 1>(h, N, mode, st, s2_blocks); break;
        case 21: rc = launch_conv_dd_cfg<2, 1>(h, N, mode, st, s2_blocks); break;
        case 31: rc = launch_conv_dd_cfg<3, 1>(h, N, mode, st, s2_blocks); break;
        case 41: rc = launch_conv_dd_cfg<4, 1>(h, N, mode, st, s2_blocks); break;
        case 32: rc = launch_conv_dd_cfg<3, 2>(h, N, mode, st, s2_blocks); break;
        case 42: rc = launch_conv_dd_cfg<4, 2>(h, N, mode, st, s2_blocks); break;
        case 34: rc = launch_conv_dd_cfg<3, 4>(h, N, mode, st, s2_blocks); break;
        case 44: rc = launch_conv_dd_cfg<4, 4>(h, N, mode, st, s2_blocks); break;
      }
      if (rc) return rc;
    }
    return 0;
  }
  return set_error(-1, "cost_reg_net_2d: D=%d unsupported (16, 32, 48, 64, 96, 128, 192, 256, 384 or 512)", a.D);
}

int launch_conv_dd_gn(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D, int h, int w,
                      hipStream_t st, double* gn_part, int gn_n, int gn_group, int gn_ngroups, int* gn_parts, const GruPro* prop) {
  ConvDDArgs a{in, wpk, bias, skip, out, D, h, w, h, w, 0, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, nullptr};
  *gn_parts = 0;
  if (gn_part && (D == 32 || D == 64)) {
    const int ntr = D == 32 ? resident_rows<32>(a, N) : resident_rows<64>(a, N);
    const long parts = ntr ? (long)cdiv(w, 16) * cdiv(h, ntr * (4 / (D / 16))) * 4 : 0;
    if (gn_epilogue_partials(parts, N)) {
      a.gn_part = gn_part; a.gn_n = gn_n; a.gn_group = gn_group; a.gn_ngroups = gn_ngroups;
      *gn_parts = (int)parts;
      if (prop) {                                            // the caller has asked can_fold_gru_applies(): this branch is taken
        if (D == 32) {
          switch (ntr) { case 1: return launch_conv_dd_resident_rows<32, 1>(a, N, st, *prop);
                         case 2: return launch_conv_dd_resident_rows<32, 2>(a, N, st, *prop);
                         default: return launch_conv_dd_resident_rows<32, 4>(a, N, st, *prop); }
        }
        switch (ntr) { case 1: return launch_conv_dd_resident_rows<64, 1>(a, N, st, *prop);
                       case 2: return launch_conv_dd_resident_rows<64, 2>(a, N, st, *prop);
                       default: return launch_conv_dd_resident_rows<64, 4>(a, N, st, *prop); }
      }
    }
  }
  if (prop) return set_error(-1, "conv_dd: the folded GRU prologue needs the small-grid kernel (D=%d, %dx%d, N=%d)", D, h, w, N);
  return launch_conv_dd(a, N, CONV_S1, st);
}

// true when launch_conv_dd_gn / _gates_gn run a level's convolutions on the small-grid kernel with epilogue partials: the
// condition for folding the elementwise kernels of a ConvGRUCell2 into the convolutions' window fills (msred.hip)
bool can_fold_gru_applies(int N, int D, int h, int w) {
  if (D != 32 && D != 64) return false;
  ConvDDArgs a{nullptr, nullptr, nullptr, nullptr, nullptr, D, h, w, h, w, 0, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, nullptr};
  const int ntr = D == 32 ? resident_rows<32>(a, N) : resident_rows<64>(a, N);
  const long parts = ntr ? (long)cdiv(w, 16) * cdiv(h, ntr * (4 / (D / 16))) * 4 : 0;
  return gru_fold_enabled(N) && gn_epilogue_partials(parts, N);
}

// Two stride-1 layers on the same input (the gate convolutions of a ConvGRUCell2) with their GroupNorm partial sums (groups
// 0 and 1 of 2): ONE launch when the small-grid kernel takes the map (*gn_parts > 0), otherwise two plain launches (*gn_parts = 0).
int launch_conv_dd_gates_gn(const float* in, const float* wpk_r, const float* bias_r, const float* skip_r, float* out_r,
                            const float* wpk_u, const float* bias_u, const float* skip_u, float* out_u, int N, int D, int h, int w,
                            hipStream_t st, double* gn_part, int gn_n, int* gn_parts, const GruPro* prop) {
  const GruPro pro = prop ? *prop : GruPro{};
  ConvDDArgs a{in, wpk_r, bias_r, skip_r, out_r, D, h, w, h, w, 0, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, nullptr};
  ConvDDArgs b = a;
  b.wpk = wpk_u; b.bias = bias_u; b.skip = skip_u; b.out = out_u;
  *gn_parts = 0;
  if (gn_part && (D == 32 || D == 64)) {
    const int ntr = D == 32 ? resident_rows<32>(a, N) : resident_rows<64>(a, N);
    const long parts = ntr ? (long)cdiv(w, 16) * cdiv(h, ntr * (4 / (D / 16))) * 4 : 0;
    if (gn_epilogue_partials(parts, N)) {
      a.gn_part = b.gn_part = gn_part; a.gn_n = b.gn_n = gn_n; a.gn_ngroups = b.gn_ngroups = 2;
      *gn_parts = (int)parts;
      if (D == 32) {
        switch (ntr) { case 1: return launch_conv_dd_resident_dual<32, 1>(a, b, N, st, pro);
                       case 2: return launch_conv_dd_resident_dual<32, 2>(a, b, N, st, pro);
                       default: return launch_conv_dd_resident_dual<32, 4>(a, b, N, st, pro); }
      }
      switch (ntr) { case 1: return launch_conv_dd_resident_dual<64, 1>(a, b, N, st, pro);
                     case 2: return launch_conv_dd_resident_dual<64, 2>(a, b, N, st, pro);
                     default: return launch_conv_dd_resident_dual<64, 4>(a, b, N, st, pro); }
    }
  }
  if (prop) return set_error(-1, "conv_dd: the folded GRU prologue needs the small-grid kernel (D=%d, %dx%d, N=%d)", D, h, w, N);
  if (int rc = launch_conv_dd(a, N, CONV_S1, st)) return rc;
  return launch_conv_dd(b, N, CONV_S1, st);
}

// ---------------------------------------------------------------------------
// softmax over D, max probability, expectation of depth.  16 lanes per pixel.
// score [N=S*B][hw][D] (n = s*B + b), planes [B][D][hw] -> vw, pd [S*B][hw].
// NQ = D/64 rounded up: the lane's scores stay in registers between the max pass and the exp pass, so the
// score volume is read once (NQ = 0: any D, two passes over global memory).
// Dp = hypothesis planes (<= D, the channels of `score`: pad channels carry -1e30 and weigh exactly 0).
template <int NQ>
__global__ __launch_bounds__(256) void k_softmax_regress(const float* __restrict__ score, PlaneSrc planes,
                                                         float* __restrict__ vw, float* __restrict__ pd, int B, int D, int hw,
                                                         size_t npix, int Dp) {
  // persistent: the grid is the resident capacity and a workgroup walks the 16-pixel groups blk, blk + grid, ... -- as one
  // workgroup per group (590 000 of them at cfg2) the launch ran at the rate workgroups are dispatched, 2.2 TB/s
  constexpr int DMAX = NQ > 0 ? 64 * NQ : 1;
  __shared__ float lp[NQ > 0 ? DMAX * 17 : 1];
  const int l = threadIdx.x & 15;
  const size_t nblk = (npix + 15) / 16;
  for (size_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
  size_t gp = blk * 16 + (threadIdx.x >> 4);
  const bool live = gp < npix;
  size_t pix = live ? gp : npix - 1;
  size_t n = pix / hw, pp = pix % hw;
  size_t b = n % B;
  const float* sc = score + pix * D;
  const PlaneLine pl = plane_line(planes, b, pp, Dp, hw);
  // The 16 pixels of a block are consecutive; read per lane, a plane value costs a whole 64-byte sector for 16 bytes
  // (lanes of a wave hold 16 different planes of 4 pixels: 4x the plane volume through L2).  When the block lies inside
  // one map the [D][16] patch is staged through LDS with full sectors instead (row pitch 17: 2-way at worst).
  const size_t gp0 = blk * 16;
  // (generated planes need no staging: a plane value is one multiply and one add)
  const bool staged = NQ > 0 && planes.mode == PLANES_EXPLICIT && gp0 + 16 <= npix && (gp0 % hw) + 16 <= (size_t)hw;     // uniform
  if (staged) {
    const float* src = planes.p + ((gp0 / hw) % B) * Dp * hw + gp0 % hw;
    for (int i = threadIdx.x; i < D * 16; i += 256) lp[(i >> 4) * 17 + (i & 15)] = src[(size_t)min(i >> 4, Dp - 1) * hw + (i & 15)];
    __syncthreads();
  }
  const float* lpp = lp + (threadIdx.x >> 4);
  float m = -INFINITY;
  f32x4 keep[NQ > 0 ? NQ : 1];
  if (NQ > 0) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d = 4 * l + 64 * i;
      keep[i] = d < D ? *(const f32x4*)(sc + d) : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      m = fmaxf(m, fmaxf(fmaxf(keep[i].x, keep[i].y), fmaxf(keep[i].z, keep[i].w)));
    }
  } else {
    for (int d = 4 * l; d < D; d += 64) {
      f32x4 v = *(const f32x4*)(sc + d);
      m = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float se = 0.f, sd = 0.f;
  // explicit fused multiply-adds in a fixed order: the sum must not depend on where the plane values come from (staged
  // through LDS, read from the tensor or generated), which a contraction left to the compiler would not guarantee
  auto term = [&](f32x4 v, int d) {
    float e0 = __expf(v.x - m), e1 = __expf(v.y - m), e2 = __expf(v.z - m), e3 = __expf(v.w - m);
    se += (e0 + e1) + (e2 + e3);
    float p0, p1, p2, p3;
    if (staged) { p0 = lpp[d * 17]; p1 = lpp[(d + 1) * 17]; p2 = lpp[(d + 2) * 17]; p3 = lpp[(d + 3) * 17]; }
    else { p0 = plane_at_pad(planes, pl, d, hw); p1 = plane_at_pad(planes, pl, d + 1, hw); p2 = plane_at_pad(planes, pl, d + 2, hw); p3 = plane_at_pad(planes, pl, d + 3, hw); }
    sd = __fmaf_rn(e3, p3, __fmaf_rn(e2, p2, __fmaf_rn(e1, p1, __fmaf_rn(e0, p0, sd))));
  };
  if (NQ > 0) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int d = 4 * l + 64 * i;
      if (d < D) term(keep[i], d);
    }
  } else {
    for (int d = 4 * l; d < D; d += 64) term(*(const f32x4*)(sc + d), d);
  }
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) { se += __shfl_xor(se, o, 64); sd += __shfl_xor(sd, o, 64); }
  if (live && l == 0) {
    vw[pix] = 1.0f / se;          // max_d softmax = exp(max - max) / sum
    pd[pix] = sd / se;
  }
  if (staged) __syncthreads();    // (uniform) the patch is refilled by the next group
  }
}

// ---------------------------------------------------------------------------
// Layer plan.  Packed weights: 11 layers x (9*D*D fragment floats + D bias floats), in the order
// conv0..conv6, conv7, conv9, conv11, prob; fp32 with D in {64, 128, 192, 256}: followed by the five stride-1 layers
// (conv0, conv2, conv4, conv6, prob) in the F(2x2, 3x3) form, 16*D*D floats each (costreg2d_wino.hip); D >= 128: then conv0 and
// prob in the F(2x4, 3x3) form, 24*D*D floats each (costreg2d_wino24.hip); D >= 192: then conv2 and conv4 in that form.
// Workspace: 3 * N*h*w*D floats.
// sm_vw != null: the `prob` layer reduces its scores over D in its epilogue (costreg_softmax.h) and writes the view
// weights / pair depths of softmax_max_regress directly (score is not written); the caller skips launch_softmax_regress.
bool cost_reg_softmax_fusable(int D, int precision, const PlaneSrc& planes) {
  (void)planes; (void)precision;      // any plane source, both precisions: one code path, so generated == materialised bit for bit
  return opt(OPT_FUSE_SOFTMAX) != 0 && D >= 16;
}

// option winograd = 0: the stride-1 layers on the direct kernel, as in rounds 1-2 (A/B)
bool cost_reg_winograd(int D, int precision) {
  return opt(OPT_WINOGRAD) != 0 && precision == PRECISION_FP32 && wino_depth_supported(D);
}

// conv0 and prob -- the two stride-1 layers on the full-size map, 24 % of cfg2's step -- in the F(2x4, 3x3) form: 24 MFMAs where
// F(2x2, 3x3) issues 32.  Not at D = 64 (the blob carries no such blocks there) and only where its 64-pixel blocks fit the width:
// 256 maps at D = 192, 96 x 192: 10.92 against 11.73 ms; 48 x 96 (two blocks for 96 columns): 3.35 against 2.89.
// Option winograd + 2: never (the maps of before, bit for bit).
bool wino24_depth_supported(int D) { return wino_depth_supported(D) && D >= 128; }
bool cost_reg_wino24(int D, int h, int w) {
  (void)h;
  return !(opt(OPT_WINOGRAD) & 2) && wino24_depth_supported(D) && w >= 128 && cdiv(w, 64) * 64 * 8 <= w * 9;
}

// conv2 and conv4 -- the stride-1 layers of the two inner levels, 96 and 48 pixels wide at cfg2 -- in the F(2x4, 3x3) form on folded
// blocks (costreg2d_wino24.hip: 8 x 32 or 8 x 16 pixels), where those tile the map and the unfolded 64-pixel blocks do not.  From
// D = 192 (the blob carries the blocks from there).  By the map's shape alone, like cost_reg_wino24: the two forms round differently,
// and a tile must give the same bits alone and in a batch (tests/test_full_size_parity.py::test_cfg4_rank_share_against_oracle); the
// folded blocks are the faster ones down to the smallest grid of the cascade (16 maps of 24 x 48: 0.111 -> 0.051 ms; 48 x 96:
// 0.220 -> 0.190; profiles/r10_fold_ab.txt).  Option winograd + 2: F(2x2, 3x3) in every stride-1 layer, as before; + 4: no folded blocks
// in any layer, here and in s2_pairs_fold (value 5: the selection of before round 10, the maps of then bit for bit).
bool wino24_inner_depth_supported(int D) { return wino24_depth_supported(D) && D >= 192; }
int cost_reg_wino24_fold(int N, int D, int h, int w) {
  (void)N;
  if ((opt(OPT_WINOGRAD) & (2 | 4)) || !wino24_inner_depth_supported(D)) return 0;
  const int f = conv_wino24_fold(h, w);
  return f > 1 ? f : 0;
}

int launch_cost_reg_net_2d(const float* x, const float* wpk, float* ws, float* score, int N, int D, int h, int w,
                           int precision, hipStream_t st, float* sm_vw, float* sm_pd, const PlaneSrc* sm_planes, int sm_B, int n_planes, int blocks) {
  // blocks = 0 (adamvs_cost_reg_net_2d_blocks: A/B, tests): no folded blocks, the selection of before; -1: by the maps
  // D = the width the network runs at; n_planes <= D hypothesis planes for the softmax (0: D)
  const bool fuse_softmax = sm_vw != nullptr;
  // the softmax epilogue of the direct kernels needs a pixel's channels in one workgroup: not at D = 384 (two launches)
  const bool epilogue_sm = fuse_softmax && D <= 256;
  const bool wino = cost_reg_winograd(D, precision);
  const size_t F = (size_t)N * h * w * D;
  const size_t LW = (size_t)9 * D * D + D;
  float* conv0 = ws;                  // F
  float* t1 = conv0 + F;              // F/4
  float* conv2 = t1 + F / 4;          // F/4
  float* t3 = conv2 + F / 4;          // F/16
  float* conv4 = t3 + F / 16;         // F/16
  float* t5 = conv4 + F / 16;         // F/64
  float* t6 = t5 + F / 64;            // F/64
  float* x7 = t6 + F / 64;            // F/16
  float* x9 = x7 + F / 16;            // F/4
  float* x11 = x9 + F / 4;            // F
  const int h2 = h / 2, w2 = w / 2, h4 = h / 4, w4 = w / 4, h8 = h / 8, w8 = w / 8;
  // The three skip additions of the hourglass (x = conv4 + conv7(x); x = conv2 + conv9(x); x = conv0 + conv11(x),
  // adamvs.py:233-236).  bf16x3: in the epilogue of the transposed layer that produces x (`skip`).  fp32: in the layer
  // that CONSUMES x (`in2`: the sum is formed when the window enters LDS, one chunk ahead of its use) -- the transposed
  // kernel's epilogue is then bias + ReLU + stores and nothing waits for it.  The same two addends, one fp32 add: same bits.
  struct L { const float* in; float* out; const float* skip; int hi, wi, ho, wo, mode, relu; };
  const L plan[11] = {
      {x, conv0, nullptr, h, w, h, w, CONV_S1, 1},
      {conv0, t1, nullptr, h, w, h2, w2, CONV_S2, 1},
      {t1, conv2, nullptr, h2, w2, h2, w2, CONV_S1, 1},
      {conv2, t3, nullptr, h2, w2, h4, w4, CONV_S2, 1},
      {t3, conv4, nullptr, h4, w4, h4, w4, CONV_S1, 1},
      {conv4, t5, nullptr, h4, w4, h8, w8, CONV_S2, 1},
      {t5, t6, nullptr, h8, w8, h8, w8, CONV_S1, 1},
      {t6, x7, conv4, h8, w8, h4, w4, CONV_T2, 1},
      {x7, x9, conv2, h4, w4, h2, w2, CONV_T2, 1},
      {x9, x11, conv0, h2, w2, h, w, CONV_T2, 1},
      {x11, score, nullptr, h, w, h, w, CONV_S1, 0},
  };
  // deferred where the CONSUMER is a transposed layer (conv7 -> conv9 -> conv11: its window is small and re-read per
  // class anyway); conv11 keeps its own skip: in the stride-1 kernel of `prob` a second input costs more than the epilogue
  // of conv11 gains (measured at cfg2: prob 42.9 -> 45.4 ms against conv11 13.6 -> 12.3)
  const bool defer = precision == PRECISION_FP32 && costreg_deferred_skips();
  for (int i = 0; i < 11; ++i) {
    const float* wl = wpk + (size_t)i * LW;
    int rc;
    if (precision == PRECISION_BF16X3) {
      const bool sm = i == 10 && epilogue_sm;
      rc = launch_conv_dd_bf16x3(plan[i].in, wl, wl + (size_t)9 * D * D, plan[i].skip, plan[i].out, N, D, plan[i].hi,
                                 plan[i].wi, plan[i].ho, plan[i].wo, plan[i].mode, plan[i].relu, st, sm ? sm_vw : nullptr,
                                 sm ? sm_pd : nullptr, sm ? sm_planes : nullptr, sm_B, n_planes);
      if (!rc && i == 10 && fuse_softmax && !epilogue_sm)
        rc = launch_softmax_regress(score, *sm_planes, sm_vw, sm_pd, N / sm_B, sm_B, D, h, w, st, n_planes);
    } else if (wino && plan[i].mode == CONV_S1) {
      // stride-1 layers in the minimal-filtering form (none of them carries a skip or takes a second input).  The channel groups of
      // a pixel are different workgroups there, so the softmax behind the last layer is every lane's partial + a merge kernel
      // (uniform planes: stage 1); with per-pixel planes, or ADAMVS_WINO_SOFTMAX=0, the scores go through the score volume to
      // k_softmax_regress
      const bool folded = blocks != 0 && (i == 2 || i == 4) && cost_reg_wino24_fold(N, D, plan[i].hi, plan[i].wi) > 0;
      const bool w24 = ((i == 0 || i == 10) && cost_reg_wino24(D, h, w)) || folded;
      // the F(2x4, 3x3) blocks of the blob: conv0, prob, then (D >= 192) conv2, conv4
      const float* ww = w24 ? wpk + (size_t)11 * LW + (size_t)5 * 16 * D * D + (size_t)(i == 0 ? 0 : (i == 10 ? 1 : 1 + i / 2)) * 24 * D * D
                            : wpk + (size_t)11 * LW + (size_t)(i == 10 ? 4 : i / 2) * 16 * D * D;
      if (i == 10 && fuse_softmax && wino_softmax_fused() && sm_planes->mode == PLANES_UNIFORM && (n_planes > 0 ? n_planes : D) > 1) {
        // every lane's softmax partial instead of the scores (D bytes per pixel instead of 4 D), in the score volume's place
        rc = (w24 ? launch_conv_wino24_softmax : launch_conv_wino_softmax)(plan[i].in, ww, wl + (size_t)9 * D * D, score, *sm_planes, sm_vw, sm_pd, N,
                                                                           sm_B, D, n_planes, h, w, st);
      } else {
        rc = w24 ? launch_conv_wino24(plan[i].in, ww, wl + (size_t)9 * D * D, nullptr, plan[i].out, N, D, plan[i].hi, plan[i].wi, plan[i].relu, st)
                 : launch_conv_wino(plan[i].in, ww, wl + (size_t)9 * D * D, nullptr, plan[i].out, N, D, plan[i].hi, plan[i].wi, plan[i].relu, st);
        if (!rc && i == 10 && fuse_softmax) rc = launch_softmax_regress(score, *sm_planes, sm_vw, sm_pd, N / sm_B, sm_B, D, h, w, st, n_planes);
      }
    } else {
      const bool give = defer && i + 1 < 11 && plan[i + 1].mode == CONV_T2;        // layer i + 1 adds this layer's skip to its input
      const bool take = defer && i > 0 && plan[i].mode == CONV_T2 && plan[i - 1].skip;
      ConvDDArgs a{plan[i].in, wl, wl + (size_t)9 * D * D, give ? nullptr : plan[i].skip, plan[i].out, D,
                   plan[i].hi, plan[i].wi, plan[i].ho, plan[i].wo, plan[i].relu, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1,
                   take ? plan[i - 1].skip : nullptr};
      if (i == 10 && epilogue_sm) { a.sm_vw = sm_vw; a.sm_pd = sm_pd; a.sm_planes = *sm_planes; a.sm_B = sm_B; a.sm_D = n_planes; }
      rc = launch_conv_dd(a, N, plan[i].mode, st, blocks);
      if (!rc && i == 10 && fuse_softmax && !epilogue_sm)
        rc = launch_softmax_regress(score, *sm_planes, sm_vw, sm_pd, N / sm_B, sm_B, D, h, w, st, n_planes);
    }
    if (rc) return rc;
  }
  return 0;
}

template <int NQ>
static int launch_softmax_nq(const float* score, const PlaneSrc& planes, float* vw, float* pd, int B, int D, int hw, size_t npix, int Dp,
                             hipStream_t st) {
  return launch_resident<k_softmax_regress<NQ>>((long)((npix + 15) / 16), 0, st, "softmax_regress", score, planes, vw, pd, B, D, hw,
                                                npix, Dp);
}

int launch_softmax_regress(const float* score, PlaneSrc planes, float* vw, float* pd, int S, int B, int D, int h, int w,
                           hipStream_t st, int n_planes) {
  size_t npix = (size_t)S * B * h * w;
  const int Dp = n_planes > 0 ? n_planes : D;
  ADAMVS_CHECK_ARG(Dp <= D, "softmax_regress: %d planes for %d score channels", Dp, D);
  switch ((D + 63) / 64) {
    case 1: return launch_softmax_nq<1>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    case 2: return launch_softmax_nq<2>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    case 3: return launch_softmax_nq<3>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    case 4: return launch_softmax_nq<4>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    case 6: return launch_softmax_nq<6>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    case 8: return launch_softmax_nq<8>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
    default: return launch_softmax_nq<0>(score, planes, vw, pd, B, D, h * w, npix, Dp, st);
  }
}

}  // namespace adamvs

using namespace adamvs;

extern "C" size_t adamvs_cost_reg_net_2d_workspace_bytes(int N, int D, int h, int w) {
  return (size_t)3 * N * h * w * D * sizeof(float);
}

static int check_precision(int precision, int D, const char* who) {
  ADAMVS_CHECK_ARG(precision == PRECISION_FP32 || precision == PRECISION_BF16X3, "%s: precision=%d (0 fp32, 1 bf16x3)", who, precision);
  ADAMVS_CHECK_ARG(precision == PRECISION_FP32 || costreg_bf16x3_depth_supported(D),
                   "%s: bf16x3 needs D in {32,64,96,128,192,256,384,512}, got %d", who, D);
  return 0;
}

extern "C" int adamvs_conv_t2_form(int N, int D, int hi, int wi) { return N > 0 && hi > 0 && wi > 0 ? conv_t2_form(N, D, hi, wi) : -1; }

extern "C" int adamvs_conv_s2_form(int N, int D, int hi, int wi, int blocks) { return N > 0 && hi > 1 && wi > 1 ? conv_s2_form(N, D, hi, wi, blocks) : -1; }
extern "C" int adamvs_cost_reg_fold(int N, int D, int h, int w) { return N > 0 && h > 0 && w > 0 ? cost_reg_wino24_fold(N, D, h, w) : -1; }
extern "C" int adamvs_conv_wino24_fold(int h, int w, int blocks) { return h > 0 && w > 0 ? conv_wino24_fold(h, w, blocks) : -1; }

extern "C" int adamvs_cost_reg_width(int D, int precision) {
  return D < 1 ? 0 : (precision == PRECISION_BF16X3 ? costreg_width_bf16x3(D) : costreg_width(D));
}

size_t adamvs::cost_reg_weight_floats(int D, int precision) {
  if (!(precision == PRECISION_BF16X3 ? costreg_bf16x3_depth_supported(D) : costreg_depth_supported(D))) return 0;
  return (size_t)11 * ((size_t)9 * D * D + D) + (precision == PRECISION_FP32 && wino_depth_supported(D) ? (size_t)5 * 16 * D * D : 0) +
         (precision == PRECISION_FP32 && wino24_depth_supported(D) ? (size_t)2 * 24 * D * D : 0) +
         (precision == PRECISION_FP32 && wino24_inner_depth_supported(D) ? (size_t)2 * 24 * D * D : 0);
}
extern "C" size_t adamvs_cost_reg_net_2d_weight_floats(int D, int precision) { return cost_reg_weight_floats(D, precision); }

extern "C" int adamvs_cost_reg_net_2d(const float* x, const float* wpk, size_t wpk_floats, float* score, int N, int D, int h, int w,
                                      int precision, void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_precision(precision, D, "cost_reg_net_2d")) return rc;
  ADAMVS_CHECK_ARG(x && wpk && score && workspace && N > 0 && h > 0 && w > 0, "cost_reg_net_2d: bad arguments");
  ADAMVS_CHECK_ARG(costreg_depth_supported(D), "cost_reg_net_2d: D=%d unsupported (16, 32, 48, 64, 96, 128, 192, 256, 384 or 512)", D);
  ADAMVS_CHECK_ARG(wpk_floats == cost_reg_weight_floats(D, precision),
                   "cost_reg_net_2d: wpk holds %zu floats, the layout for D=%d precision=%d has %zu (include/adamvs_hip.h)", wpk_floats, D,
                   precision, cost_reg_weight_floats(D, precision));
  ADAMVS_CHECK_ARG((h % 8) == 0 && (w % 8) == 0, "cost_reg_net_2d: h=%d w=%d must be multiples of 8 (three stride-2 levels)", h, w);
  ADAMVS_CHECK_ARG(workspace_bytes >= adamvs_cost_reg_net_2d_workspace_bytes(N, D, h, w),
                   "cost_reg_net_2d: workspace too small (%zu < %zu bytes)", workspace_bytes,
                   adamvs_cost_reg_net_2d_workspace_bytes(N, D, h, w));
  return launch_cost_reg_net_2d(x, wpk, (float*)workspace, score, N, D, h, w, precision, (hipStream_t)stream);
}

extern "C" int adamvs_cost_reg_net_2d_blocks(const float* x, const float* wpk, size_t wpk_floats, float* score, int N, int D, int h, int w,
                                             int blocks, void* workspace, size_t workspace_bytes, void* stream) {
  ADAMVS_CHECK_ARG(x && wpk && score && workspace && N > 0 && h > 0 && w > 0, "cost_reg_net_2d_blocks: bad arguments");
  ADAMVS_CHECK_ARG(blocks == -1 || blocks == 0, "cost_reg_net_2d_blocks: blocks=%d (-1 by the maps, 0 no folded blocks)", blocks);
  ADAMVS_CHECK_ARG(costreg_depth_supported(D), "cost_reg_net_2d_blocks: D=%d unsupported", D);
  ADAMVS_CHECK_ARG(wpk_floats == cost_reg_weight_floats(D, PRECISION_FP32), "cost_reg_net_2d_blocks: wpk holds %zu floats, the layout for D=%d has %zu",
                   wpk_floats, D, cost_reg_weight_floats(D, PRECISION_FP32));
  ADAMVS_CHECK_ARG((h % 8) == 0 && (w % 8) == 0, "cost_reg_net_2d_blocks: h=%d w=%d must be multiples of 8", h, w);
  ADAMVS_CHECK_ARG(workspace_bytes >= adamvs_cost_reg_net_2d_workspace_bytes(N, D, h, w), "cost_reg_net_2d_blocks: workspace too small (%zu bytes)",
                   workspace_bytes);
  return launch_cost_reg_net_2d(x, wpk, (float*)workspace, score, N, D, h, w, PRECISION_FP32, (hipStream_t)stream, nullptr, nullptr, nullptr, 1, 0, blocks);
}

extern "C" int adamvs_conv3x3_dd_s2_blocks(const float* in, const float* wpk, const float* bias, float* out, int N, int D, int hi, int wi,
                                           int relu, int blocks, void* stream) {
  ADAMVS_CHECK_ARG(in && wpk && bias && out && N > 0 && hi > 0 && wi > 0, "conv3x3_dd_s2_blocks: bad arguments");
  ADAMVS_CHECK_ARG(costreg_depth_supported(D), "conv3x3_dd_s2_blocks: D=%d unsupported", D);
  ADAMVS_CHECK_ARG((hi % 2) == 0 && (wi % 2) == 0, "conv3x3_dd_s2_blocks: stride 2 needs even hi, wi");
  ADAMVS_CHECK_ARG(blocks == -1 || blocks == 0 || blocks == 2 || blocks == 4, "conv3x3_dd_s2_blocks: blocks=%d (-1 by the map, 0, 2, 4)", blocks);
  ConvDDArgs a{in, wpk, bias, nullptr, out, D, hi, wi, hi / 2, wi / 2, relu, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, nullptr};
  return launch_conv_dd(a, N, CONV_S2, (hipStream_t)stream, blocks);
}

extern "C" int adamvs_conv3x3_dd(const float* in, const float* in2, const float* wpk, const float* bias, const float* skip,
                                 float* out, int N, int D, int hi, int wi, int mode, int relu, int precision, void* stream) {
  if (int rc = check_precision(precision, D, "conv3x3_dd")) return rc;
  ADAMVS_CHECK_ARG(in && wpk && bias && out && N > 0 && hi > 0 && wi > 0, "conv3x3_dd: bad arguments");
  ADAMVS_CHECK_ARG(costreg_depth_supported(D), "conv3x3_dd: D=%d unsupported (16, 32, 48, 64, 96, 128, 192, 256, 384 or 512)", D);
  ADAMVS_CHECK_ARG(mode >= 0 && mode <= 2, "conv3x3_dd: mode=%d (0 stride 1, 1 stride 2, 2 transposed stride 2)", mode);
  ADAMVS_CHECK_ARG(mode != CONV_S2 || ((hi % 2) == 0 && (wi % 2) == 0), "conv3x3_dd: stride 2 needs even hi, wi");
  int ho = mode == CONV_S2 ? hi / 2 : (mode == CONV_T2 ? 2 * hi : hi);
  int wo = mode == CONV_S2 ? wi / 2 : (mode == CONV_T2 ? 2 * wi : wi);
  ADAMVS_CHECK_ARG(!(in2 && (precision == PRECISION_BF16X3 || mode == CONV_S2)),
                   "conv3x3_dd: in2 is implemented for fp32, modes 0 and 2 (otherwise pass the addition as the producer's skip)");
  if (precision == PRECISION_BF16X3)
    return launch_conv_dd_bf16x3(in, wpk, bias, skip, out, N, D, hi, wi, ho, wo, mode, relu, (hipStream_t)stream);
  ConvDDArgs a{in, wpk, bias, skip, out, D, hi, wi, ho, wo, relu, nullptr, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, in2};
  return launch_conv_dd(a, N, mode, (hipStream_t)stream);
}

extern "C" int adamvs_prob_softmax_regress(const float* in, const float* wpk, const float* bias, const float* planes,
                                           float* view_weight, float* pair_depth, int S, int B, int D, int h, int w, int precision,
                                           void* stream) {
  if (int rc = check_precision(precision, D, "prob_softmax_regress")) return rc;
  ADAMVS_CHECK_ARG(in && wpk && bias && planes && view_weight && pair_depth && S > 0 && B > 0 && h > 0 && w > 0,
                   "prob_softmax_regress: bad arguments");
  ADAMVS_CHECK_ARG(costreg_depth_supported(D) && D <= 256, "prob_softmax_regress: D=%d unsupported (16, 32, 48, 64, 96, 128, 192 or 256)", D);
  const PlaneSrc ps = explicit_planes(planes);
  if (precision == PRECISION_BF16X3)
    return launch_conv_dd_bf16x3(in, wpk, bias, nullptr, nullptr, S * B, D, h, w, h, w, CONV_S1, 0, (hipStream_t)stream, view_weight,
                                 pair_depth, &ps, B);
  ConvDDArgs a{in, wpk, bias, nullptr, nullptr, D, h, w, h, w, 0, view_weight, pair_depth, ps, B, nullptr};
  return launch_conv_dd(a, S * B, CONV_S1, (hipStream_t)stream);
}

extern "C" int adamvs_softmax_max_regress(const float* score, const float* planes, float* view_weight, float* pair_depth,
                                          int S, int B, int D, int h, int w, void* stream) {
  ADAMVS_CHECK_ARG(score && planes && view_weight && pair_depth && S > 0 && B > 0 && D > 0 && (D % 4) == 0 && h > 0 && w > 0,
                   "softmax_max_regress: bad arguments (D=%d must be a multiple of 4)", D);
  return launch_softmax_regress(score, explicit_planes(planes), view_weight, pair_depth, S, B, D, h, w, (hipStream_t)stream);
}
