// Stride-1 layers of CostRegNet2D (reference models/adamvs.py:198-238: conv0, conv2, conv4, conv6, prob; blocks
// models/module.py:254-261) in the minimal-filtering form F(2x4, 3x3): a 2 x 4 output tile from a 4 x 6 input patch,
// 24 products per (cin, cout) pair instead of the direct form's 72 (F(2x2, 3x3), costreg2d_wino.hip: 32 for the same
// eight outputs), fp32 throughout.
//     Y = At2 [ (G2 g G4t) .* (Bt2 d B4) ] A4,       d = the 4 x 6 input patch, g = the 3 x 3 filter
//     rows    (F(2,3)): Bt2 = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1],  G2 = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1],  At2 = [1 1 1 0; 0 1 -1 -1]
//     columns (F(4,3)): Bt4 = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1],
//                       G4  = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1],
//                       At4 = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// Why 2 x 4 and not 4 x 4 (36 products per sixteen outputs): this kernel family gives a WAVE one row i of the transformed
// patch -- its row of Bt d B costs a handful of packed vector instructions, and every transformed value feeds MT MFMAs --
// and a workgroup one wave per SIMD.  Six patch rows do not divide over four SIMDs; three rows per wave (18 positions)
// leave accumulator registers for one tile row and two channel tiles, i.e. one MFMA per weight fragment fetched from L2
// (32 B per CU and clock).  With four rows of six positions the wave keeps 6 x MT 4 x NT 2 = 48 accumulator tiles -- the
// 192 registers of the F(2x2, 3x3) kernel -- and the same 48 MFMAs per k-step, for 4 x 64 instead of 6 x 32 output pixels.
// Rounding: the column transform has the factors 4, 5, 8 and 1/24: 9e-7 relative L1 against a float64 convolution at
// D = 192 where the direct kernel has 6e-7 and F(2x2, 3x3) 4e-7; per element at most 2.9e-6 of max |ref| (tests/test_costreg_wino24.py).
//
// OUTCOME.  Round 4 (one workgroup per CU, MT 4 x NT 2): a quarter fewer MFMAs than F(2x2, 3x3), 3.5 % less time at 96 x 192, slower on
// every smaller level of the hourglass; the network stayed on F(2x2, 3x3).  Round 9: two workgroups per CU (WPS 2, 24 accumulator
// tiles per wave: MT 2 x NT 2 or MT 4 x NT 1), the bias through the accumulators, the softmax partials of `prob` (SM).  256 maps of
// 96 x 192 at D = 192: 10.92 ms (MT 2 x NT 2) / 11.01 (MT 4 x NT 1) / 11.13 (one workgroup) against 11.73 for F(2x2, 3x3); with the
// softmax partials 10.97 (MT 4 x NT 1) / 12.11 (one workgroup) against 12.02.  48 x 96, where 64-pixel blocks cover 128 columns: 3.35
// against 2.89.  conv0 and prob of the network take this form on maps at least 128 wide (costreg2d.hip::cost_reg_wino24): cfg2's step
// 385.7 -> 376.9 ms.  Timing builds of round 4 (-DWINO24_EXP, of 5.84 ms per 128 maps, one workgroup per CU): no epilogue -0.53, no
// fragment loads -0.68, no transform -0.71, no window fill and barrier -0.97, no raw-row reads -0.57 -- every part a tenth, none dominant.
// Round 10: folded blocks (FOLD, below) tile the 96- and 48-pixel levels; 1024 maps at D = 192: 48 x 96 10.66 ms on 8 x 32 blocks against
// 11.54 for F(2x2, 3x3) (13.43 on 64-pixel blocks), 24 x 48 2.51 on 8 x 16 against 3.79 (3.33); conv2 and conv4 of the network take them:
// cfg2's step 373.2 -> 368.3 ms together with the folded stride-2 pair form (costreg2d.hip).  The FOLD 1 instantiations are the
// instruction streams of before.
//
// Mapping (as costreg2d_wino.hip unless said): workgroup = 4 waves = patch rows i; a tile = NT tile rows x 16 tiles x
// MT channel tiles = 2 NT x 64 output pixels x 16 MT channels; LDS window (2 NT + 2) x 66 pixels x 16 input channels, double-buffered,
// one barrier per chunk.  Per tile row and k-step a wave reads two raw rows of six (six ds_read_b64), forms
// T = rowA + sgn rowB (three packed FMAs) and the six column values in six more:
//     (v0, v5) = 4 (t0, t1) - 5 (t2, t3) + (t4, t5)
//     (a, c) = t4 - (4, 1) t2,  (b, e) = t3 - (4, 1) t1,   (v1, v2) = a +- b,   (v3, v4) = c +- 2 e
// -- every operand a register pair as it was loaded (op_sel picks the half), nine packed instructions per 24 MFMAs.
// Weight fragments: per (k-step, row i, channel tile) a lane holds the six positions of its row, fetched as 16 + 8 bytes
// from two arrays.  Epilogue: Z_i[b] = sum_j At4[b][j] M[i][j] (b = 0..3) in registers, through LDS (4 rows x 4 b x MT x 1 KB),
// wave (a, b') forms Y[a][b] = sum_i At2[a][i] Z_i[b] for b = 2 b', 2 b' + 1, applies ReLU / skip and stores (the bias came through
// accumulator position (1, 1)); SM: the softmax partial of the lane's 16 MT channels instead, as k_conv_wino<..., SM>.
// FOLD (Wino24Geom): an MFMA column is an independent tile, and nothing above needs the 16 of an instruction in one tile row.  With
// FOLD = F they are 16 / F tiles of each of F tile rows: the block is 2 NT F rows x 64 / F columns, the window (2 NT F + 2) x (64 / F + 2)
// pixels at a row pitch that keeps the raw-row reads on 16 different bank quadruples; the lane's tile row and tile enter the pinned
// read bases and the epilogue's lane offset once, the loop is the unfolded one.  conv2 / conv4 of the network (96 and 48 columns:
// 3 x 32, 3 x 16) take FOLD 2 (MT 2 x NT 2: 8 x 32) and FOLD 4 (MT 4 x NT 1: 8 x 16) (costreg2d.hip::cost_reg_wino24_fold).
#include <stdlib.h>
#include <type_traits>

#include "common.h"
#include "costreg_softmax.h"
#include "costreg_wino.h"
#include "kernels.h"
#include "persistent.h"
#include "planes.h"

// Timing builds only (tools/build_variant.py <name> -DWINO24_EXP=<bits>; results are wrong): 1 no epilogue, 2 no weight loads in the loop,
// 4 no input transform, 8 no window fill / barrier (32 no barrier only, 64 no LDS stores only, 128 no window loads only), 256 no raw-row reads.
#ifndef WINO24_EXP
#define WINO24_EXP 0
#endif

namespace adamvs {

// WinoArgs (costreg_wino.h); wpk: [D/4][4][D/16][64][4] (patch columns 0-3) then [D/4][4][D/16][64][2] (columns 4, 5): k-step, patch
// row i, channel tile, lane (A-fragment order) -- 24 bytes per lane and (k-step, channel tile), fetched as 16 + 8

// FOLD = F: the 16 MFMA columns are 16 / F tiles of each of F tile rows -- a block F times narrower and F times taller, the same
// accumulators, fragments and MFMAs (levels of the hourglass whose width is no multiple of 64: 96 = 3 x 32, 48 = 3 x 16).  Lane p
// holds tile p % (16 / F) of the tile rows (p / (16 / F)) NT + t, t = 0 .. NT - 1.
template <int MT, int NT, int FOLD = 1>
struct Wino24Geom {
  static_assert(FOLD == 1 || FOLD == 2 || FOLD == 4, "16 / FOLD tiles of FOLD tile rows");
  static constexpr int KC = 16, KS = KC / 4;                 // input channels per LDS chunk, k-steps per chunk
  static constexpr int TPR = 16 / FOLD, BW = 4 * TPR, BH = 2 * NT * FOLD;   // tiles per tile row; the block's columns and rows
  static constexpr int LR = BH + 2, LCW = BW + 2;            // the window
  // Row pitch: the 16 lanes p of a ds_read_b64 start at pixel (p / TPR) 2 NT LC + 4 (p % TPR) of their plane and must take 16
  // different bank quadruples, as the pixels 4 p of the unfolded form do: the smallest pitch from the window's width up that does it
  // (FOLD 1: 66, the window; FOLD 2, NT 2: 40 for 34; FOLD 4, NT 1: 24 for 18).  The pad columns are filled with zeros and never read.
  static constexpr bool pitch_ok(int lc) {
    unsigned seen = 0;
    for (int p = 0; p < 16; ++p) seen |= 1u << ((((p / TPR) * 2 * NT * lc + 4 * (p % TPR)) & 63) >> 2);
    return seen == 0xffffu && lc % 2 == 0;                   // (even: the 8-byte reads at pixel 4 t + 2 j stay aligned)
  }
  static constexpr int pitch() { int lc = LCW; while (!pitch_ok(lc)) ++lc; return lc; }
  static constexpr int LC = pitch(), NPIX = LR * LC;
  // == 2 (mod 4): a lane reads 8 bytes at pixel 4 p -- banks 4p, 4p+1 -- and the k-rows q, q + 1 of a 32-lane ds_read_b64 group take the other two of every four
  static constexpr int PLANE = (NPIX + 3) / 4 * 4 + 2;
  static constexpr int GP = (4 * PLANE + 63) / 64 * 64 + 16; // channel-group pitch: the 4 groups of 16 neighbouring pixels of a fill on 64 different banks
  static constexpr int CHUNK = KS * GP;                      // floats per buffer
  static constexpr int ZFLOATS = 4 * 4 * MT * 64 * 4;        // epilogue exchange of one tile row
  static constexpr int LDS_FLOATS = (2 * CHUNK > ZFLOATS) ? 2 * CHUNK : ZFLOATS;
  static constexpr size_t LDS_BYTES = (size_t)(LDS_FLOATS + 512) * 4;   // dynamic: above 64 KB with MT = 4
  static_assert(PLANE >= NPIX, "plane pitch");
};

template <int MT, int NT, int WPS, bool SM, int FOLD = 1>
__global__ __launch_bounds__(256, WPS) void k_conv_wino24(WinoArgs a, TileGrid tg, int groups, unsigned mgroups) {
  using G = Wino24Geom<MT, NT, FOLD>;
  static_assert(!SM || MT == 4, "k_softmax_merge reads four partials per channel group of 64");
  constexpr int KC = G::KC, KS = G::KS, LC = G::LC, LCW = G::LCW, TPR = G::TPR, NPIX = G::NPIX, PLANE = G::PLANE, GP = G::GP, CHUNK = G::CHUNK;
  constexpr int NITEMS = NPIX * (KC / 4), NITA = (NITEMS + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) float lds[];   // G::LDS_BYTES: the buffers / the epilogue's exchange + the layer's bias vector (D <= 512)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave = patch row i
  const int p = lane & 15, q = lane >> 4;
  const int fr = FOLD == 1 ? 0 : p / TPR, ft = FOLD == 1 ? p : p % TPR;   // the lane's tile: tile rows fr NT + t, tile ft of the row
  const int D = a.D, NTILES = D / 16, NC = D / KC;

  // ---- per-lane constants (tile-independent)
  // window fill: item = (pixel of the window, group of 4 channels of the chunk); lane tid holds the items tid + 256 it: the same
  // channel group g for all of them and the pixels pp0 + 64 it -- LDS addresses one pinned base + immediates, global offsets
  // formed per tile (window_of) from (row, column) = pp / LC, pp % LC.  The last round's surplus lanes repeat the last item.
  constexpr int LAST = NITEMS - 1 - 256 * (NITA - 1);        // last item of the last round
  const int fg = tid & 3, pp0 = tid >> 2;
  const int ppl = tid <= LAST ? pp0 + 64 * (NITA - 1) : NPIX - 1;
  unsigned xlds0 = (unsigned)((fg * GP + pp0) * 4), xldsl = (unsigned)(((tid <= LAST ? fg : KC / 4 - 1) * GP + ppl) * 4);
  unsigned gch = (unsigned)((tid <= LAST ? fg : KC / 4 - 1) * 16);   // the last round's channel-group byte offset
  pin(xlds0); pin(xldsl);
  // raw patch rows of the wave: T = rowA + sgn * rowB  (i = 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3)
  const int rowA = wave == 0 ? 0 : (wave == 2 ? 2 : 1);
  const int rowB = wave == 3 ? 3 : (wave == 2 ? 1 : 2);
  const float sgn = wave == 1 ? 1.0f : -1.0f;
  const f32x2 sgn2 = {sgn, sgn};
  f32x2 k41 = {-4.0f, -1.0f}, kpm = {1.0f, -1.0f}, kpm2 = {2.0f, -2.0f}, k4 = {4.0f, 4.0f}, k5 = {-5.0f, -5.0f};
  // three separately pinned bases per row: merged into ds_read2_b64 the pairs would need a vector add per read for the address
  unsigned pa0 = (unsigned)((q * PLANE + (2 * NT * fr + rowA) * LC + 4 * ft) * 4), pb0 = (unsigned)((q * PLANE + (2 * NT * fr + rowB) * LC + 4 * ft) * 4);
  unsigned pa1 = pa0 + 8, pa2 = pa0 + 16, pb1 = pb0 + 8, pb2 = pb0 + 16;
  pin(pa0); pin(pa1); pin(pa2); pin(pb0); pin(pb1); pin(pb2);
  const buf_rsrc rw = make_rsrc(a.wpk);
  const unsigned wsecond = (unsigned)D * (unsigned)D * 16u * 4u;     // byte offset of the array of patch columns 4, 5
  unsigned woff = (unsigned)(lane * 16), woff2 = wsecond + (unsigned)(lane * 8);
  pin(woff); pin(woff2);
  // epilogue: wave (oa, ob) stores output pixels (2 ty + oa, 4 tx + 2 ob + {0, 1}) of every 2 x 4 tile
  const int oa = wave >> 1, ob = wave & 1;
  const float os = oa ? -1.0f : 1.0f;
  unsigned ooff = (unsigned)((((2 * NT * fr + oa) * a.w + 4 * ft + 2 * ob) * D + 4 * q) * 4);   // + the tile's origin and the tile row
  pin(ooff);

  struct Tile { int n, r0, c0, cg; };
  auto decode = [&](int t) {
    int n, tx, ty;
    tile_coords(tg, t, n, tx, ty);                           // tx runs over (block column, channel group)
    const int bx = groups == 1 ? tx : (int)__umulhi((unsigned)tx, mgroups);
    return Tile{n, ty * G::BH, bx * G::BW, tx - bx * groups};
  };
  buf_rsrc rx;
  unsigned xoff[NITA];
  auto window_of = [&](const Tile& t) {                      // out-of-image pixels read as zero (BUF_OOB)
    rx = make_rsrc((const char*)a.in + (((long)t.n * a.h + (t.r0 - 1)) * a.w + (t.c0 - 1)) * (long)D * 4);
#pragma unroll
    for (int it = 0; it < NITA; ++it) {
      const int pp = it + 1 < NITA ? pp0 + 64 * it : ppl, r = pp / LC, c = pp - r * LC;
      const bool ok = (unsigned)(t.r0 - 1 + r) < (unsigned)a.h && (unsigned)(t.c0 - 1 + c) < (unsigned)a.w && (LC == LCW || c < LCW);
      xoff[it] = ok ? (unsigned)((r * a.w + c) * D * 4) + (it + 1 < NITA ? (unsigned)(fg * 16) : gch) : BUF_OOB;
    }
  };

  f32x4 acc[6][MT][NT];
  f32x4 xs[NITA];
  struct Frag { f32x4 lo[MT]; f32x2 hi[MT]; };               // positions 0-3 | 4, 5 of the wave's row
  Frag wf0, wf1, wf2, wf3;                                   // four named fragment sets (below)
  // The bias rides in the accumulators: At2 E A4 is all ones for E = the unit matrix element (1, 1) in this form too (column 1 of
  // At2 and of At4 is all ones), so position (1, 1) of every tile starts from the bias (wave 1, first k-step); from LDS, as in k_conv_wino
  f32x4 cb[MT];
  for (int i = tid; i < D; i += 256) lds[G::LDS_FLOATS + i] = a.bias[i];
  int cg = 0;                                                // channel group of the fragments being requested

  auto load_w = [&](Frag& wf, int ks) {                      // ks: global k-step
    if ((WINO24_EXP & 2) && ks > 3) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const unsigned frag = (unsigned)((ks * 4 + wave) * NTILES + cg * MT + mt);                          // uniform
      wf.lo[mt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, woff, frag * 1024u, 0));
      wf.hi[mt] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rw, woff2, frag * 512u, 0));
    }
  };
  auto load_x = [&](int ch) {
#pragma unroll
    for (int it = 0; it < NITA; ++it)
      xs[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, xoff[it], (unsigned)ch * 4u, 0));
  };
  auto read_bias = [&]() {                                   // before the first k-step of a tile (cg = its channel group)
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const f32x4 b = *(const f32x4*)(lds + G::LDS_FLOATS + (cg * MT + mt) * 16 + 4 * q);
      cb[mt] = wave == 1 ? b : zero;
    }
  };
  auto store_items = [&](int buf, int i0, int i1) {          // window items [i0, i1) of the staged chunk -> buffer `buf`
#pragma unroll
    for (int it = i0; it < i1; ++it) {
      float* dl = (float*)((char*)lds + (it + 1 < NITA ? xlds0 : xldsl)) + buf * CHUNK + (it + 1 < NITA ? 64 * it : 0);
      dl[0] = xs[it].x; dl[PLANE] = xs[it].y; dl[2 * PLANE] = xs[it].z; dl[3 * PLANE] = xs[it].w;
    }
  };
  struct Raw { f32x2 a01, a23, a45, b01, b23, b45; };
  auto read_raw = [&](Raw& r, int buf, int ks, int t) {
    const int off = (buf * CHUNK + ks * GP + 2 * t * LC) * 4;
    r.a01 = *(const f32x2*)((const char*)lds + pa0 + off); r.a23 = *(const f32x2*)((const char*)lds + pa1 + off);
    r.a45 = *(const f32x2*)((const char*)lds + pa2 + off);
    r.b01 = *(const f32x2*)((const char*)lds + pb0 + off); r.b23 = *(const f32x2*)((const char*)lds + pb1 + off);
    r.b45 = *(const f32x2*)((const char*)lds + pb2 + off);
  };
  // one tile row of one k-step: 9 packed vector instructions, 6 MT MFMAs.  FIRST: the first k-step of a tile starts the sums
  auto tile_row = [&](const Frag& wf, const Raw& r, int t, auto firstc) {
    constexpr bool FIRST = decltype(firstc)::value;
    const f32x2 t01 = __builtin_elementwise_fma(sgn2, r.b01, r.a01), t23 = __builtin_elementwise_fma(sgn2, r.b23, r.a23),
                t45 = __builtin_elementwise_fma(sgn2, r.b45, r.a45);
    f32x2 v05 = __builtin_elementwise_fma(k4, t01, __builtin_elementwise_fma(k5, t23, t45));
    const f32x2 ac = __builtin_elementwise_fma(__builtin_shufflevector(t23, t23, 0, 0), k41, __builtin_shufflevector(t45, t45, 0, 0));
    const f32x2 be = __builtin_elementwise_fma(__builtin_shufflevector(t01, t01, 1, 1), k41, __builtin_shufflevector(t23, t23, 1, 1));
    f32x2 v12 = __builtin_elementwise_fma(__builtin_shufflevector(be, be, 0, 0), kpm, __builtin_shufflevector(ac, ac, 0, 0));
    f32x2 v34 = __builtin_elementwise_fma(__builtin_shufflevector(be, be, 1, 1), kpm2, __builtin_shufflevector(ac, ac, 1, 1));
    if (WINO24_EXP & 4) { v05 = r.a01; v12 = r.a23; v34 = r.b45; }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[0][mt][t] = mfma16(wf.lo[mt].x, v05.x, FIRST ? zero : acc[0][mt][t]);
      acc[1][mt][t] = mfma16(wf.lo[mt].y, v12.x, FIRST ? cb[mt] : acc[1][mt][t]);
      acc[2][mt][t] = mfma16(wf.lo[mt].z, v12.y, FIRST ? zero : acc[2][mt][t]);
      acc[3][mt][t] = mfma16(wf.lo[mt].w, v34.x, FIRST ? zero : acc[3][mt][t]);
      acc[4][mt][t] = mfma16(wf.hi[mt].x, v34.y, FIRST ? zero : acc[4][mt][t]);
      acc[5][mt][t] = mfma16(wf.hi[mt].y, v05.y, FIRST ? zero : acc[5][mt][t]);
    }
  };
  // one k-step (4 input channels): the raw rows of the NEXT tile row (or of the next k-step's first) are requested before the
  // MFMAs of the current one.  FILL: the staged chunk c+1 goes to the other buffer between the tile rows, then chunk c+2 is requested.
  auto kstep = [&](const Frag& wf, Raw& r, int buf, int ks, bool fill, int next_ch, auto firstc) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      Raw nx;
      const bool more = t + 1 < NT || ks + 1 < KS;
      if (more && !(WINO24_EXP & 256)) read_raw(nx, buf, t + 1 < NT ? ks : ks + 1, t + 1 < NT ? t + 1 : 0);
      __builtin_amdgcn_sched_barrier(0);
      tile_row(wf, r, t, firstc);
      if (fill && !(WINO24_EXP & (8 | 64))) store_items(buf ^ 1, t * NITA / NT, (t + 1) * NITA / NT);
      __builtin_amdgcn_sched_barrier(0);
      if (more && !(WINO24_EXP & 256)) r = nx;
    }
    if (fill && !(WINO24_EXP & (8 | 128))) load_x(next_ch);
  };
  const int last_ks = NC * KS - 1;
  static_assert(KS == 4, "four k-steps per chunk, one per fragment set");
  auto chunk = [&](int c, auto curc, auto firstc, bool fill, int next_ch) {
    constexpr int CUR = decltype(curc)::value;
    Raw r;
    read_raw(r, CUR, 0, 0);
    if constexpr (WPS == 2) {                                // two sets, one k-step ahead
      kstep(wf0, r, CUR, 0, fill, next_ch, firstc);
      load_w(wf0, min(c * KS + 2, last_ks));
      kstep(wf1, r, CUR, 1, false, 0, std::false_type{});
      load_w(wf1, min(c * KS + 3, last_ks));
      kstep(wf0, r, CUR, 2, false, 0, std::false_type{});
      load_w(wf0, min(c * KS + 4, last_ks));
      kstep(wf1, r, CUR, 3, false, 0, std::false_type{});
      load_w(wf1, min(c * KS + 5, last_ks));
      if (!(WINO24_EXP & (8 | 32))) __syncthreads();
      return;
    }
    load_w(wf3, min(c * KS + 3, last_ks));
    kstep(wf0, r, CUR, 0, fill, next_ch, firstc);
    load_w(wf0, min(c * KS + 4, last_ks));
    kstep(wf1, r, CUR, 1, false, 0, std::false_type{});
    load_w(wf1, min(c * KS + 5, last_ks));
    kstep(wf2, r, CUR, 2, false, 0, std::false_type{});
    load_w(wf2, min(c * KS + 6, last_ks));
    kstep(wf3, r, CUR, 3, false, 0, std::false_type{});
    if (!(WINO24_EXP & (8 | 32))) __syncthreads();
  };

  // ---- tile loop (persistent grid, as k_conv_wino)
  // Workgroups i, i + 8, ... share an XCD and its L2 (cdna_hip_programming.md T1): give them NEIGHBOURING tiles of every sweep
  // -- the channel groups of a pixel block and the blocks above and below it, which read the same window -- instead of every
  // eighth one.  (Strided, the three groups of a block met in three different L2s: 2 FETCH + WRITE = 9 x the layer's input.)
  const int nwg = (int)gridDim.x, xq = nwg / 8, xr = nwg % 8, xcd = (int)blockIdx.x % 8;
  int tile = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (int)blockIdx.x / 8;
  Tile cur = decode(tile);
  window_of(cur);
  cg = cur.cg;
  load_x(0);
  load_w(wf0, 0);
  load_w(wf1, min(1, last_ks));
  if (WPS == 1) load_w(wf2, min(2, last_ks));
  wait_vmem_all();
  while (true) {
    const int next = tile + (int)gridDim.x;
    const bool more = next < tg.ntiles;
    store_items(0, 0, NITA);
    load_x(KC);
    __syncthreads();
    read_bias();
    chunk(0, std::integral_constant<int, 0>{}, std::true_type{}, true, 2 * KC);
    chunk(1, std::integral_constant<int, 1>{}, std::false_type{}, true, 3 * KC);
    for (int c = 2; c < NC - 2; c += 2) {                    // NC is even (>= 4) for every supported D
      chunk(c, std::integral_constant<int, 0>{}, std::false_type{}, true, (c + 2) * KC);
      chunk(c + 1, std::integral_constant<int, 1>{}, std::false_type{}, true, (c + 3) * KC);
    }
    const Tile done = cur;
    if (more) {
      cur = decode(next);
      window_of(cur);
    }
    chunk(NC - 2, std::integral_constant<int, 0>{}, std::false_type{}, true, 0);
    chunk(NC - 1, std::integral_constant<int, 1>{}, std::false_type{}, false, 0);
#pragma unroll
    for (int j = 0; j < 6; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) drain(acc[j][mt][0]);   // (tile row 0 is read first; tools/mfma_hazard_lint.py checks the rest)

    cg = cur.cg;
    // the next tile's first fragment sets fly during the epilogue
    if (more) {
      load_w(wf0, 0);
      load_w(wf1, min(1, last_ks));
      if (WPS == 1) load_w(wf2, min(2, last_ks));
    }
    // ---- epilogue of `done`: the four rows meet through LDS, one tile row per round
    if (!((WINO24_EXP & 1) && a.relu != 12345)) {
      const long img = (long)done.n * a.h * a.w * (long)D * 4;
      const buf_rsrc ro = make_rsrc((char*)a.out + img);
      const buf_rsrc rk = make_rsrc((const char*)(a.skip ? a.skip : a.out) + img);
      f32x4* zl = (f32x4*)lds;
      // SM: the tile's plane line (uniform: scalar loads) and the partials' descriptor, as in k_conv_wino
      const int sm_b = SM ? done.n % a.sm_B : 0, sm_last = a.sm_D - 1, dq = 4 * q;
      const float sm_lo = SM ? a.sm_planes.p[2 * sm_b] : 0.f, sm_hi = SM ? a.sm_planes.p[2 * sm_b + 1] : 0.f;
      const float sm_step = (sm_hi - sm_lo) / (float)sm_last;   // as planes.h::plane_line
      const buf_rsrc rp = make_rsrc((char*)a.sm_part + (size_t)done.n * a.h * a.w * (size_t)(64 * groups));      // 4 partials of 16 bytes per channel group
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        if (t) __syncthreads();                                // the previous round's readers are done
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const f32x4 s12 = acc[1][mt][t] + acc[2][mt][t], d12 = acc[1][mt][t] - acc[2][mt][t];
          const f32x4 s34 = acc[3][mt][t] + acc[4][mt][t], d34 = acc[3][mt][t] - acc[4][mt][t];
          zl[((wave * 4 + 0) * MT + mt) * 64 + lane] = (acc[0][mt][t] + s12) + s34;
          zl[((wave * 4 + 1) * MT + mt) * 64 + lane] = d12 + 2.0f * d34;
          zl[((wave * 4 + 2) * MT + mt) * 64 + lane] = s12 + 4.0f * s34;
          zl[((wave * 4 + 3) * MT + mt) * 64 + lane] = (d12 + 8.0f * d34) + acc[5][mt][t];
        }
        __syncthreads();
        const int oy = done.r0 + 2 * (NT * fr + t) + oa, ox = done.c0 + 4 * ft + 2 * ob;
        const unsigned tbase = ooff + (unsigned)((((done.r0 + 2 * t) * a.w + done.c0) * D + done.cg * MT * 16) * 4);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          if constexpr (SM) {
            // the softmax partial of the lane's 16 channels of pixel (oy, ox + bb): k_conv_wino's, one 16-byte store per lane, pixel
            // and round, always issued (out-of-image pixels: BUF_OOB) so that the wait below counts right
            float m = -INFINITY, se = 0.f, sd = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
              const f32x4 z0 = zl[(((oa + 0) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
              const f32x4 z1 = zl[(((oa + 1) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
              const f32x4 z2 = zl[(((oa + 2) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
              const f32x4 v = z0 + os * (z1 + z2);
              const float mn = fmaxf(m, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
              const float sc = __expf(m - mn);                   // (first tile: exp(-inf) = 0 times 0)
              const int d = (done.cg * MT + mt) * 16 + dq;
              const float e0 = __expf(v.x - mn), e1 = __expf(v.y - mn), e2 = __expf(v.z - mn), e3 = __expf(v.w - mn);
              se = __fmaf_rn(se, sc, (e0 + e1) + (e2 + e3));
              sd = sd * sc;
              sd = __fmaf_rn(e3, plane_value(sm_lo, sm_step, min(d + 3, sm_last)), __fmaf_rn(e2, plane_value(sm_lo, sm_step, min(d + 2, sm_last)),
                   __fmaf_rn(e1, plane_value(sm_lo, sm_step, min(d + 1, sm_last)), __fmaf_rn(e0, plane_value(sm_lo, sm_step, min(d, sm_last)), sd))));
              m = mn;
            }
            const unsigned pbase = (oy < a.h && ox + bb < a.w) ? (unsigned)(((oy * a.w + ox + bb) * (4 * groups) + done.cg * 4 + q) * 16) : BUF_OOB;
            buf_store4(rp, pbase, f32x4{m, se, sd, 0.f});
            continue;
          }
          const unsigned obase = (oy < a.h && ox + bb < a.w) ? tbase + (unsigned)(bb * D * 4) : BUF_OOB;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            const f32x4 z0 = zl[(((oa + 0) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
            const f32x4 z1 = zl[(((oa + 1) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
            const f32x4 z2 = zl[(((oa + 2) * 4 + 2 * ob + bb) * MT + mt) * 64 + lane];
            f32x4 v = z0 + os * (z1 + z2);
            if (a.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            if (a.skip) v += buf_load4(rk, obase == BUF_OOB ? BUF_OOB : obase + mt * 64);
            buf_store4(ro, obase == BUF_OOB ? BUF_OOB : obase + mt * 64, v);
          }
        }
      }
    }
    if (!more) break;
    tile = next;
    // the window chunk and the fragments were requested BEFORE the epilogue's 2 NT MT stores (vmcnt retires in order)
    wait_vmem_but<SM ? 2 * NT : 2 * NT * MT>();
    __syncthreads();                                         // the epilogue's LDS readers are done: the buffers are free
  }
}

template <int MT, int NT, int WPS, bool SM = false, int FOLD = 1>
static int launch_wino24_cfg(const WinoArgs& a, int N, hipStream_t st) {
  using G = Wino24Geom<MT, NT, FOLD>;
  const int groups = a.D / (16 * MT);
  TileGrid tg;
  if (int rc = make_tile_grid(tg, groups * cdiv(a.w, G::BW), cdiv(a.h, G::BH), N)) return rc;
  return launch_resident<k_conv_wino24<MT, NT, WPS, SM, FOLD>>(tg.ntiles, G::LDS_BYTES, st, "conv_wino24", a, tg, groups,
                                                               (unsigned)(((1ull << 32) + groups - 1) / groups));
}

// Three tilings, the same bits.  Two workgroups per CU leave a wave 24 accumulator tiles: MT 2 x NT 2 (a fragment feeds two MFMAs, six
// channel groups per pixel block at D = 192) or MT 4 x NT 1 (one MFMA per fragment, a 4-row window per 2 output rows); one workgroup
// per CU holds MT 4 x NT 2.  256 maps of 96 x 192 at D = 192: 10.92 / 11.01 / 11.13 ms (F(2x2, 3x3): 11.73); 64 maps 2.62 / 2.79 / 2.81
// (2.89); 32 maps at D = 256 2.29 / 2.37 / 2.43 (2.50): MT 2 x NT 2 wherever the epilogue allows it (the softmax partials need MT 4).
// Option wino_wps = 1 / 2 forces the one-workgroup form / MT 4 x NT 1 (A/B).
//
// Folded blocks (Wino24Geom): FOLD 2 with MT 2 x NT 2 covers 8 x 32 pixels, FOLD 4 with MT 4 x NT 1 covers 8 x 16 -- the widths 96 and
// 48 of the inner hourglass levels tile exactly, where the 64-pixel blocks pad a quarter.  Per pixel the same sums in the same order:
// every form gives the same bits.  conv_wino24_fold: the FOLD a map takes.  blocks = -1 (what every caller but the A/B entry point
// passes): a folded form where the unfolded blocks would pad the width and the folded ones tile the map in both directions; 2 / 4: that
// FOLD wherever the width is a multiple of its block's (adamvs_conv3x3_dd_wino24_blocks: A/B, tests, any height); 1: the 64-pixel
// blocks.  A forced wino_wps keeps the unfolded blocks.
int conv_wino24_fold(int h, int w, int blocks) {
  if (opt(OPT_WINO_WPS) == 1 || opt(OPT_WINO_WPS) == 2) return 1;
  if (blocks == 2 || blocks == 4) return w % (64 / blocks) == 0 ? blocks : 1;
  if (blocks != -1 || w % 64 == 0 || h % 8 != 0) return 1;
  return w % 32 == 0 ? 2 : (w % 16 == 0 ? 4 : 1);
}

int launch_conv_wino24(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D, int h, int w,
                       int relu, hipStream_t st, int blocks) {
  const WinoArgs a{in, wpk, bias, skip, out, D, h, w, relu, nullptr, PlaneSrc{nullptr, 0, 0.f}, 1, D};
  ADAMVS_CHECK_ARG(wino_depth_supported(D), "conv_wino24: D=%d unsupported (a multiple of 64 up to 512)", D);
  ADAMVS_CHECK_ARG((size_t)h * w * D * 4 < 0x7fffffffu, "conv_wino24: a map of %dx%dx%d floats exceeds the 2 GiB a buffer descriptor spans", h, w, D);
  switch (conv_wino24_fold(h, w, blocks)) {
    case 2: return launch_wino24_cfg<2, 2, 2, false, 2>(a, N, st);
    case 4: return launch_wino24_cfg<4, 1, 2, false, 4>(a, N, st);
    default: break;
  }
  switch (opt(OPT_WINO_WPS)) {
    case 1: return launch_wino24_cfg<4, 2, 1>(a, N, st);
    case 2: return launch_wino24_cfg<4, 1, 2>(a, N, st);
    default: return launch_wino24_cfg<2, 2, 2>(a, N, st);
  }
}

// `prob` in this form with the softmax partials behind it: launch_conv_wino_softmax's arguments and partial layout
int launch_conv_wino24_softmax(const float* in, const float* wpk, const float* bias, float* part, const PlaneSrc& planes, float* vw, float* pd,
                               int N, int B, int D, int n_planes, int h, int w, hipStream_t st) {
  const WinoArgs a{in, wpk, bias, nullptr, nullptr, D, h, w, 0, part, planes, B, n_planes > 0 ? n_planes : D};
  ADAMVS_CHECK_ARG(planes.mode == PLANES_UNIFORM && a.sm_D > 1, "conv_wino24_softmax: planes uniform per tile, at least two (mode %d, %d planes)", planes.mode, a.sm_D);
  ADAMVS_CHECK_ARG(wino_depth_supported(D), "conv_wino24_softmax: D=%d unsupported (a multiple of 64 up to 512)", D);
  ADAMVS_CHECK_ARG((size_t)h * w * D * 4 < 0x7fffffffu, "conv_wino24_softmax: a map of %dx%dx%d floats exceeds the 2 GiB a buffer descriptor spans", h, w, D);
  if (int rc = opt(OPT_WINO_WPS) == 1 ? launch_wino24_cfg<4, 2, 1, true>(a, N, st) : launch_wino24_cfg<4, 1, 2, true>(a, N, st)) return rc;
  return launch_softmax_merge(part, vw, pd, (size_t)N * h * w, D / 16, st);
}

}  // namespace adamvs

using namespace adamvs;

extern "C" int adamvs_conv3x3_dd_wino24(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N,
                                        int D, int h, int w, int relu, void* stream) {
  ADAMVS_CHECK_ARG(in && wpk && bias && out && N > 0 && h > 0 && w > 0, "conv3x3_dd_wino24: bad arguments");
  return launch_conv_wino24(in, wpk, bias, skip, out, N, D, h, w, relu, (hipStream_t)stream);
}

extern "C" int adamvs_conv3x3_dd_wino24_blocks(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N,
                                               int D, int h, int w, int relu, int blocks, void* stream) {
  ADAMVS_CHECK_ARG(in && wpk && bias && out && N > 0 && h > 0 && w > 0, "conv3x3_dd_wino24_blocks: bad arguments");
  ADAMVS_CHECK_ARG(blocks == -1 || blocks == 1 || blocks == 2 || blocks == 4, "conv3x3_dd_wino24_blocks: blocks=%d (-1 by the map, 1, 2, 4)", blocks);
  return launch_conv_wino24(in, wpk, bias, skip, out, N, D, h, w, relu, (hipStream_t)stream, blocks);
}

extern "C" int adamvs_prob_softmax_regress_wino24(const float* in, const float* wpk, const float* bias, const float* depth_range, float* view_weight,
                                                  float* pair_depth, int S, int B, int D, int h, int w, void* workspace,
                                                  size_t workspace_bytes, void* stream) {
  ADAMVS_CHECK_ARG(in && wpk && bias && depth_range && view_weight && pair_depth && workspace && S > 0 && B > 0 && h > 0 && w > 0,
                   "prob_softmax_regress_wino24: bad arguments");
  ADAMVS_CHECK_ARG(wino_depth_supported(D) && D > 1, "prob_softmax_regress_wino24: D=%d unsupported (a multiple of 64 up to 512)", D);
  // the partials' layout is the F(2x2, 3x3) kernel's: the same workspace size
  ADAMVS_CHECK_ARG(workspace_bytes >= wino_softmax_part_floats(S * B, D, h, w) * sizeof(float),
                   "prob_softmax_regress_wino24: workspace too small (%zu < %zu bytes)", workspace_bytes,
                   wino_softmax_part_floats(S * B, D, h, w) * sizeof(float));
  return launch_conv_wino24_softmax(in, wpk, bias, (float*)workspace, PlaneSrc{depth_range, PLANES_UNIFORM, 0.f}, view_weight, pair_depth, S * B, B,
                                    D, D, h, w, (hipStream_t)stream);
}
