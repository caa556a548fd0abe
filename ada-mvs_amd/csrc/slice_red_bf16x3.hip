// Split-bf16 ("bf16x3") versions of the small 3x3 convolutions of SliceCostRegNetRED
// (reference models/adamvs.py:400-424, models/module.py:5-52): conv1 (two-row form), the two ConvGRU gate /
// candidate convolutions and conv2.  Same persistent pipeline and fused epilogues as slice_red.hip; the
// channel contraction runs on v_mfma_f32_16x16x32_bf16 with every fp32 operand split into hi + lo bf16 halves
// (a.b ~ a_hi.b_hi + a_hi.b_lo + a_lo.b_hi, fp32 accumulation; see costreg2d_bf16x3.hip).
//
// The contraction index is flattened: k = pos * CIN + cin, pos = tap (ky,kx) -- or (input row rr, kx) for the
// two-row conv1 -- padded with zero weights to a multiple of 32.  A lane's k-group (8 consecutive k = 8 channels
// of ONE position, since CIN is a multiple of 8) is one 16-byte LDS read from a pixel-major tile
// [pixel][CIN + 8 pad] of bf16 (hi and lo images); the activations are split when the tile is written.
#include "common.h"
#include "kernels.h"
#include "persistent.h"
#include "slice_roles_bx3.h"

namespace adamvs {

template <int CA, int CB, int NT, int STRIDE, int EPI>
__global__ __launch_bounds__(256) void k_conv_small_bx3(SmallConvArgsBx a, TileGrid tg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  ConvSmallBx3Role<CA, CB, NT, STRIDE, EPI>::run(a, tg, TileRange{0, tg.ntiles}, blockIdx.x, gridDim.x, lds);
}

__global__ __launch_bounds__(256, 2) void k_gru1_fused_bx3(Gru1Args a, TileGrid tg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Gru1FusedBx3Role::run(a, tg, TileRange{0, tg.ntiles}, blockIdx.x, gridDim.x, lds);
}

template <int CA, int CB, int NT, int STRIDE, int EPI>
static int launch_bx(const SmallConvArgsBx& a, int N, hipStream_t st, const char* name) {
  constexpr int TR = (EPI == BXE_TWO_ROW) ? 8 : 4, TC = 16;
  constexpr int LR = (STRIDE == 1) ? TR + 2 : 2 * TR + 1;
  constexpr int LC = (STRIDE == 1) ? TC + 2 : 2 * TC + 1;
  constexpr size_t lds = (size_t)2 * LR * LC * bx_pixel_pitch(CA + CB) * sizeof(__bf16);
  static_assert(lds <= 64 * 1024, "tile exceeds the default dynamic LDS limit");
  TileGrid tg;
  if (int rc = make_tile_grid(tg, cdiv(a.wo, TC), cdiv(a.ho, TR), N)) return rc;
  return launch_resident<k_conv_small_bx3<CA, CB, NT, STRIDE, EPI>>(tg.ntiles, lds, st, name, a, tg);
}

int launch_conv1_bf16x3(const float* cost, const float* w, float* c1, int N, int C, int h, int w_, hipStream_t st) {
  SmallConvArgsBx a{cost, nullptr, (const bf16x8*)w, nullptr, c1, nullptr, nullptr, h, w_, h, w_, 8};
  if (C == 32) return launch_bx<32, 0, 1, 1, BXE_TWO_ROW>(a, N, st, "conv1 (bf16x3)");
  if (C == 16) return launch_bx<16, 0, 1, 1, BXE_TWO_ROW>(a, N, st, "conv1 (bf16x3)");
  if (C == 8) return launch_bx<8, 0, 1, 1, BXE_TWO_ROW>(a, N, st, "conv1 (bf16x3)");
  return set_error(-1, "conv1: C=%d unsupported (8, 16 or 32)", C);
}

__global__ __launch_bounds__(256, 2) void k_gru2_fused_bx3(Gru2Args a, TileGrid tg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  Gru2FusedBx3Role::run(a, tg, TileRange{0, tg.ntiles}, blockIdx.x, gridDim.x, lds);
}

static int launch_gru2_fused(const Gru2Args& a, int B, hipStream_t st) {
  TileGrid tg;
  if (int rc = make_tile_grid(tg, Gru2FusedBx3Role::tiles_x(a), Gru2FusedBx3Role::tiles_y(a), B)) return rc;
  return launch_resident<k_gru2_fused_bx3>(tg.ntiles, Gru2FusedBx3Role::LDS_BYTES, st, "gru2 fused (bf16x3)", a, tg);
}

static int launch_gru1_fused(const Gru1Args& a, int B, hipStream_t st) {
  constexpr size_t lds = (size_t)2 * 12 * 34 * 32 + 10 * 32 * 32;
  TileGrid tg;
  if (int rc = make_tile_grid(tg, cdiv(a.w, 30), cdiv(a.h, 8), B)) return rc;
  return launch_resident<k_gru1_fused_bx3>(tg.ntiles, lds, st, "gru1 fused (bf16x3)", a, tg);
}

// GRU level 1 (fused) / conv2 / GRU level 2 (fused) of one recurrent step (the decoder stays on the fp32 path).
// *h1_now, *h2_now receive the buffers that hold the states after the step.
int launch_gru_convs_bf16x3(const float* c1, const FuseWeights& fw, const StepBuffers& sb, int B, int h, int w, int d,
                            float** h1_now, float** h2_now, hipStream_t st) {
  const int h2 = h / 2, w2 = w / 2;
  int rc;
  // level 1 fused; its state alternates between the h1 and rh1 buffers (step d reads the one step d-1 wrote)
  float* hin = (d & 1) ? sb.rh1 : sb.h1;
  float* hout = (d & 1) ? sb.h1 : sb.rh1;
  {
    Gru1Args g{c1, hin, hout, (const bf16x8*)fw.gates1, fw.gates1_b, (const bf16x8*)fw.cand1, fw.cand1_b, h, w};
    if ((rc = launch_gru1_fused(g, B, st))) return rc;
  }
  *h1_now = hout;
  {
    SmallConvArgsBx a{hout, nullptr, (const bf16x8*)fw.conv2, nullptr, sb.c2, nullptr, nullptr, h, w, h2, w2, 16};
    if ((rc = launch_bx<8, 0, 1, 2, BXE_RELU>(a, B, st, "conv2 (bf16x3)"))) return rc;
  }
  {  // level 2 fused; its state alternates between the h2 and rh2 buffers like level 1's
    float* gin = (d & 1) ? sb.rh2 : sb.h2;
    float* gout = (d & 1) ? sb.h2 : sb.rh2;
    Gru2Args g{sb.c2, gin, gout, (const bf16x8*)fw.gates2, fw.gates2_b, (const bf16x8*)fw.cand2, fw.cand2_b, h2, w2};
    if ((rc = launch_gru2_fused(g, B, st))) return rc;
    *h2_now = gout;
  }
  return 0;
}

}  // namespace adamvs
