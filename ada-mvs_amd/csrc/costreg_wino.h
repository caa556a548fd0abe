// What the two minimal-filtering forms of a stride-1 CostRegNet2D layer share: F(2x2, 3x3) (costreg2d_wino.hip) and
// F(2x4, 3x3) (costreg2d_wino24.hip).
#pragma once

#include "planes.h"

namespace adamvs {

struct WinoArgs {
  const float* in;     // [N][h*w][D]
  const float* wpk;    // A fragments of U = G g Gt; the order is each kernel's (include/adamvs_hip.h)
  const float* bias;   // [D]
  const float* skip;   // [N][h*w][D] or null; added after the ReLU
  float* out;          // [N][h*w][D]
  int D, h, w, relu;
  // SM kernels (the `prob` layer under adamvs_depth_stage_forward): no `out`; every lane reduces the 16 scores it holds of a
  // pixel to (max, sum of exp, sum of exp * plane) and stores that partial, [N][h*w][D/16][4]; k_softmax_merge finishes
  float* sm_part;
  PlaneSrc sm_planes;
  int sm_B, sm_D;      // image n belongs to tile n % sm_B; sm_D hypothesis planes (<= D: pad channels score -1e30)
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// k_softmax_merge (costreg2d_wino.hip) over npix pixels of np = D / 16 partials each
int launch_softmax_merge(const float* part, float* vw, float* pd, size_t npix, int np, hipStream_t st);

}  // namespace adamvs
