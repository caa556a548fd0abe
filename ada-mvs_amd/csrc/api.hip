// C-ABI glue: error plumbing, the one-step op and the whole-stage driver
// (InferDepthNet0.forward, reference models/adamvs.py:433-533).
#include <stdarg.h>
#include <string.h>

#include <atomic>
#include <mutex>

#include "../../include/adamvs_hip.h"
#include "common.h"
#include "kernels.h"
#include "lod2_plane.h"

namespace adamvs {

thread_local char g_last_error[512] = "";

int set_error(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
  va_end(ap);
  return code;
}

static_assert(sizeof(FuseWeights) == sizeof(adamvs_fuse_weights), "adamvs_fuse_weights layout");

// ---- run-time options (options.h; documented in include/adamvs_hip.h "OPTIONS")
struct OptionEntry { const char* name; int def; };
static const OptionEntry g_option_table[OPT_COUNT] = {
#define ADAMVS_OPTION_ROW(e, n, d) {n, d},
    ADAMVS_OPTION_LIST(ADAMVS_OPTION_ROW)
#undef ADAMVS_OPTION_ROW
};
static std::atomic<int> g_option_value[OPT_COUNT];
static std::once_flag g_option_once;
// defaults, then ADAMVS_<NAME> from the environment: the library's one read of the process environment besides the two cost
// tables of recurrence.hip (tuning), made once
static void option_init() {
  std::call_once(g_option_once, [] {
    for (int i = 0; i < OPT_COUNT; ++i) {
      int v = g_option_table[i].def;
      char key[64] = "ADAMVS_";
      size_t n = strlen(key);
      for (const char* c = g_option_table[i].name; *c && n + 1 < sizeof(key); ++c) key[n++] = (*c >= 'a' && *c <= 'z') ? (char)(*c - 32) : *c;
      key[n] = 0;
      if (const char* e = getenv(key))
        if (*e) v = atoi(e);
      g_option_value[i].store(v, std::memory_order_relaxed);
    }
  });
}
int opt(Option o) {
  option_init();
  return g_option_value[o].load(std::memory_order_relaxed);
}
static int option_index(const char* name) {
  if (!name) return -1;
  for (int i = 0; i < OPT_COUNT; ++i)
    if (!strcmp(name, g_option_table[i].name)) return i;
  return -1;
}

static size_t align_up(size_t n) { return (n + 63) & ~(size_t)63; }   // in floats: 256-byte slots

// Zero fills and device-to-device copies are KERNELS here, not the runtime's asynchronous memset / memcpy calls.  Inside a captured
// hipGraph those become memset / memcpy nodes, and on this stack (ROCm 7.x, gfx950) a memset node between kernel nodes was observed to
// run out of order with them: a replayed stage started its recurrence from the previous replay's states as soon as the kernels around
// the node were short (profiles/r06_graph_memset_node.txt: the same graph is bit-exact over 28 replays with the fill as a kernel and
// wrong from the second replay on with the memset call, whatever the kernel-argument placement).
__global__ __launch_bounds__(256) void k_fill_zero(float* __restrict__ p, size_t n) {
  const size_t n4 = n / 4, stride = (size_t)gridDim.x * 256, i0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (((size_t)p & 15) == 0)
    for (size_t i = i0; i < n4; i += stride) ((f32x4*)p)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  else
    for (size_t i = i0; i < n4 * 4; i += stride) p[i] = 0.f;
  if (i0 < n - n4 * 4) p[n4 * 4 + i0] = 0.f;
}
__global__ __launch_bounds__(256) void k_copy_floats(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
static unsigned fill_grid(size_t n) { return (unsigned)(n / 1024 + 1 < 2048 ? n / 1024 + 1 : 2048); }
hipError_t zero_floats(float* p, size_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_fill_zero, dim3(fill_grid(n)), dim3(256), 0, st, p, n);
  return hipGetLastError();
}
hipError_t copy_floats(const float* src, float* dst, size_t n, hipStream_t st) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(k_copy_floats, dim3(fill_grid(n)), dim3(256), 0, st, src, dst, n);
  return hipGetLastError();
}

// Workspace of one stage.  The hypothesis axis is processed in chunks of DC = sweep_chunk_planes(D) planes (aggregation
// -> conv1 -> recurrence -> soft-argmin accumulation per chunk, reference models/adamvs.py:495-531 runs the same
// chain per plane), so nothing below grows with D except the stage-1 similarity / score volumes, whose hypothesis axis
// is CostRegNet2D's channel axis (models/adamvs.py:464-486).
struct StageCarve {
  size_t c1, h1[4], rh1, u1, c2[2], h2[2], rh2, u2, vol[2], acc, agg, sim, score, creg, total;   // offsets in floats
  int dc;
};

// the width CostRegNet2D runs at for the stage's D hypotheses (kernels.h::costreg_width; 0: none)
static int stage_reg_width(const adamvs_stage_desc& s) {
  return s.precision == PRECISION_BF16X3 ? costreg_width_bf16x3(s.D) : costreg_width(s.D);
}

static StageCarve carve(const adamvs_stage_desc& s) {
  StageCarve c;
  size_t hw = (size_t)s.h * s.w, hw4 = (size_t)(s.h / 2) * (s.w / 2);
  size_t HW = s.in_up ? 4 * hw : hw;
  size_t o = 0;
  auto take = [&](size_t n) { size_t r = o; o += align_up(n); return r; };
  c.dc = sweep_chunk_planes(s.D);
  c.c1 = take((size_t)c.dc * s.B * hw * 8);
  for (int i = 0; i < 4; ++i) c.h1[i] = take((size_t)s.B * hw * 8);
  c.rh1 = take((size_t)s.B * hw * 8);
  c.u1 = take((size_t)s.B * hw * 8);
  for (int i = 0; i < 2; ++i) c.c2[i] = take((size_t)s.B * hw4 * 16);
  for (int i = 0; i < 2; ++i) c.h2[i] = take((size_t)s.B * hw4 * 16);
  c.rh2 = take((size_t)s.B * hw4 * 16);
  c.u2 = take((size_t)s.B * hw4 * 16);
  for (int i = 0; i < 2; ++i) c.vol[i] = take((size_t)s.B * c.dc * HW);      // the decoder runs two or three hypotheses behind level 1
  c.acc = take(3 * (size_t)s.B * HW);
  c.agg = take(sweep_workspace_floats(s.B, s.C, s.D, s.h, s.w));
  c.sim = c.score = c.creg = o;
  if (s.first_stage) {
    // the similarity / score volumes and CostRegNet2D's activations at the width the network runs at (>= D)
    size_t F = (size_t)s.S * s.B * hw * stage_reg_width(s);
    c.sim = take(F);
    c.score = take(F);
    c.creg = take(3 * F);
  }
  c.total = o;
  return c;
}

static int check_desc(const adamvs_stage_desc* d) {
  ADAMVS_CHECK_ARG(d, "stage: null descriptor");
  ADAMVS_CHECK_ARG(d->B > 0 && d->S > 0 && d->D > 1 && d->h > 1 && d->w > 1, "stage: bad shape (B=%d S=%d D=%d h=%d w=%d)",
                   d->B, d->S, d->D, d->h, d->w);
  ADAMVS_CHECK_ARG(d->C == 8 || d->C == 16 || d->C == 32, "stage: C=%d unsupported (8, 16 or 32)", d->C);
  ADAMVS_CHECK_ARG((d->h % 2) == 0 && (d->w % 2) == 0, "stage: h=%d w=%d must be even", d->h, d->w);
  ADAMVS_CHECK_ARG(d->B <= 65535, "stage: B=%d tiles per call (at most 65535)", d->B);
  ADAMVS_CHECK_ARG(d->precision == PRECISION_FP32 || d->precision == PRECISION_BF16X3, "stage: precision=%d (0 fp32, 1 bf16x3)", d->precision);
  ADAMVS_CHECK_ARG(d->eps_in_numerator == 0 || d->eps_in_numerator == 1, "stage: eps_in_numerator=%d (0 or 1)", d->eps_in_numerator);
  ADAMVS_CHECK_ARG(d->plane_mode >= PLANES_EXPLICIT && d->plane_mode <= PLANES_WINDOW, "stage: plane_mode=%d (0 explicit, 1 uniform, 2 window)", d->plane_mode);
  ADAMVS_CHECK_ARG(d->precision_fuse == PRECISION_FP32 || d->precision_fuse == PRECISION_BF16X3,
                   "stage: precision_fuse=%d (0 fp32, 1 bf16x3)", d->precision_fuse);
  if (d->first_stage) {
    ADAMVS_CHECK_ARG(stage_reg_width(*d) > 0, "stage: D=%d hypotheses: CostRegNet2D runs at widths up to 512", d->D);
    ADAMVS_CHECK_ARG((d->h % 8) == 0 && (d->w % 8) == 0, "stage: first stage needs h=%d w=%d multiples of 8", d->h, d->w);
  } else {
    ADAMVS_CHECK_ARG(d->prev_h > 0 && d->prev_w > 0, "stage: prev_h/prev_w missing");
  }
  return 0;
}

}  // namespace adamvs

using namespace adamvs;

extern "C" int adamvs_version(void) { return ADAMVS_ABI_VERSION; }

extern "C" int adamvs_option_count(void) { return OPT_COUNT; }
extern "C" const char* adamvs_option_name(int index) { return index >= 0 && index < OPT_COUNT ? g_option_table[index].name : nullptr; }
extern "C" int adamvs_option_default(const char* name, int* value) {
  const int i = option_index(name);
  ADAMVS_CHECK_ARG(i >= 0 && value, "option_default: unknown option '%s' (include/adamvs_hip.h, OPTIONS)", name ? name : "(null)");
  *value = g_option_table[i].def;
  return 0;
}
extern "C" int adamvs_get_option(const char* name, int* value) {
  const int i = option_index(name);
  ADAMVS_CHECK_ARG(i >= 0 && value, "get_option: unknown option '%s' (include/adamvs_hip.h, OPTIONS)", name ? name : "(null)");
  *value = opt((Option)i);
  return 0;
}
extern "C" int adamvs_set_option(const char* name, int value) {
  const int i = option_index(name);
  ADAMVS_CHECK_ARG(i >= 0, "set_option: unknown option '%s' (include/adamvs_hip.h, OPTIONS)", name ? name : "(null)");
  option_init();
  g_option_value[i].store(value, std::memory_order_relaxed);
  return 0;
}
extern "C" const char* adamvs_last_error_string(void) { return g_last_error; }

extern "C" size_t adamvs_slice_reg_step_scratch_bytes(int B, int h, int w) {
  size_t hw = (size_t)h * w, hw4 = (size_t)(h / 2) * (w / 2);
  return (3 * align_up((size_t)B * hw * 8) + 3 * align_up((size_t)B * hw4 * 16)) * sizeof(float);
}

extern "C" int adamvs_slice_reg_step(const float* cost, float* state1, float* state2, const adamvs_fuse_weights* weights,
                                     float* reg_cost, int B, int C, int h, int w, int in_up, int precision, void* scratch,
                                     size_t scratch_bytes, void* stream) {
  ADAMVS_CHECK_ARG(precision == PRECISION_FP32 || precision == PRECISION_BF16X3, "slice_reg_step: precision=%d (0 fp32, 1 bf16x3)", precision);
  ADAMVS_CHECK_ARG(cost && state1 && state2 && weights && reg_cost && scratch, "slice_reg_step: null pointer");
  ADAMVS_CHECK_ARG(B > 0 && h > 1 && w > 1 && (h % 2) == 0 && (w % 2) == 0, "slice_reg_step: bad shape (B=%d h=%d w=%d, even sizes)", B, h, w);
  ADAMVS_CHECK_ARG(C == 8 || C == 16 || C == 32, "slice_reg_step: C=%d unsupported (8, 16 or 32)", C);
  ADAMVS_CHECK_ARG(scratch_bytes >= adamvs_slice_reg_step_scratch_bytes(B, h, w), "slice_reg_step: scratch too small");
  hipStream_t st = (hipStream_t)stream;
  size_t n1 = align_up((size_t)B * h * w * 8), n2 = align_up((size_t)B * (h / 2) * (w / 2) * 16);
  float* s = (float*)scratch;
  float* c1 = s;
  StepBuffers sb{state1, s + n1, s + 2 * n1, s + 3 * n1, state2, s + 3 * n1 + n2, s + 3 * n1 + 2 * n2};
  FuseWeights fw;
  memcpy(&fw, weights, sizeof(fw));
  int rc = launch_conv1(cost, fw.conv1, c1, B, C, h, w, precision, st);
  if (rc) return rc;
  float* h1_now = state1;
  float* h2_now = state2;
  if ((rc = launch_slice_step(c1, fw, sb, reg_cost, B, h, w, 1, 0, in_up, precision, st, &h1_now, &h2_now))) return rc;
  if (h1_now != state1) {              // the split-bf16 GRU kernels write the new state to the other buffer
    hipError_t e = copy_floats(h1_now, state1, (size_t)B * h * w * 8, st);
    if (e != hipSuccess) return set_error((int)e, "slice_reg_step: state copy: %s", hipGetErrorString(e));
  }
  if (h2_now != state2) {
    hipError_t e = copy_floats(h2_now, state2, (size_t)B * (h / 2) * (w / 2) * 16, st);
    if (e != hipSuccess) return set_error((int)e, "slice_reg_step: state copy: %s", hipGetErrorString(e));
  }
  return 0;
}

extern "C" int adamvs_recurrence_schedule(int precision_fuse, long long pixels) { return recurrence_mode(precision_fuse, (long)pixels); }
extern "C" int adamvs_gru_wino_mask(void) { return gru_wino_mask(); }

extern "C" size_t adamvs_depth_stage_workspace_bytes(const adamvs_stage_desc* desc) {
  if (check_desc(desc)) return 0;
  return carve(*desc).total * sizeof(float);
}

static int stage_forward(const adamvs_stage_desc* desc, const float* feat, const float* rt, const float* planes,
                         const float* prev_conf, const float* w_reg, size_t w_reg_floats, const adamvs_fuse_weights* w_fuse,
                         float* view_weight, float* pair_depth, float* depth, float* confidence, int phases, void* workspace,
                         size_t workspace_bytes, void* stream, bool timing_only) {
  int rc = check_desc(desc);
  if (rc) return rc;
  ADAMVS_CHECK_ARG(phases >= 0 && phases <= ADAMVS_PHASE_ALL, "stage: phases=%d (a subset of ADAMVS_PHASE_ALL = 15)", phases);
  const adamvs_stage_desc& s = *desc;
  ADAMVS_CHECK_ARG(feat && rt && planes && w_fuse && view_weight && depth && confidence && workspace, "stage: null pointer");
  ADAMVS_CHECK_ARG(!s.first_stage || (w_reg && pair_depth), "stage: first stage needs w_reg and pair_depth");
  ADAMVS_CHECK_ARG(!s.first_stage || w_reg_floats == cost_reg_weight_floats(stage_reg_width(s), s.precision),
                   "stage: w_reg holds %zu floats; D=%d hypotheses run at width %d, whose layout has %zu (include/adamvs_hip.h)",
                   w_reg_floats, s.D, stage_reg_width(s), cost_reg_weight_floats(stage_reg_width(s), s.precision));
  ADAMVS_CHECK_ARG(s.first_stage || prev_conf, "stage: later stages need prev_conf");
  StageCarve c = carve(s);
  ADAMVS_CHECK_ARG(workspace_bytes >= c.total * sizeof(float), "stage: workspace too small (%zu < %zu bytes)", workspace_bytes,
                   c.total * sizeof(float));
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  FuseWeights fw;
  memcpy(&fw, w_fuse, sizeof(fw));
  const PlaneSrc ps{planes, s.plane_mode, s.half_span, s.plane_mode == PLANES_WINDOW ? s.half_span_dev : nullptr};

  // -- view weights: scored by CostRegNet2D (stage 1) or resampled from the previous stage
  if (!(phases & ADAMVS_PHASE_VIEW_WEIGHTS)) {
  } else if (s.first_stage) {
    // Dr >= D: the width CostRegNet2D runs at (w_reg is packed for it: adamvs_cost_reg_width); the pad channels of the
    // similarity volume are zeros, their scores -1e30, so the softmax sees D hypotheses
    const int Dr = stage_reg_width(s);
    if ((rc = launch_pair_similarity(feat, rt, ps, ws + c.sim, s.B, s.S, s.C, s.D, s.h, s.w, st, Dr))) return rc;
    if (cost_reg_softmax_fusable(Dr, s.precision, ps)) {       // softmax / max / regression in the epilogue of the last layer
      if ((rc = launch_cost_reg_net_2d(ws + c.sim, w_reg, ws + c.creg, ws + c.score, s.S * s.B, Dr, s.h, s.w, s.precision, st,
                                       view_weight, pair_depth, &ps, s.B, s.D)))
        return rc;
    } else {
      if ((rc = launch_cost_reg_net_2d(ws + c.sim, w_reg, ws + c.creg, ws + c.score, s.S * s.B, Dr, s.h, s.w, s.precision, st))) return rc;
      if ((rc = launch_softmax_regress(ws + c.score, ps, view_weight, pair_depth, s.S, s.B, Dr, s.h, s.w, st, s.D))) return rc;
    }
  } else {
    if ((rc = adamvs_resize_bilinear(prev_conf, view_weight, s.S * s.B, s.prev_h, s.prev_w, s.h, s.w, stream))) return rc;
  }

  // -- per chunk of hypotheses: weighted aggregation + conv1 (state-independent), the recurrence, soft-argmin accumulation.
  // With the three bits set they are interleaved chunk by chunk and the recurrence runs as a pipeline across chunk
  // boundaries.  The workspace holds ONE chunk of conv1 outputs and two of cost slices, so with more than one chunk a
  // proper subset of the three cannot hand its results to a later call: refused by adamvs_depth_stage_forward.  The measurement
  // entry point adamvs_bench_stage_phase (bench.py's phase-by-phase timing) runs the selected phase alone over all chunks on
  // whatever the buffers hold: its duration is the phase's, it promises no maps.
  const bool do_agg = phases & ADAMVS_PHASE_AGGREGATE, do_rec = phases & ADAMVS_PHASE_RECURRENCE, do_arg = phases & ADAMVS_PHASE_SOFT_ARGMIN;
  if (!do_agg && !do_rec && !do_arg) return 0;
  const size_t hw = (size_t)s.h * s.w, hw4 = (size_t)(s.h / 2) * (s.w / 2);
  const int dc = c.dc, nchunks = (s.D + dc - 1) / dc;
  ADAMVS_CHECK_ARG(nchunks == 1 || (do_agg && do_rec && do_arg) || timing_only,
                   "stage: phases=%d selects a proper subset of AGGREGATE|RECURRENCE|SOFT_ARGMIN, but D=%d runs in %d chunks of %d "
                   "hypotheses and the workspace keeps one: pass all three in one call (adamvs_bench_stage_phase times one "
                   "phase alone, no maps)", phases, s.D, nchunks, dc);
  const size_t c1_stride = (size_t)s.B * hw * 8;
  GruStateRing rb{{ws + c.h1[0], ws + c.h1[1], ws + c.h1[2], ws + c.h1[3]}, ws + c.rh1, ws + c.u1, {ws + c.c2[0], ws + c.c2[1]},
                  {ws + c.h2[0], ws + c.h2[1]}, ws + c.rh2, ws + c.u2};
  // schedule 0 with conv2 in the level-1 gate launch runs on the pipelined driver below as schedule 6 (lags {1, 1}, one role per
  // launch: launch_lagged_step); adamvs_recurrence_schedule keeps reporting 0 for it
  int mode = recurrence_mode(s.precision_fuse, (long)s.B * s.h * s.w);
  if (mode == 0 && conv2_in_gates1_applies(fw, s.h, s.w, s.precision_fuse)) mode = 6;
  const bool pipelined = mode != 0;
  const int lag = recurrence_lags(mode, s.precision_fuse).dec;       // the decoder runs `lag` hypotheses behind level 1
  if (do_rec) {      // zero initial states (adamvs.py:448-449): h1[-1] = ring slot 3, h2[-1] = ring slot 1 (slot 0 when sequential)
    hipError_t e = zero_floats(pipelined ? rb.h1[3] : rb.h1[0], (size_t)s.B * hw * 8, st);
    if (e == hipSuccess) e = zero_floats(pipelined ? rb.h2[1] : rb.h2[0], (size_t)s.B * hw4 * 16, st);
    if (e != hipSuccess) return set_error((int)e, "stage: zero initial states: %s", hipGetErrorString(e));
  }
  auto vol_of = [&](int d) { return ws + c.vol[(d / dc) & 1]; };
  auto argmin_chunk = [&](int k) {
    const int d0 = k * dc, nd = (d0 + dc < s.D ? d0 + dc : s.D) - d0;
    return launch_soft_argmin_chunk(ws + c.vol[k & 1], dc, ps, s.D, d0, nd, ws + c.acc, k == 0, k == nchunks - 1, depth, confidence,
                                    s.B, s.h, s.w, s.in_up, st);
  };
  StepBuffers sb{rb.h1[0], rb.rh1, rb.u1, rb.c2[0], rb.h2[0], rb.rh2, rb.u2};     // sequential mode: states updated in place
  for (int k = 0; k < nchunks; ++k) {
    const int d0 = k * dc, d1 = d0 + dc < s.D ? d0 + dc : s.D;
    if (do_agg && (rc = launch_sweep_conv1_chunk(feat, rt, ps, view_weight, fw.conv1, ws + c.c1, ws + c.agg, s.B, s.S, s.C, s.D, d0,
                                                 d1, s.h, s.w, s.precision_fuse, s.eps_in_numerator, st)))
      return rc;
    if (do_rec) {
      for (int t = d0; t < d1; ++t) {
        const float* c1_t = ws + c.c1 + (size_t)(t - d0) * c1_stride;
        if (pipelined) {
          // level 1 of hypothesis t, level 2 of t-1 (t-2), decoder of t-lag (which may belong to the previous chunk)
          const int sd = t - lag;
          if ((rc = launch_recur_pipeline_step(rb, fw, s.B, s.h, s.w, s.D, t, c1_t, sd >= 0 ? vol_of(sd) : nullptr, dc, sd >= 0 ? sd % dc : 0,
                                               s.in_up, s.precision_fuse, mode, st)))
            return rc;
          if (do_arg && sd >= 0 && sd % dc == dc - 1 && (rc = argmin_chunk(sd / dc))) return rc;   // a chunk of the volume is complete
        } else if ((rc = launch_slice_step(c1_t, fw, sb, vol_of(t), s.B, s.h, s.w, dc, t % dc, s.in_up, s.precision_fuse, st))) {
          return rc;
        }
      }
      if (!pipelined && do_arg && (rc = argmin_chunk(k))) return rc;
    } else if (do_arg && (rc = argmin_chunk(k))) {
      return rc;
    }
  }
  if (do_rec && pipelined) {
    for (int t = s.D; t < s.D + lag; ++t) {     // drain: the levels and decoders still behind
      const int sd = t - lag;
      if ((rc = launch_recur_pipeline_step(rb, fw, s.B, s.h, s.w, s.D, t, nullptr, sd >= 0 ? vol_of(sd) : nullptr, dc, sd >= 0 ? sd % dc : 0,
                                           s.in_up, s.precision_fuse, mode, st)))
        return rc;
      if (do_arg && sd >= 0 && sd % dc == dc - 1 && sd / dc < nchunks - 1 && (rc = argmin_chunk(sd / dc))) return rc;
    }
    if (do_arg && (rc = argmin_chunk(nchunks - 1))) return rc;
  }
  return 0;
}

extern "C" int adamvs_depth_stage_forward(const adamvs_stage_desc* desc, const float* feat, const float* rt,
                                          const float* planes, const float* prev_conf, const float* w_reg, size_t w_reg_floats,
                                          const adamvs_fuse_weights* w_fuse, float* view_weight, float* pair_depth,
                                          float* depth, float* confidence, int phases, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return stage_forward(desc, feat, rt, planes, prev_conf, w_reg, w_reg_floats, w_fuse, view_weight, pair_depth, depth, confidence,
                       phases, workspace, workspace_bytes, stream, false);
}

// MEASUREMENT ONLY (bench.py's phase table): the selected phases of a stage for their duration; depth / confidence are not valid
extern "C" int adamvs_bench_stage_phase(const adamvs_stage_desc* desc, const float* feat, const float* rt,
                                        const float* planes, const float* prev_conf, const float* w_reg, size_t w_reg_floats,
                                        const adamvs_fuse_weights* w_fuse, float* view_weight, float* pair_depth,
                                        float* depth, float* confidence, int phases, void* workspace,
                                        size_t workspace_bytes, void* stream) {
  return stage_forward(desc, feat, rt, planes, prev_conf, w_reg, w_reg_floats, w_fuse, view_weight, pair_depth, depth, confidence,
                       phases, workspace, workspace_bytes, stream, true);
}

// ---- depth-map fusion (fusion.hip): every argument is checked here, before any launch
extern "C" int adamvs_fusion_max_sources(void) { return ADAMVS_FUSION_MAX_SOURCES; }

static bool finite_f(float v) { return v == v && v <= 3.402823466e38f && v >= -3.402823466e38f; }

extern "C" int adamvs_geo_consistency(const float* ref_depth, const float* ref_conf, int H, int W, const adamvs_fusion_source* sources,
                                      int N, float prob_threshold, float pix_threshold, float rel_depth_threshold, int min_consistent,
                                      unsigned char* count, float* fused, unsigned* block_kept, void* stream) {
  ADAMVS_CHECK_ARG(ref_depth && ref_conf && sources && count && fused && block_kept, "geo_consistency: null pointer");
  ADAMVS_CHECK_ARG(H > 0 && W > 0 && (long)H * W < (1L << 31), "geo_consistency: bad reference size H=%d W=%d", H, W);
  ADAMVS_CHECK_ARG(N >= 1 && N <= ADAMVS_FUSION_MAX_SOURCES, "geo_consistency: N=%d sources (1 .. %d)", N, ADAMVS_FUSION_MAX_SOURCES);
  ADAMVS_CHECK_ARG(finite_f(prob_threshold), "geo_consistency: prob_threshold is not finite");
  ADAMVS_CHECK_ARG(finite_f(pix_threshold) && pix_threshold > 0.f, "geo_consistency: pix_threshold must be finite and > 0");
  ADAMVS_CHECK_ARG(finite_f(rel_depth_threshold) && rel_depth_threshold > 0.f, "geo_consistency: rel_depth_threshold must be finite and > 0");
  ADAMVS_CHECK_ARG(min_consistent >= 0, "geo_consistency: min_consistent=%d (>= 0)", min_consistent);
  for (int s = 0; s < N; ++s) {
    ADAMVS_CHECK_ARG(sources[s].depth, "geo_consistency: source %d: null depth pointer", s);
    ADAMVS_CHECK_ARG(sources[s].H > 0 && sources[s].W > 0 && (long)sources[s].H * sources[s].W < (1L << 31),
                     "geo_consistency: source %d: bad size H=%d W=%d", s, sources[s].H, sources[s].W);
    for (int k = 0; k < 12; ++k)
      ADAMVS_CHECK_ARG(finite_f(sources[s].fwd[k]) && finite_f(sources[s].back[k]), "geo_consistency: source %d: transform not finite", s);
  }
  return launch_geo_consistency(ref_depth, ref_conf, H, W, sources, N, prob_threshold, pix_threshold, rel_depth_threshold, min_consistent,
                                count, fused, block_kept, (hipStream_t)stream);
}

extern "C" int adamvs_fusion_scan(const unsigned* block_kept, unsigned* offsets, int nblocks, void* stream) {
  ADAMVS_CHECK_ARG(block_kept && offsets, "fusion_scan: null pointer");
  ADAMVS_CHECK_ARG(nblocks > 0, "fusion_scan: nblocks=%d (> 0)", nblocks);
  return launch_fusion_scan(block_kept, offsets, nblocks, (hipStream_t)stream);
}

extern "C" int adamvs_fusion_emit(const float* fused, const unsigned char* rgba, int H, int W, const double* camera, const unsigned* offsets,
                                  double* xyz, unsigned char* rgb, long capacity, void* stream) {
  ADAMVS_CHECK_ARG(fused && rgba && camera && offsets && xyz && rgb, "fusion_emit: null pointer");
  ADAMVS_CHECK_ARG(H > 0 && W > 0 && (long)H * W < (1L << 31), "fusion_emit: bad size H=%d W=%d", H, W);
  ADAMVS_CHECK_ARG(capacity >= (long)H * W, "fusion_emit: capacity %ld < H W = %ld points", capacity, (long)H * W);
  for (int k = 0; k < 21; ++k)
    ADAMVS_CHECK_ARG(std::isfinite(camera[k]), "fusion_emit: camera[%d] is not finite", k);
  return launch_fusion_emit(fused, rgba, H, W, camera, offsets, xyz, rgb, capacity, (hipStream_t)stream);
}

// ---- DSM (dsm.hip): every argument is checked here, before any launch
static int dsm_check_grid(const adamvs_dsm_grid* g, const char* what) {
  ADAMVS_CHECK_ARG(g, "%s: null grid", what);
  ADAMVS_CHECK_ARG(std::isfinite(g->gsd) && g->gsd > 0.0, "%s: gsd=%g must be finite and > 0", what, g->gsd);
  ADAMVS_CHECK_ARG(std::isfinite(g->x0) && std::isfinite(g->y_top) && std::isfinite(g->z_ref), "%s: grid origin / z_ref not finite", what);
  ADAMVS_CHECK_ARG(g->W > 0 && g->H > 0 && (long)g->W * g->H <= ADAMVS_DSM_MAX_CELLS, "%s: grid W=%d H=%d (W H <= %d cells)", what, g->W,
                   g->H, ADAMVS_DSM_MAX_CELLS);
  return 0;
}

static int dsm_check_points(long n, long seq0, const char* what) {
  ADAMVS_CHECK_ARG(n >= 0, "%s: n=%ld (>= 0)", what, n);
  ADAMVS_CHECK_ARG(seq0 >= 0 && seq0 <= (1L << 32) - n, "%s: seq0=%ld + n=%ld exceeds 2^32 points", what, seq0, n);
  return 0;
}

extern "C" int adamvs_dsm_accumulate(const adamvs_dsm_grid* grid, const double* xyz, long n, long seq0, int mode, unsigned long long* key,
                                     unsigned* count, long long* sum, void* stream) {
  if (int rc = dsm_check_grid(grid, "dsm_accumulate")) return rc;
  if (int rc = dsm_check_points(n, seq0, "dsm_accumulate")) return rc;
  ADAMVS_CHECK_ARG(mode == ADAMVS_DSM_MAX || mode == ADAMVS_DSM_MEAN, "dsm_accumulate: mode=%d (0 max, 1 mean)", mode);
  ADAMVS_CHECK_ARG(xyz && key && count && (sum || mode == ADAMVS_DSM_MAX), "dsm_accumulate: null pointer");
  return launch_dsm_accumulate(*grid, xyz, n, seq0, mode, key, count, sum, (hipStream_t)stream);
}

extern "C" int adamvs_dsm_claim(const adamvs_dsm_grid* grid, const double* xyz, const unsigned char* rgb, long n, long seq0,
                                const unsigned long long* key, unsigned* color, void* stream) {
  if (int rc = dsm_check_grid(grid, "dsm_claim")) return rc;
  if (int rc = dsm_check_points(n, seq0, "dsm_claim")) return rc;
  ADAMVS_CHECK_ARG(xyz && rgb && key && color, "dsm_claim: null pointer");
  return launch_dsm_claim(*grid, xyz, rgb, n, seq0, key, color, (hipStream_t)stream);
}

extern "C" int adamvs_dsm_finalize(const adamvs_dsm_grid* grid, const unsigned long long* key, const unsigned* count, const long long* sum,
                                   const unsigned* color, int mode, int min_count, float* dsm, unsigned short* count16, unsigned char* rgba,
                                   void* stream) {
  if (int rc = dsm_check_grid(grid, "dsm_finalize")) return rc;
  ADAMVS_CHECK_ARG(mode == ADAMVS_DSM_MAX || mode == ADAMVS_DSM_MEAN, "dsm_finalize: mode=%d (0 max, 1 mean)", mode);
  ADAMVS_CHECK_ARG(min_count >= 1, "dsm_finalize: min_count=%d (>= 1)", min_count);
  ADAMVS_CHECK_ARG(key && count && color && dsm && count16 && rgba && (sum || mode == ADAMVS_DSM_MAX), "dsm_finalize: null pointer");
  return launch_dsm_finalize(*grid, key, count, sum, color, mode, min_count, dsm, count16, (unsigned*)rgba, (hipStream_t)stream);
}

// ---- DSM gap fill (dsm_fill.hip)
static int dsm_fill_check_size(int W, int H, const char* what) {
  ADAMVS_CHECK_ARG(W > 0 && H > 0 && (long)W * H <= ADAMVS_DSM_MAX_CELLS, "%s: grid W=%d H=%d (W H <= %d cells)", what, W, H,
                   ADAMVS_DSM_MAX_CELLS);
  return 0;
}

extern "C" long adamvs_dsm_fill_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "dsm_fill_workspace_bytes")) return rc;
  return dsm_fill_workspace_bytes(W, H);
}

extern "C" int adamvs_dsm_fill(int W, int H, const float* dsm, const unsigned char* rgba, double r_cells, double tol_height,
                               double tol_colour, int max_cycles, void* workspace, long workspace_bytes, float* dsm_out,
                               unsigned char* rgba_out, int* dist2, unsigned char* filled, adamvs_dsm_fill_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "dsm_fill")) return rc;
  ADAMVS_CHECK_ARG(dsm && rgba && workspace && dsm_out && rgba_out && dist2 && filled && stats, "dsm_fill: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(r_cells) && r_cells > 0.0 && r_cells <= ADAMVS_DSM_FILL_MAX_RADIUS,
                   "dsm_fill: r_cells=%g must be finite, > 0 and <= %d", r_cells, ADAMVS_DSM_FILL_MAX_RADIUS);
  ADAMVS_CHECK_ARG(std::isfinite(tol_height) && tol_height > 0.0, "dsm_fill: tol_height=%g must be finite and > 0", tol_height);
  ADAMVS_CHECK_ARG(std::isfinite(tol_colour) && tol_colour > 0.0, "dsm_fill: tol_colour=%g must be finite and > 0", tol_colour);
  ADAMVS_CHECK_ARG(max_cycles >= 1, "dsm_fill: max_cycles=%d (>= 1)", max_cycles);
  const long need = dsm_fill_workspace_bytes(W, H);
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "dsm_fill: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  return launch_dsm_fill(W, H, dsm, rgba, r_cells, tol_height, tol_colour, max_cycles, workspace, dsm_out, rgba_out, dist2, filled,
                         stats, (hipStream_t)stream);
}

// ---- DSM ground filter (dsm_dtm.hip)
// true iff the byte ranges [a, a + na) and [b, b + nb) share a byte
static bool dtm_overlap(const void* a, long na, const void* b, long nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" long adamvs_dtm_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "dtm_workspace_bytes")) return rc;
  return dtm_workspace_bytes(W, H);
}

extern "C" int adamvs_dsm_open(int W, int H, const float* src, int r, void* workspace, long workspace_bytes, float* dst, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "dsm_open")) return rc;
  ADAMVS_CHECK_ARG(src && workspace && dst, "dsm_open: null pointer");
  ADAMVS_CHECK_ARG(r >= 1 && r <= ADAMVS_DTM_MAX_RADIUS, "dsm_open: r=%d (1 .. %d)", r, ADAMVS_DTM_MAX_RADIUS);
  const long need = dtm_workspace_bytes(W, H), n4 = 4L * W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "dsm_open: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  ADAMVS_CHECK_ARG(!dtm_overlap(src, n4, dst, n4) && !dtm_overlap(src, n4, workspace, need) && !dtm_overlap(dst, n4, workspace, need),
                   "dsm_open: src, dst and the workspace must not overlap");
  return launch_dsm_open(W, H, src, r, workspace, dst, (hipStream_t)stream);
}

extern "C" int adamvs_dtm_classify(int W, int H, const float* dsm, int levels, const int* radius, const double* dh, void* workspace,
                                   long workspace_bytes, unsigned char* level, float* opened, adamvs_dtm_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "dtm_classify")) return rc;
  ADAMVS_CHECK_ARG(dsm && radius && dh && workspace && level && opened && stats, "dtm_classify: null pointer");
  ADAMVS_CHECK_ARG(levels >= 1 && levels <= ADAMVS_DTM_MAX_LEVELS, "dtm_classify: levels=%d (1 .. %d)", levels, ADAMVS_DTM_MAX_LEVELS);
  for (int k = 0; k < levels; ++k) {
    ADAMVS_CHECK_ARG(radius[k] >= 1 && radius[k] <= ADAMVS_DTM_MAX_RADIUS, "dtm_classify: radius[%d]=%d (1 .. %d)", k, radius[k],
                     ADAMVS_DTM_MAX_RADIUS);
    ADAMVS_CHECK_ARG(k == 0 || radius[k] > radius[k - 1], "dtm_classify: radius[%d]=%d does not exceed radius[%d]=%d", k, radius[k], k - 1,
                     radius[k - 1]);
    ADAMVS_CHECK_ARG(std::isfinite(dh[k]) && dh[k] > 0.0, "dtm_classify: dh[%d]=%g must be finite and > 0", k, dh[k]);
  }
  const long need = dtm_workspace_bytes(W, H), n = (long)W * H, n4 = 4 * n;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "dtm_classify: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  ADAMVS_CHECK_ARG(!dtm_overlap(dsm, n4, opened, n4) && !dtm_overlap(dsm, n4, level, n) && !dtm_overlap(opened, n4, level, n) &&
                       !dtm_overlap(dsm, n4, workspace, need) && !dtm_overlap(opened, n4, workspace, need) &&
                       !dtm_overlap(level, n, workspace, need),
                   "dtm_classify: dsm, level, opened and the workspace must not overlap");
  return launch_dtm_classify(W, H, dsm, levels, radius, dh, workspace, level, opened, stats, (hipStream_t)stream);
}

// ---- Building extraction (dsm_buildings.hip)
struct BldBuffer {
  const void* p;
  long bytes;
};

static bool bld_any_overlap(const BldBuffer* b, int count) {
  for (int i = 0; i < count; ++i)
    for (int j = i + 1; j < count; ++j)
      if (dtm_overlap(b[i].p, b[i].bytes, b[j].p, b[j].bytes)) return true;
  return false;
}

extern "C" long adamvs_bld_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "bld_workspace_bytes")) return rc;
  return bld_workspace_bytes(W, H);
}

extern "C" int adamvs_bld_flags(int W, int H, const float* dsm, const float* ndsm, double min_height, int r_open, int s, double smooth_tol,
                                void* workspace, long workspace_bytes, unsigned char* flags, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "bld_flags")) return rc;
  ADAMVS_CHECK_ARG(dsm && ndsm && workspace && flags, "bld_flags: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(min_height) && min_height > 0.0, "bld_flags: min_height=%g must be finite and > 0", min_height);
  ADAMVS_CHECK_ARG(r_open >= 0 && r_open <= ADAMVS_DTM_MAX_RADIUS, "bld_flags: r_open=%d (0 .. %d)", r_open, ADAMVS_DTM_MAX_RADIUS);
  ADAMVS_CHECK_ARG(s >= 1 && s <= ADAMVS_BLD_MAX_STRIDE, "bld_flags: s=%d (1 .. %d)", s, ADAMVS_BLD_MAX_STRIDE);
  ADAMVS_CHECK_ARG(std::isfinite(smooth_tol) && smooth_tol >= 0.0, "bld_flags: smooth_tol=%g must be finite and >= 0", smooth_tol);
  const long need = bld_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "bld_flags: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{dsm, 4 * n}, {ndsm, 4 * n}, {flags, n}, {workspace, need}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "bld_flags: dsm, ndsm, flags and the workspace must not overlap");
  return launch_bld_flags(W, H, dsm, ndsm, min_height, r_open, s, smooth_tol, workspace, flags, (hipStream_t)stream);
}

extern "C" int adamvs_bld_label(int W, int H, const unsigned char* flags, void* workspace, long workspace_bytes, int* parent,
                                adamvs_bld_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "bld_label")) return rc;
  ADAMVS_CHECK_ARG(flags && workspace && parent && stats, "bld_label: null pointer");
  const long need = bld_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "bld_label: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{flags, n}, {parent, 4 * n}, {workspace, need}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "bld_label: flags, parent and the workspace must not overlap");
  return launch_bld_label(W, H, flags, workspace, parent, stats, (hipStream_t)stream);
}

extern "C" int adamvs_bld_table(int W, int H, const unsigned char* flags, const float* ndsm, const int* label, long N, long long* table,
                                void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "bld_table")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(N >= 0 && N <= n, "bld_table: N=%ld (0 .. W H = %ld)", N, n);
  ADAMVS_CHECK_ARG(flags && ndsm && label && (table || N == 0), "bld_table: null pointer");
  const BldBuffer b[] = {{flags, n}, {ndsm, 4 * n}, {label, 4 * n}, {table, 8L * ADAMVS_BLD_COLUMNS * N}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, N ? 4 : 3), "bld_table: flags, ndsm, label and the table must not overlap");
  return launch_bld_table(W, H, flags, ndsm, label, N, table, (hipStream_t)stream);
}

// ---- Roof planes (dsm_roofs.hip)
static int roof_check_size(int W, int H, const char* what) {
  ADAMVS_CHECK_ARG(W > 0 && H > 0 && W <= ADAMVS_ROOF_MAX_SIDE && H <= ADAMVS_ROOF_MAX_SIDE && (long)W * H <= ADAMVS_DSM_MAX_CELLS,
                   "%s: grid W=%d H=%d (each <= %d, W H <= %d cells)", what, W, H, ADAMVS_ROOF_MAX_SIDE, ADAMVS_DSM_MAX_CELLS);
  return 0;
}

static bool roof_tol_ok(double v) { return std::isfinite(v) && v >= 0.0; }

extern "C" long adamvs_roof_workspace_bytes(int W, int H) {
  if (int rc = roof_check_size(W, H, "roof_workspace_bytes")) return rc;
  return roof_workspace_bytes(W, H);
}

extern "C" int adamvs_roof_links(int W, int H, const float* dsm, const int* building, int s, double smooth_tol, double g_tol,
                                 double step_tol, unsigned char* link, void* stream) {
  if (int rc = roof_check_size(W, H, "roof_links")) return rc;
  ADAMVS_CHECK_ARG(dsm && building && link, "roof_links: null pointer");
  ADAMVS_CHECK_ARG(s >= 1 && s <= ADAMVS_BLD_MAX_STRIDE, "roof_links: s=%d (1 .. %d)", s, ADAMVS_BLD_MAX_STRIDE);
  ADAMVS_CHECK_ARG(roof_tol_ok(smooth_tol) && roof_tol_ok(g_tol) && roof_tol_ok(step_tol),
                   "roof_links: smooth_tol=%g, g_tol=%g, step_tol=%g must be finite and >= 0", smooth_tol, g_tol, step_tol);
  const long n = (long)W * H;
  const BldBuffer b[] = {{dsm, 4 * n}, {building, 4 * n}, {link, n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "roof_links: dsm, building and link must not overlap");
  return launch_roof_links(W, H, dsm, building, s, smooth_tol, g_tol, step_tol, link, (hipStream_t)stream);
}

extern "C" int adamvs_roof_label(int W, int H, const unsigned char* link, void* workspace, long workspace_bytes, int* parent,
                                 adamvs_bld_stats* stats, void* stream) {
  if (int rc = roof_check_size(W, H, "roof_label")) return rc;
  ADAMVS_CHECK_ARG(link && workspace && parent && stats, "roof_label: null pointer");
  const long need = roof_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "roof_label: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{link, n}, {parent, 4 * n}, {workspace, need}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "roof_label: link, parent and the workspace must not overlap");
  return launch_roof_label(W, H, link, workspace, parent, stats, (hipStream_t)stream);
}

extern "C" int adamvs_roof_moments(int W, int H, const float* dsm, const int* label, const int* building, double z_ref, long N,
                                   long long* table, void* stream) {
  if (int rc = roof_check_size(W, H, "roof_moments")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(N >= 0 && N <= n, "roof_moments: N=%ld (0 .. W H = %ld)", N, n);
  ADAMVS_CHECK_ARG(dsm && label && building && (table || N == 0), "roof_moments: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(z_ref), "roof_moments: z_ref=%g must be finite", z_ref);
  const BldBuffer b[] = {{dsm, 4 * n}, {label, 4 * n}, {building, 4 * n}, {table, 8L * ADAMVS_ROOF_COLUMNS * N}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, N ? 4 : 3), "roof_moments: dsm, label, building and the table must not overlap");
  return launch_roof_moments(W, H, dsm, label, building, z_ref, N, table, (hipStream_t)stream);
}

extern "C" int adamvs_roof_grow(int W, int H, const float* dsm, const int* building, double z_ref, long P, const double* planes,
                                double assign_tol, int round0, int rounds, int* label0, int* label1, unsigned* counts, void* stream) {
  if (int rc = roof_check_size(W, H, "roof_grow")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(P >= 0 && P <= n, "roof_grow: P=%ld (0 .. W H = %ld)", P, n);
  ADAMVS_CHECK_ARG(dsm && building && (planes || P == 0) && label0 && label1 && counts, "roof_grow: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(z_ref), "roof_grow: z_ref=%g must be finite", z_ref);
  ADAMVS_CHECK_ARG(roof_tol_ok(assign_tol), "roof_grow: assign_tol=%g must be finite and >= 0", assign_tol);
  ADAMVS_CHECK_ARG(round0 >= 0 && rounds >= 0 && round0 <= ADAMVS_ROOF_MAX_GROW && rounds <= ADAMVS_ROOF_MAX_GROW - round0,
                   "roof_grow: rounds %d .. %d + %d (at most %d in all)", round0, round0, rounds, ADAMVS_ROOF_MAX_GROW);
  const BldBuffer b[] = {{dsm, 4 * n}, {building, 4 * n}, {label0, 4 * n}, {label1, 4 * n}, {counts, 4L * ADAMVS_ROOF_MAX_GROW},
                         {planes, 24 * P}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, P ? 6 : 5), "roof_grow: dsm, building, the two label buffers, counts and planes must not overlap");
  return launch_roof_grow(W, H, dsm, building, z_ref, P, planes, assign_tol, round0, rounds, label0, label1, counts, (hipStream_t)stream);
}

extern "C" int adamvs_roof_residuals(int W, int H, const float* dsm, const int* label, double z_ref, long R, const double* planes,
                                     double assign_tol, long long* table, void* stream) {
  if (int rc = roof_check_size(W, H, "roof_residuals")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(R >= 0 && R <= n, "roof_residuals: R=%ld (0 .. W H = %ld)", R, n);
  ADAMVS_CHECK_ARG(dsm && label && ((planes && table) || R == 0), "roof_residuals: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(z_ref), "roof_residuals: z_ref=%g must be finite", z_ref);
  ADAMVS_CHECK_ARG(roof_tol_ok(assign_tol), "roof_residuals: assign_tol=%g must be finite and >= 0", assign_tol);
  const BldBuffer b[] = {{dsm, 4 * n}, {label, 4 * n}, {planes, 24 * R}, {table, 16 * R}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, R ? 4 : 2), "roof_residuals: dsm, label, planes and the table must not overlap");
  return launch_roof_residuals(W, H, dsm, label, z_ref, R, planes, assign_tol, table, (hipStream_t)stream);
}

// ---- LoD2 solids (dsm_lod2.hip)
static int lod2_check_size(int W, int H, const char* what) {
  ADAMVS_CHECK_ARG(W > 0 && H > 0 && W <= ADAMVS_LOD2_MAX_SIDE && H <= ADAMVS_LOD2_MAX_SIDE && (long)W * H <= ADAMVS_DSM_MAX_CELLS,
                   "%s: grid W=%d H=%d (each <= %d, W H <= %d cells)", what, W, H, ADAMVS_LOD2_MAX_SIDE, ADAMVS_DSM_MAX_CELLS);
  return 0;
}

extern "C" long adamvs_lod2_workspace_bytes(int W, int H) {
  if (int rc = lod2_check_size(W, H, "lod2_workspace_bytes")) return rc;
  return lod2_workspace_bytes(W, H);
}

extern "C" int adamvs_lod2_corner_heights_host(long P, const long long* planes, long n, const int* plane, const int* row, const int* col,
                                               long long* zq) {
  ADAMVS_CHECK_ARG(P >= 0 && n >= 0, "lod2_corner_heights_host: P=%ld, n=%ld must be >= 0", P, n);
  ADAMVS_CHECK_ARG(n == 0 || (planes && plane && row && col && zq), "lod2_corner_heights_host: null pointer");
  for (long i = 0; i < n; ++i)
    ADAMVS_CHECK_ARG(plane[i] >= 1 && plane[i] <= P && row[i] >= 0 && row[i] <= ADAMVS_LOD2_MAX_SIDE && col[i] >= 0 &&
                         col[i] <= ADAMVS_LOD2_MAX_SIDE,
                     "lod2_corner_heights_host: entry %ld: plane %d (1 .. %ld) at corner (%d, %d) (0 .. %d)", i, plane[i], P, row[i], col[i],
                     ADAMVS_LOD2_MAX_SIDE);
  for (long i = 0; i < n; ++i) zq[i] = lod2_corner_height(planes + 3 * (long)(plane[i] - 1), row[i], col[i]);
  return 0;
}

extern "C" int adamvs_lod2_fill(int W, int H, const int* building, long P, int round0, int rounds, int* label0, int* label1,
                                unsigned* counts, void* stream) {
  if (int rc = lod2_check_size(W, H, "lod2_fill")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "lod2_fill: P=%ld (0 .. %d)", P, ADAMVS_DSM_MAX_CELLS);
  ADAMVS_CHECK_ARG(building && label0 && label1 && counts, "lod2_fill: null pointer");
  ADAMVS_CHECK_ARG(round0 >= 0 && rounds >= 0 && round0 <= ADAMVS_LOD2_MAX_FILL && rounds <= ADAMVS_LOD2_MAX_FILL - round0,
                   "lod2_fill: rounds %d .. %d + %d (at most %d in all)", round0, round0, rounds, ADAMVS_LOD2_MAX_FILL);
  const BldBuffer b[] = {{building, 4 * n}, {label0, 4 * n}, {label1, 4 * n}, {counts, 4L * ADAMVS_LOD2_MAX_FILL}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "lod2_fill: building, the two label buffers and counts must not overlap");
  return launch_lod2_fill(W, H, building, P, round0, rounds, label0, label1, counts, (hipStream_t)stream);
}

extern "C" int adamvs_lod2_table(int W, int H, const float* dtm, const int* building, const int* label, double z_ref, long B, long P,
                                 const long long* planes, long long* table, void* stream) {
  if (int rc = lod2_check_size(W, H, "lod2_table")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(B >= 0 && B <= ADAMVS_DSM_MAX_CELLS && P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "lod2_table: B=%ld, P=%ld (0 .. %d)", B, P,
                   ADAMVS_DSM_MAX_CELLS);
  ADAMVS_CHECK_ARG(dtm && building && label && (planes || P == 0) && (table || B == 0), "lod2_table: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(z_ref), "lod2_table: z_ref=%g must be finite", z_ref);
  const BldBuffer b[] = {{dtm, 4 * n}, {building, 4 * n}, {label, 4 * n}, {table, 8L * ADAMVS_LOD2_COLUMNS * B}, {planes, 24 * P}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, !B ? 3 : !P ? 4 : 5), "lod2_table: dtm, building, label, the table and planes must not overlap");
  return launch_lod2_table(W, H, dtm, building, label, z_ref, B, P, planes, table, (hipStream_t)stream);
}

extern "C" int adamvs_lod2_transpose(int W, int H, const int* src, int* dst, void* stream) {
  if (int rc = lod2_check_size(W, H, "lod2_transpose")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(src && dst, "lod2_transpose: null pointer");
  const BldBuffer b[] = {{src, 4 * n}, {dst, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 2), "lod2_transpose: src and dst must not overlap");
  return launch_lod2_transpose(W, H, src, dst, (hipStream_t)stream);
}

extern "C" int adamvs_lod2_count(int W, int H, const int* label, const int* label_t, long P, void* workspace, long workspace_bytes,
                                 unsigned* total, void* stream) {
  if (int rc = lod2_check_size(W, H, "lod2_count")) return rc;
  const long n = (long)W * H, need = lod2_workspace_bytes(W, H);
  ADAMVS_CHECK_ARG(P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "lod2_count: P=%ld (0 .. %d)", P, ADAMVS_DSM_MAX_CELLS);
  ADAMVS_CHECK_ARG(label && label_t && workspace && total, "lod2_count: null pointer");
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "lod2_count: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{label, 4 * n}, {label_t, 4 * n}, {workspace, need}, {total, 4}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "lod2_count: label, label_t, total and the workspace must not overlap");
  return launch_lod2_count(W, H, label, label_t, P, workspace, total, (hipStream_t)stream);
}

extern "C" int adamvs_lod2_runs(int W, int H, const int* label, const int* label_t, long P, const long long* planes, const int* plane_base,
                                long N, void* workspace, long workspace_bytes, int* records, void* stream) {
  if (int rc = lod2_check_size(W, H, "lod2_runs")) return rc;
  const long n = (long)W * H, need = lod2_workspace_bytes(W, H), edges = (long)(H + 1) * W + (long)(W + 1) * H;
  ADAMVS_CHECK_ARG(P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "lod2_runs: P=%ld (0 .. %d)", P, ADAMVS_DSM_MAX_CELLS);
  ADAMVS_CHECK_ARG(N >= 0 && N <= edges, "lod2_runs: N=%ld (0 .. %ld lattice edges)", N, edges);
  ADAMVS_CHECK_ARG(label && label_t && workspace && ((planes && plane_base) || P == 0) && (records || N == 0), "lod2_runs: null pointer");
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "lod2_runs: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{label, 4 * n}, {label_t, 4 * n}, {workspace, need}, {records, 4L * ADAMVS_LOD2_FIELDS * N}, {planes, 24 * P},
                         {plane_base, 4 * P}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, !N ? 3 : !P ? 4 : 6), "lod2_runs: the inputs, the records and the workspace must not overlap");
  return launch_lod2_runs(W, H, label, label_t, P, planes, plane_base, N, workspace, records, (hipStream_t)stream);
}

// ---- Trees (dsm_trees.hip)
extern "C" long adamvs_tree_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "tree_workspace_bytes")) return rc;
  return tree_workspace_bytes(W, H);
}

extern "C" int adamvs_tree_surface(int W, int H, const float* ndsm, const int* building, double min_height, int smooth_passes,
                                   void* workspace, long workspace_bytes, unsigned char* mask, int* q, int* s, int* s_max, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "tree_surface")) return rc;
  ADAMVS_CHECK_ARG(ndsm && workspace && mask && q && s && s_max, "tree_surface: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(min_height) && min_height > 0.0, "tree_surface: min_height=%g must be finite and > 0", min_height);
  ADAMVS_CHECK_ARG(smooth_passes >= 0 && smooth_passes <= 2, "tree_surface: smooth_passes=%d (0 .. 2)", smooth_passes);
  const long need = tree_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "tree_surface: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{ndsm, 4 * n}, {workspace, need}, {mask, n}, {q, 4 * n}, {s, 4 * n}, {s_max, 4}, {building, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, building ? 7 : 6), "tree_surface: ndsm, building, mask, q, s, s_max and the workspace must not overlap");
  return launch_tree_surface(W, H, ndsm, building, min_height, smooth_passes, workspace, mask, q, s, s_max, (hipStream_t)stream);
}

extern "C" int adamvs_tree_parents(int W, int H, const int* s, int r_cap, const int* thr, void* workspace, long workspace_bytes, int* parent,
                                   adamvs_tree_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "tree_parents")) return rc;
  ADAMVS_CHECK_ARG(s && thr && workspace && parent && stats, "tree_parents: null pointer");
  ADAMVS_CHECK_ARG(r_cap >= 1 && r_cap <= ADAMVS_TREE_MAX_RADIUS, "tree_parents: r_cap=%d (1 .. %d)", r_cap, ADAMVS_TREE_MAX_RADIUS);
  ADAMVS_CHECK_ARG(thr[0] == 0, "tree_parents: thr[1]=%d must be 0", thr[0]);
  for (int k = 1; k < r_cap; ++k)
    ADAMVS_CHECK_ARG(thr[k] >= thr[k - 1], "tree_parents: thr[%d]=%d is below thr[%d]=%d", k + 1, thr[k], k, thr[k - 1]);
  const long need = tree_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "tree_parents: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {parent, 4 * n}, {workspace, need}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "tree_parents: s, parent and the workspace must not overlap");
  return launch_tree_parents(W, H, s, r_cap, thr, workspace, parent, stats, (hipStream_t)stream);
}

extern "C" int adamvs_tree_roots(int W, int H, const int* parent, void* workspace, long workspace_bytes, int* root, adamvs_tree_stats* stats,
                                 void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "tree_roots")) return rc;
  ADAMVS_CHECK_ARG(parent && workspace && root && stats, "tree_roots: null pointer");
  const long need = tree_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "tree_roots: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{parent, 4 * n}, {root, 4 * n}, {workspace, need}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "tree_roots: parent, root and the workspace must not overlap");
  return launch_tree_roots(W, H, parent, workspace, root, stats, (hipStream_t)stream);
}

extern "C" int adamvs_tree_crowns(int W, int H, const int* s, const int* root, const int* number, int ratio_pm, long rc2, int* label,
                                  long long* unassigned, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "tree_crowns")) return rc;
  ADAMVS_CHECK_ARG(s && root && number && label && unassigned, "tree_crowns: null pointer");
  ADAMVS_CHECK_ARG(ratio_pm >= 0 && ratio_pm <= 1000, "tree_crowns: ratio_pm=%d (0 .. 1000)", ratio_pm);
  ADAMVS_CHECK_ARG(rc2 >= 0, "tree_crowns: rc2=%ld must be >= 0", rc2);
  const long n = (long)W * H;
  const BldBuffer b[] = {{s, 4 * n}, {root, 4 * n}, {number, 4 * n}, {label, 4 * n}, {unassigned, 8}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 5), "tree_crowns: s, root, number, label and unassigned must not overlap");
  return launch_tree_crowns(W, H, s, root, number, ratio_pm, rc2, label, unassigned, (hipStream_t)stream);
}

extern "C" int adamvs_tree_table(int W, int H, const int* label, const int* q, const int* s, const int* root, long T, long long* table,
                                 void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "tree_table")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(T >= 0 && T <= n, "tree_table: T=%ld (0 .. W H = %ld)", T, n);
  ADAMVS_CHECK_ARG(label && q && s && root && (table || T == 0), "tree_table: null pointer");
  const BldBuffer b[] = {{label, 4 * n}, {q, 4 * n}, {s, 4 * n}, {root, 4 * n}, {table, 8L * ADAMVS_TREE_COLUMNS * T}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, T ? 5 : 4), "tree_table: label, q, s, root and the table must not overlap");
  return launch_tree_table(W, H, label, q, s, root, T, table, (hipStream_t)stream);
}

// ---- Contours (dsm_contours.hip)
static int contour_check_levels(int K, const int* lev, const char* what) {
  ADAMVS_CHECK_ARG(K >= 0 && K <= ADAMVS_CONTOUR_MAX_LEVELS, "%s: K=%d (0 .. %d)", what, K, ADAMVS_CONTOUR_MAX_LEVELS);
  ADAMVS_CHECK_ARG(lev, "%s: null pointer", what);
  for (int k = 1; k < K; ++k)
    ADAMVS_CHECK_ARG(lev[k] > lev[k - 1], "%s: lev[%d]=%d does not exceed lev[%d]=%d", what, k, lev[k], k - 1, lev[k - 1]);
  return 0;
}

static int contour_check_segments(long N, const char* what) {
  ADAMVS_CHECK_ARG(N >= 0 && N < (1L << 31), "%s: N=%ld (0 .. 2^31 - 1)", what, N);
  return 0;
}

extern "C" long adamvs_contour_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "contour_workspace_bytes")) return rc;
  return contour_workspace_bytes(W, H);
}

extern "C" long adamvs_contour_rank_workspace_bytes(long N) {
  if (int rc = contour_check_segments(N, "contour_rank_workspace_bytes")) return rc;
  return contour_rank_workspace_bytes(N);
}

extern "C" int adamvs_contour_surface(int W, int H, const float* z, double z_ref, int smooth_passes, void* workspace, long workspace_bytes,
                                      int* s, int* info, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "contour_surface")) return rc;
  ADAMVS_CHECK_ARG(z && workspace && s && info, "contour_surface: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(z_ref), "contour_surface: z_ref=%g must be finite", z_ref);
  ADAMVS_CHECK_ARG(smooth_passes >= 0 && smooth_passes <= 2, "contour_surface: smooth_passes=%d (0 .. 2)", smooth_passes);
  const long need = contour_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "contour_surface: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{z, 4 * n}, {workspace, need}, {s, 4 * n}, {info, 12}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "contour_surface: z, s, info and the workspace must not overlap");
  return launch_contour_surface(W, H, z, z_ref, smooth_passes, workspace, s, info, (hipStream_t)stream);
}

extern "C" int adamvs_contour_count(int W, int H, const int* s, int K, const int* lev, void* workspace, long workspace_bytes, int* count,
                                    adamvs_contour_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "contour_count")) return rc;
  ADAMVS_CHECK_ARG(s && workspace && count && stats, "contour_count: null pointer");
  if (int rc = contour_check_levels(K, lev, "contour_count")) return rc;
  const long need = contour_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "contour_count: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {workspace, need}, {count, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 3), "contour_count: s, count and the workspace must not overlap");
  return launch_contour_count(W, H, s, K, lev, workspace, count, stats, (hipStream_t)stream);
}

extern "C" int adamvs_contour_segments(int W, int H, const int* s, int K, const int* lev, long N, void* workspace, long workspace_bytes,
                                       int* seg_entry, int* seg_exit, int* seg_level, int* succ, int* pred, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "contour_segments")) return rc;
  if (int rc = contour_check_segments(N, "contour_segments")) return rc;
  ADAMVS_CHECK_ARG(s && workspace && (N == 0 || (seg_entry && seg_exit && seg_level && succ && pred)), "contour_segments: null pointer");
  if (int rc = contour_check_levels(K, lev, "contour_segments")) return rc;
  const long need = contour_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "contour_segments: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {workspace, need}, {seg_entry, 4 * N}, {seg_exit, 4 * N}, {seg_level, 4 * N}, {succ, 4 * N}, {pred, 4 * N}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, N ? 7 : 2), "contour_segments: s, the five segment arrays and the workspace must not overlap");
  return launch_contour_segments(W, H, s, K, lev, N, workspace, seg_entry, seg_exit, seg_level, succ, pred, (hipStream_t)stream);
}

extern "C" int adamvs_contour_rank(long N, const int* pred, void* workspace, long workspace_bytes, int* start, int* rank,
                                   unsigned char* closed, adamvs_contour_stats* stats, void* stream) {
  if (int rc = contour_check_segments(N, "contour_rank")) return rc;
  ADAMVS_CHECK_ARG(workspace && stats && (N == 0 || (pred && start && rank && closed)), "contour_rank: null pointer");
  const long need = contour_rank_workspace_bytes(N);
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "contour_rank: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{workspace, need}, {pred, 4 * N}, {start, 4 * N}, {rank, 4 * N}, {closed, N}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, N ? 5 : 1), "contour_rank: pred, start, rank, closed and the workspace must not overlap");
  return launch_contour_rank(N, pred, workspace, start, rank, closed, stats, (hipStream_t)stream);
}

extern "C" int adamvs_contour_lines(int W, int H, const int* s, int K, const int* lev, long N, long M, const int* seg_entry,
                                    const int* seg_exit, const int* seg_level, const int* succ, const int* start, const int* rank,
                                    const unsigned char* closed, void* workspace, long workspace_bytes, long long* line_first,
                                    int* line_start, int* line_level, unsigned char* line_closed, long long* vertex, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "contour_lines")) return rc;
  if (int rc = contour_check_segments(N, "contour_lines")) return rc;
  ADAMVS_CHECK_ARG(M >= 0 && M <= N && (M > 0) == (N > 0) && N + M < (1L << 31), "contour_lines: M=%ld lines of N=%ld segments (N + M < 2^31)", M, N);
  ADAMVS_CHECK_ARG(s && workspace && line_first, "contour_lines: null pointer");
  ADAMVS_CHECK_ARG(N == 0 || (seg_entry && seg_exit && seg_level && succ && start && rank && closed && line_start && line_level && line_closed && vertex),
                   "contour_lines: null pointer");
  if (int rc = contour_check_levels(K, lev, "contour_lines")) return rc;
  const long need = contour_rank_workspace_bytes(N), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "contour_lines: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {workspace, need}, {line_first, 8 * (M + 1)}, {seg_entry, 4 * N}, {seg_exit, 4 * N}, {seg_level, 4 * N},
                         {succ, 4 * N}, {start, 4 * N}, {rank, 4 * N}, {closed, N}, {line_start, 4 * M}, {line_level, 4 * M}, {line_closed, M},
                         {vertex, 24 * (N + M)}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, N ? 14 : 3), "contour_lines: the inputs, the outputs and the workspace must not overlap");
  return launch_contour_lines(W, H, s, K, lev, N, M, seg_entry, seg_exit, seg_level, succ, start, rank, closed, workspace, line_first, line_start,
                              line_level, line_closed, vertex, (hipStream_t)stream);
}

// ---- Drainage (dsm_drainage.hip)
extern "C" long adamvs_drain_workspace_bytes(int W, int H) {
  if (int rc = dsm_fill_check_size(W, H, "drain_workspace_bytes")) return rc;
  return drain_workspace_bytes(W, H);
}

extern "C" int adamvs_drain_fill(int W, int H, const int* s, int smooth_passes, int max_rounds, void* workspace, long workspace_bytes, int* r,
                                 int* F, adamvs_drain_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "drain_fill")) return rc;
  ADAMVS_CHECK_ARG(s && workspace && r && F && stats, "drain_fill: null pointer");
  ADAMVS_CHECK_ARG(smooth_passes >= 0 && smooth_passes <= 2, "drain_fill: smooth_passes=%d (0 .. 2)", smooth_passes);
  ADAMVS_CHECK_ARG(max_rounds >= 1, "drain_fill: max_rounds=%d must be >= 1", max_rounds);
  const long need = drain_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "drain_fill: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {workspace, need}, {r, 4 * n}, {F, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "drain_fill: s, r, F and the workspace must not overlap");
  return launch_drain_fill(W, H, s, smooth_passes, max_rounds, workspace, r, F, stats, (hipStream_t)stream);
}

extern "C" int adamvs_drain_direction(int W, int H, const int* F, unsigned char* dir, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "drain_direction")) return rc;
  ADAMVS_CHECK_ARG(F && dir, "drain_direction: null pointer");
  const long n = (long)W * H;
  const BldBuffer b[] = {{F, 4 * n}, {dir, n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 2), "drain_direction: F and dir must not overlap");
  return launch_drain_direction(W, H, F, dir, (hipStream_t)stream);
}

extern "C" int adamvs_drain_accumulate(int W, int H, const unsigned char* dir, const int* value, void* workspace, long workspace_bytes,
                                       int* acc, int* root, adamvs_drain_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "drain_accumulate")) return rc;
  ADAMVS_CHECK_ARG(dir && workspace && acc && root && stats, "drain_accumulate: null pointer");
  const long need = drain_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "drain_accumulate: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{dir, n}, {workspace, need}, {acc, 4 * n}, {root, 4 * n}, {value, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, value ? 5 : 4), "drain_accumulate: dir, value, acc, root and the workspace must not overlap");
  return launch_drain_accumulate(W, H, dir, value, workspace, acc, root, stats, (hipStream_t)stream);
}

extern "C" int adamvs_drain_streams(int W, int H, const unsigned char* dir, const int* acc, int min_cells, void* workspace, long workspace_bytes,
                                    unsigned char* nd, int* link, int* pos, adamvs_drain_stats* stats, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "drain_streams")) return rc;
  ADAMVS_CHECK_ARG(dir && acc && workspace && nd && link && pos && stats, "drain_streams: null pointer");
  ADAMVS_CHECK_ARG(min_cells >= 1, "drain_streams: min_cells=%d must be >= 1", min_cells);
  const long need = drain_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "drain_streams: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{dir, n}, {acc, 4 * n}, {workspace, need}, {nd, n}, {link, 4 * n}, {pos, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 6), "drain_streams: dir, acc, nd, link, pos and the workspace must not overlap");
  return launch_drain_streams(W, H, dir, acc, min_cells, workspace, nd, link, pos, stats, (hipStream_t)stream);
}

extern "C" int adamvs_drain_links(int W, int H, const unsigned char* dir, const unsigned char* nd, const int* link, const int* pos, long L,
                                  long P, void* workspace, long workspace_bytes, int* link_first, int* link_head, int* link_end, int* link_to,
                                  int* vertex, void* stream) {
  if (int rc = dsm_fill_check_size(W, H, "drain_links")) return rc;
  const long need = drain_workspace_bytes(W, H), n = (long)W * H;
  ADAMVS_CHECK_ARG(L >= 0 && L <= n && P >= 2 * L && P < (1L << 31) && (L > 0 || P == 0), "drain_links: L=%ld links with P=%ld vertices (L <= W H, 2 L <= P < 2^31)",
                   L, P);
  ADAMVS_CHECK_ARG(dir && nd && link && pos && workspace && link_first, "drain_links: null pointer");
  ADAMVS_CHECK_ARG(L == 0 || (link_head && link_end && link_to && vertex), "drain_links: null pointer");
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "drain_links: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{dir, n}, {nd, n}, {link, 4 * n}, {pos, 4 * n}, {workspace, need}, {link_first, 4 * (L + 1)}, {link_head, 4 * L},
                         {link_end, 4 * L}, {link_to, 4 * L}, {vertex, 4 * P}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, L ? 10 : 6), "drain_links: the inputs, the outputs and the workspace must not overlap");
  return launch_drain_links(W, H, dir, nd, link, pos, L, P, workspace, link_first, link_head, link_end, link_to, vertex, (hipStream_t)stream);
}

// ---- Solar (dsm_solar.hip)
static int solar_check_size(int W, int H, int K, const char* what) {
  if (int rc = dsm_fill_check_size(W, H, what)) return rc;
  ADAMVS_CHECK_ARG(W <= ADAMVS_SOLAR_MAX_SIDE && H <= ADAMVS_SOLAR_MAX_SIDE, "%s: grid W=%d H=%d (a side of at most %d cells)", what, W, H,
                   ADAMVS_SOLAR_MAX_SIDE);
  ADAMVS_CHECK_ARG(K == 8 || K == 16 || K == 32, "%s: K=%d directions (8, 16 or 32)", what, K);
  return 0;
}

extern "C" long adamvs_solar_workspace_bytes(int W, int H, int K) {
  if (int rc = solar_check_size(W, H, K, "solar_workspace_bytes")) return rc;
  return solar_workspace_bytes(W, H, K);
}

extern "C" int adamvs_solar_horizon(int W, int H, int K, const int* s, void* workspace, long workspace_bytes, int* hz_n, int* hz_h,
                                    adamvs_solar_stats* stats, void* stream) {
  if (int rc = solar_check_size(W, H, K, "solar_horizon")) return rc;
  ADAMVS_CHECK_ARG(s && workspace && hz_n && hz_h && stats, "solar_horizon: null pointer");
  const long need = solar_workspace_bytes(W, H, K), n = (long)W * H;
  ADAMVS_CHECK_ARG(workspace_bytes >= need, "solar_horizon: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  const BldBuffer b[] = {{s, 4 * n}, {workspace, need}, {hz_n, 4 * n * K}, {hz_h, 4 * n * K}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "solar_horizon: s, hz_n, hz_h and the workspace must not overlap");
  return launch_solar_horizon(W, H, K, s, workspace, hz_n, hz_h, stats, (hipStream_t)stream);
}

extern "C" int adamvs_solar_svf(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, const double* weight, double q, double* svf,
                                void* stream) {
  if (int rc = solar_check_size(W, H, K, "solar_svf")) return rc;
  ADAMVS_CHECK_ARG(s && hz_n && hz_h && weight && svf, "solar_svf: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(q) && q > 0.0, "solar_svf: q=%g must be finite and > 0", q);
  for (int k = 0; k < K; ++k) ADAMVS_CHECK_ARG(std::isfinite(weight[k]) && weight[k] > 0.0, "solar_svf: weight[%d]=%g must be finite and > 0", k, weight[k]);
  const long n = (long)W * H;
  const BldBuffer b[] = {{s, 4 * n}, {hz_n, 4 * n * K}, {hz_h, 4 * n * K}, {svf, 8 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, 4), "solar_svf: s, hz_n, hz_h and svf must not overlap");
  return launch_solar_svf(W, H, K, s, hz_n, hz_h, weight, q, svf, (hipStream_t)stream);
}

extern "C" int adamvs_solar_expose(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, int T, const int* sector, const double* thr,
                                   const int* minutes_w, const int* energy_w, const int* sun, const int* label, long P, const int* normal,
                                   void* workspace, long workspace_bytes, int* minutes, int* direct, void* stream) {
  if (int rc = solar_check_size(W, H, K, "solar_expose")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(T >= 0 && T <= ADAMVS_SOLAR_MAX_SAMPLES, "solar_expose: T=%d samples (0 .. %d)", T, ADAMVS_SOLAR_MAX_SAMPLES);
  ADAMVS_CHECK_ARG(s && hz_n && hz_h && workspace && minutes && direct, "solar_expose: null pointer");
  ADAMVS_CHECK_ARG(T == 0 || (sector && thr && minutes_w && energy_w && sun), "solar_expose: null pointer");
  ADAMVS_CHECK_ARG(P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "solar_expose: P=%ld planes (0 .. %d)", P, ADAMVS_DSM_MAX_CELLS);
  ADAMVS_CHECK_ARG((label == nullptr) == (normal == nullptr), "solar_expose: label and normal go together");
  long sum_m = 0, sum_e = 0;
  for (int t = 0; t < T; ++t) {
    ADAMVS_CHECK_ARG(sector[t] >= 0 && sector[t] < K && (t == 0 || sector[t] >= sector[t - 1]), "solar_expose: sector[%d]=%d (0 .. %d, ascending)", t,
                     sector[t], K - 1);
    ADAMVS_CHECK_ARG(std::isfinite(thr[t]) && thr[t] >= 0.0, "solar_expose: thr[%d]=%g must be finite and >= 0", t, thr[t]);
    ADAMVS_CHECK_ARG(minutes_w[t] >= 0 && energy_w[t] >= 0, "solar_expose: the weights of sample %d (%d, %d) must be >= 0", t, minutes_w[t], energy_w[t]);
    for (int a = 0; a < 3; ++a)
      ADAMVS_CHECK_ARG(sun[3 * t + a] >= -32768 && sun[3 * t + a] <= 32768, "solar_expose: sun[%d][%d]=%d (|v| <= 32768)", t, a, sun[3 * t + a]);
    sum_m += minutes_w[t];
    sum_e += energy_w[t];
  }
  ADAMVS_CHECK_ARG(sum_m <= 2147483647L && sum_e <= 2147483647L, "solar_expose: the weights sum to %ld minutes and %ld energy units (at most 2^31 - 1 each)",
                   sum_m, sum_e);
  ADAMVS_CHECK_ARG(workspace_bytes >= ADAMVS_SOLAR_HEAD_BYTES, "solar_expose: workspace of %ld bytes, %d needed", workspace_bytes, ADAMVS_SOLAR_HEAD_BYTES);
  const BldBuffer b[] = {{s, 4 * n}, {hz_n, 4 * n * K}, {hz_h, 4 * n * K}, {workspace, ADAMVS_SOLAR_HEAD_BYTES}, {minutes, 4 * n}, {direct, 4 * n},
                         {label, 4 * n}, {normal, 12 * (P + 1)}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, label ? 8 : 6), "solar_expose: the inputs, the outputs and the workspace must not overlap");
  return launch_solar_expose(W, H, K, s, hz_n, hz_h, T, sector, thr, minutes_w, energy_w, sun, label, P, normal, workspace, minutes, direct,
                             (hipStream_t)stream);
}

extern "C" int adamvs_solar_plane_sums(int W, int H, const int* s, const int* label, long P, const int* minutes, const int* direct, long long* table,
                                       void* stream) {
  if (int rc = solar_check_size(W, H, 8, "solar_plane_sums")) return rc;
  const long n = (long)W * H;
  ADAMVS_CHECK_ARG(s && minutes && direct && table, "solar_plane_sums: null pointer");
  ADAMVS_CHECK_ARG(P >= 0 && P <= ADAMVS_DSM_MAX_CELLS, "solar_plane_sums: P=%ld planes (0 .. %d)", P, ADAMVS_DSM_MAX_CELLS);
  const BldBuffer b[] = {{s, 4 * n}, {minutes, 4 * n}, {direct, 4 * n}, {table, 24 * (P + 1)}, {label, 4 * n}};
  ADAMVS_CHECK_ARG(!bld_any_overlap(b, label ? 5 : 4), "solar_plane_sums: s, label, minutes, direct and the table must not overlap");
  return launch_solar_plane_sums(W, H, s, label, P, minutes, direct, table, (hipStream_t)stream);
}

// ---- TSDF mesh (mesh.hip): every argument is checked here, before any launch
static int mesh_check_brick(const adamvs_mesh_brick* b, const char* what) {
  ADAMVS_CHECK_ARG(b, "%s: null brick", what);
  ADAMVS_CHECK_ARG(b->B == 32 || b->B == 64 || b->B == 128, "%s: B=%d (32, 64 or 128)", what, b->B);
  ADAMVS_CHECK_ARG(std::isfinite(b->voxel) && b->voxel > 0.0, "%s: voxel=%g must be finite and > 0", what, b->voxel);
  ADAMVS_CHECK_ARG(std::isfinite(b->mu) && b->mu > 0.0, "%s: mu=%g must be finite and > 0", what, b->mu);
  ADAMVS_CHECK_ARG(std::isfinite(b->origin[0]) && std::isfinite(b->origin[1]) && std::isfinite(b->origin[2]), "%s: origin not finite",
                   what);
  ADAMVS_CHECK_ARG(b->bx >= 0 && b->by >= 0 && b->bz >= 0, "%s: brick index (%d, %d, %d) < 0", what, b->bx, b->by, b->bz);
  const int bmax = b->bx > b->by ? (b->bx > b->bz ? b->bx : b->bz) : (b->by > b->bz ? b->by : b->bz);
  const double far = ((double)bmax + 1.0) * b->B * b->voxel;
  ADAMVS_CHECK_ARG(far <= ADAMVS_MESH_MAX_EXTENT, "%s: brick (%d, %d, %d) reaches %g m from the origin (at most %g)", what, b->bx, b->by,
                   b->bz, far, ADAMVS_MESH_MAX_EXTENT);
  ADAMVS_CHECK_ARG(b->min_weight >= 1 && b->min_weight <= 65535, "%s: min_weight=%d (1 .. 65535)", what, b->min_weight);
  return 0;
}

extern "C" int adamvs_mesh_check_views(const adamvs_mesh_view* views, int nviews) {
  ADAMVS_CHECK_ARG(views, "mesh_check_views: null pointer");
  ADAMVS_CHECK_ARG(nviews >= 1 && nviews <= ADAMVS_MESH_MAX_VIEWS, "mesh_check_views: nviews=%d (1 .. %d)", nviews, ADAMVS_MESH_MAX_VIEWS);
  for (int i = 0; i < nviews; ++i) {
    const adamvs_mesh_view& v = views[i];
    ADAMVS_CHECK_ARG(v.depth && v.rgba, "mesh_check_views: view %d has a null pointer", i);
    ADAMVS_CHECK_ARG(v.H >= 1 && v.W >= 1, "mesh_check_views: view %d is %d x %d", i, v.H, v.W);
    for (int k = 0; k < 9; ++k)
      ADAMVS_CHECK_ARG(std::isfinite(v.K[k]) && std::isfinite(v.R[k]), "mesh_check_views: view %d: K or R_cw not finite", i);
    ADAMVS_CHECK_ARG(v.K[6] == 0.f && v.K[7] == 0.f && v.K[8] == 1.f, "mesh_check_views: view %d: K's last row is not 0 0 1", i);
    for (int k = 0; k < 3; ++k)
      ADAMVS_CHECK_ARG(std::isfinite(v.c[k]) && std::fabs(v.c[k]) <= ADAMVS_MESH_MAX_EXTENT,
                       "mesh_check_views: view %d: camera %g m from the origin along axis %d (at most %g)", i, (double)v.c[k], k,
                       ADAMVS_MESH_MAX_EXTENT);
  }
  return 0;
}

extern "C" int adamvs_tsdf_integrate(const adamvs_mesh_brick* brick, const adamvs_mesh_view* views, int nviews, const int* view_list,
                                     int nlist, float* tsdf, unsigned short* weight, unsigned* rgba, void* stream) {
  if (int rc = mesh_check_brick(brick, "tsdf_integrate")) return rc;
  ADAMVS_CHECK_ARG(nviews >= 1 && nviews <= ADAMVS_MESH_MAX_VIEWS, "tsdf_integrate: nviews=%d (1 .. %d)", nviews, ADAMVS_MESH_MAX_VIEWS);
  ADAMVS_CHECK_ARG(nlist >= 0 && nlist <= nviews, "tsdf_integrate: nlist=%d (0 .. nviews=%d)", nlist, nviews);
  ADAMVS_CHECK_ARG(views && (view_list || nlist == 0) && tsdf && weight && rgba, "tsdf_integrate: null pointer");
  return launch_tsdf_integrate(*brick, views, nviews, view_list, nlist, tsdf, weight, rgba, (hipStream_t)stream);
}

extern "C" int adamvs_mesh_classify(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned short* weight, unsigned* cube_code,
                                    unsigned* block_tris, void* stream) {
  if (int rc = mesh_check_brick(brick, "mesh_classify")) return rc;
  ADAMVS_CHECK_ARG(tsdf && weight && cube_code && block_tris, "mesh_classify: null pointer");
  return launch_mesh_classify(*brick, tsdf, weight, cube_code, block_tris, (hipStream_t)stream);
}

extern "C" int adamvs_mesh_count_vertices(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned* cube_code,
                                          unsigned char* edge_mask, unsigned* block_verts, void* stream) {
  if (int rc = mesh_check_brick(brick, "mesh_count_vertices")) return rc;
  ADAMVS_CHECK_ARG(tsdf && cube_code && edge_mask && block_verts, "mesh_count_vertices: null pointer");
  return launch_mesh_count_vertices(*brick, tsdf, cube_code, edge_mask, block_verts, (hipStream_t)stream);
}

extern "C" int adamvs_mesh_emit(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned* rgba, const unsigned* cube_code,
                                const unsigned char* edge_mask, const unsigned* vert_offsets, const unsigned* tri_offsets,
                                unsigned vertex_base, double* xyz, unsigned char* rgb, unsigned* first_vertex, long vert_capacity,
                                unsigned* faces, long tri_capacity, void* stream) {
  if (int rc = mesh_check_brick(brick, "mesh_emit")) return rc;
  ADAMVS_CHECK_ARG(tsdf && rgba && cube_code && edge_mask && vert_offsets && tri_offsets && first_vertex, "mesh_emit: null pointer");
  ADAMVS_CHECK_ARG(vert_capacity >= 0 && tri_capacity >= 0, "mesh_emit: capacity < 0");
  ADAMVS_CHECK_ARG((xyz && rgb) || vert_capacity == 0, "mesh_emit: null vertex output");
  ADAMVS_CHECK_ARG(faces || tri_capacity == 0, "mesh_emit: null face output");
  return launch_mesh_emit(*brick, tsdf, rgba, cube_code, edge_mask, vert_offsets, tri_offsets, vertex_base, xyz, rgb, first_vertex,
                          vert_capacity, faces, tri_capacity, (hipStream_t)stream);
}

// ---- the lattice and the counts of mesh simplification and the cloud stages: one check each
static const long SIMPLIFY_MAX = (1L << 31) - 1;

static int check_lattice(const double* origin, double cell, const char* what) {
  ADAMVS_CHECK_ARG(origin, "%s: null origin", what);
  ADAMVS_CHECK_ARG(std::isfinite(cell) && cell > 0, "%s: cell=%g must be finite and > 0", what, cell);
  ADAMVS_CHECK_ARG(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "%s: origin is not finite", what);
  return 0;
}

static int check_count(long n, const char* name, const char* what, long least = 1) {
  ADAMVS_CHECK_ARG(n >= least && n <= SIMPLIFY_MAX, "%s: %s=%ld (%ld .. 2^31 - 1)", what, name, n, least);
  return 0;
}

// ---- mesh simplification (mesh_simplify.hip): every argument is checked here, before any launch
extern "C" int adamvs_simplify_keys(const double* origin, double cell, const double* xyz, long nv, long long* keys, unsigned char* bad,
                                    void* stream) {
  if (int rc = check_lattice(origin, cell, "simplify_keys")) return rc;
  if (int rc = check_count(nv, "nv", "simplify_keys")) return rc;
  ADAMVS_CHECK_ARG(xyz && keys && bad, "simplify_keys: null pointer");
  return launch_simplify_keys(origin, cell, xyz, nv, keys, bad, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_corners(const unsigned* faces, long nf, const int* vcell, long nv, int nc, int* fcell, int* entry_cell,
                                       unsigned char* survive, void* stream) {
  if (int rc = check_count(nf, "nf", "simplify_corners")) return rc;
  if (int rc = check_count(nv, "nv", "simplify_corners")) return rc;
  ADAMVS_CHECK_ARG(nc >= 1 && nc <= nv, "simplify_corners: nc=%d (1 .. nv = %ld)", nc, nv);
  ADAMVS_CHECK_ARG(faces && vcell && fcell && entry_cell && survive, "simplify_corners: null pointer");
  return launch_simplify_corners(faces, nf, vcell, nv, nc, fcell, entry_cell, survive, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_accumulate(const double* origin, double cell, const long long* keys, int nc, const double* xyz,
                                          const unsigned char* rgb, long nv, const unsigned* faces, long nf, const long long* entry,
                                          const long long* fstart, const long long* vorder, const long long* vstart, double* quadric,
                                          double* member, unsigned long long* colour, void* stream) {
  if (int rc = check_lattice(origin, cell, "simplify_accumulate")) return rc;
  if (int rc = check_count(nf, "nf", "simplify_accumulate")) return rc;
  if (int rc = check_count(nv, "nv", "simplify_accumulate")) return rc;
  ADAMVS_CHECK_ARG(nc >= 1 && nc <= nv, "simplify_accumulate: nc=%d (1 .. nv = %ld)", nc, nv);
  ADAMVS_CHECK_ARG(keys && xyz && rgb && faces && entry && fstart && vorder && vstart && quadric && member && colour,
                   "simplify_accumulate: null pointer");
  return launch_simplify_accumulate(origin, cell, keys, nc, xyz, rgb, nv, faces, nf, entry, fstart, vorder, vstart, quadric, member, colour,
                                    (hipStream_t)stream);
}

extern "C" int adamvs_simplify_solve(const double* origin, double cell, double rank_eps, const long long* keys, int nc,
                                     const double* quadric, const double* member, const unsigned long long* colour,
                                     const long long* vstart, double* pos, unsigned char* col, unsigned char* rank, unsigned char* fallback,
                                     double* error, void* stream) {
  if (int rc = check_lattice(origin, cell, "simplify_solve")) return rc;
  if (int rc = check_count(nc, "nc", "simplify_solve")) return rc;
  ADAMVS_CHECK_ARG(rank_eps >= 0 && rank_eps < 1, "simplify_solve: rank_eps=%g (0 <= rank_eps < 1)", rank_eps);
  ADAMVS_CHECK_ARG(keys && quadric && member && colour && vstart && pos && col && rank && fallback && error, "simplify_solve: null pointer");
  return launch_simplify_solve(origin, cell, rank_eps, keys, nc, quadric, member, colour, vstart, pos, col, rank, fallback, error,
                               (hipStream_t)stream);
}

extern "C" int adamvs_simplify_solve_host(const double* quadric, const double* mean, long n, double cell, double rank_eps, double* p,
                                          int* rank, int* fallback, double* error) {
  if (int rc = check_count(n, "n", "simplify_solve_host")) return rc;
  ADAMVS_CHECK_ARG(std::isfinite(cell) && cell > 0, "simplify_solve_host: cell=%g must be finite and > 0", cell);
  ADAMVS_CHECK_ARG(rank_eps >= 0 && rank_eps < 1, "simplify_solve_host: rank_eps=%g (0 <= rank_eps < 1)", rank_eps);
  ADAMVS_CHECK_ARG(quadric && mean && p && rank && fallback && error, "simplify_solve_host: null pointer");
  for (long j = 0; j < n; ++j)
    simplify_solve_host(quadric + 10 * j, mean + 3 * j, cell, rank_eps, p + 3 * j, rank + j, fallback + j, error + j);
  return 0;
}

extern "C" int adamvs_simplify_triples(const int* fcell, long nf, const long long* surv, long ns, int* tri, void* stream) {
  if (int rc = check_count(nf, "nf", "simplify_triples")) return rc;
  ADAMVS_CHECK_ARG(ns >= 1 && ns <= nf, "simplify_triples: ns=%ld (1 .. nf = %ld)", ns, nf);
  ADAMVS_CHECK_ARG(fcell && surv && tri, "simplify_triples: null pointer");
  return launch_simplify_triples(fcell, nf, surv, ns, tri, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_first(const int* tri, const long long* surv, const long long* order, long ns, long nf, unsigned char* keep,
                                     void* stream) {
  if (int rc = check_count(nf, "nf", "simplify_first")) return rc;
  ADAMVS_CHECK_ARG(ns >= 1 && ns <= nf, "simplify_first: ns=%ld (1 .. nf = %ld)", ns, nf);
  ADAMVS_CHECK_ARG(tri && surv && order && keep, "simplify_first: null pointer");
  return launch_simplify_first(tri, surv, order, ns, nf, keep, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_mark(const int* fcell, const unsigned char* keep, long nf, int nc, unsigned char* used, void* stream) {
  if (int rc = check_count(nf, "nf", "simplify_mark")) return rc;
  if (int rc = check_count(nc, "nc", "simplify_mark")) return rc;
  ADAMVS_CHECK_ARG(fcell && keep && used, "simplify_mark: null pointer");
  return launch_simplify_mark(fcell, keep, nf, nc, used, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_count(const unsigned char* flags, long n, unsigned* block_count, void* stream) {
  if (int rc = check_count(n, "n", "simplify_count")) return rc;
  ADAMVS_CHECK_ARG(flags && block_count, "simplify_count: null pointer");
  return launch_simplify_count(flags, n, block_count, (hipStream_t)stream);
}

extern "C" int adamvs_simplify_emit(const double* pos, const unsigned char* col, const unsigned char* used, int nc,
                                    const unsigned* cell_offsets, const int* fcell, const unsigned char* keep, long nf,
                                    const unsigned* face_offsets, double* xyz, unsigned char* rgb, unsigned* new_index, long vert_capacity,
                                    unsigned* faces, long face_capacity, void* stream) {
  if (int rc = check_count(nf, "nf", "simplify_emit")) return rc;
  if (int rc = check_count(nc, "nc", "simplify_emit")) return rc;
  ADAMVS_CHECK_ARG(pos && col && used && cell_offsets && fcell && keep && face_offsets && new_index, "simplify_emit: null pointer");
  ADAMVS_CHECK_ARG(vert_capacity >= 0 && face_capacity >= 0, "simplify_emit: capacity < 0");
  ADAMVS_CHECK_ARG((xyz && rgb) || vert_capacity == 0, "simplify_emit: null vertex output");
  ADAMVS_CHECK_ARG(faces || face_capacity == 0, "simplify_emit: null face output");
  return launch_simplify_emit(pos, col, used, nc, cell_offsets, fcell, keep, nf, face_offsets, xyz, rgb, new_index, vert_capacity, faces,
                              face_capacity, (hipStream_t)stream);
}

// ---- mesh smoothing (mesh_smooth.hip): every argument is checked here, before any launch
static const long SMOOTH_MAX_FACES = ((1L << 31) - 1) / 3;      // the 3 nf (vertex, face) entries are counted in 31 bits

static int smooth_check_counts(long nv, long nf, const char* what) {
  ADAMVS_CHECK_ARG(nv >= 1 && nv <= SIMPLIFY_MAX, "%s: nv=%ld (1 .. 2^31 - 1)", what, nv);
  ADAMVS_CHECK_ARG(nf >= 1 && nf <= SMOOTH_MAX_FACES, "%s: nf=%ld (1 .. (2^31 - 1) / 3)", what, nf);
  return 0;
}

extern "C" int adamvs_smooth_faces(const double* p, long nv, const unsigned* faces, long nf, double* rec, void* stream) {
  if (int rc = smooth_check_counts(nv, nf, "smooth_faces")) return rc;
  ADAMVS_CHECK_ARG(p && faces && rec, "smooth_faces: null pointer");
  ADAMVS_CHECK_ARG(((uintptr_t)rec & 63) == 0, "smooth_faces: rec is not aligned to 64 bytes");
  return launch_smooth_faces(p, nv, faces, nf, rec, (hipStream_t)stream);
}

extern "C" int adamvs_smooth_edge_keys(const unsigned* faces, long nf, long long* keys, void* stream) {
  if (int rc = smooth_check_counts(1, nf, "smooth_edge_keys")) return rc;
  ADAMVS_CHECK_ARG(faces && keys, "smooth_edge_keys: null pointer");
  return launch_mesh_edge_keys(faces, nf, keys, "smooth_edge_keys", (hipStream_t)stream);
}

extern "C" int adamvs_smooth_boundary(const long long* keys, long n, long nv, unsigned char* fixed, void* stream) {
  ADAMVS_CHECK_ARG(n >= 1 && n <= SIMPLIFY_MAX, "smooth_boundary: n=%ld (1 .. 2^31 - 1)", n);
  ADAMVS_CHECK_ARG(nv >= 1 && nv <= SIMPLIFY_MAX, "smooth_boundary: nv=%ld (1 .. 2^31 - 1)", nv);
  ADAMVS_CHECK_ARG(keys && fixed, "smooth_boundary: null pointer");
  return launch_smooth_boundary(keys, n, nv, fixed, (hipStream_t)stream);
}

extern "C" int adamvs_smooth_filter(const double* rec, const double* nin, double* nout, const unsigned* faces, long nf, long nv,
                                    const int* vface, const long long* vstart, double sigma_s, double sigma_r, void* stream) {
  if (int rc = smooth_check_counts(nv, nf, "smooth_filter")) return rc;
  ADAMVS_CHECK_ARG(std::isfinite(sigma_s) && sigma_s > 0, "smooth_filter: sigma_s=%g must be finite and > 0", sigma_s);
  ADAMVS_CHECK_ARG(std::isfinite(sigma_r) && sigma_r > 0, "smooth_filter: sigma_r=%g must be finite and > 0", sigma_r);
  ADAMVS_CHECK_ARG(rec && nin && nout && faces && vface && vstart, "smooth_filter: null pointer");
  ADAMVS_CHECK_ARG(nin != nout, "smooth_filter: the normals are double-buffered, nin == nout");
  ADAMVS_CHECK_ARG(((uintptr_t)rec & 63) == 0, "smooth_filter: rec is not aligned to 64 bytes");
  return launch_smooth_filter(rec, nin, nout, faces, nf, nv, vface, vstart, sigma_s, sigma_r, (hipStream_t)stream);
}

extern "C" int adamvs_smooth_centroids(const double* p, long nv, const unsigned* faces, long nf, double* cen, void* stream) {
  if (int rc = smooth_check_counts(nv, nf, "smooth_centroids")) return rc;
  ADAMVS_CHECK_ARG(p && faces && cen, "smooth_centroids: null pointer");
  return launch_smooth_centroids(p, nv, faces, nf, cen, (hipStream_t)stream);
}

extern "C" int adamvs_smooth_update(const double* p0, const double* p, double* pout, long nv, const double* nrm, const double* cen,
                                    long nf, const int* vface, const long long* vstart, const unsigned char* fixed, double cap,
                                    unsigned char* clamped, void* stream) {
  if (int rc = smooth_check_counts(nv, nf, "smooth_update")) return rc;
  ADAMVS_CHECK_ARG(std::isfinite(cap) && cap > 0, "smooth_update: cap=%g must be finite and > 0", cap);
  ADAMVS_CHECK_ARG(p0 && p && pout && nrm && cen && vface && vstart && fixed && clamped, "smooth_update: null pointer");
  ADAMVS_CHECK_ARG(p != pout && p0 != pout, "smooth_update: the positions are double-buffered, pout aliases an input");
  return launch_smooth_update(p0, p, pout, nv, nrm, cen, nf, vface, vstart, fixed, cap, clamped, (hipStream_t)stream);
}

// ---- mesh cleaning (mesh_clean.hip): every argument is checked here, before any launch; the limits are smoothing's
extern "C" int adamvs_clean_components(const unsigned* faces, long nf, long nv, const int* parent_in, int* parent_out, unsigned* changed,
                                       void* stream) {
  if (int rc = smooth_check_counts(nv, nf, "clean_components")) return rc;
  ADAMVS_CHECK_ARG(faces && parent_in && parent_out && changed, "clean_components: null pointer");
  ADAMVS_CHECK_ARG(parent_in != parent_out, "clean_components: the labels are double-buffered, parent_in == parent_out");
  return launch_clean_components(faces, nf, nv, parent_in, parent_out, changed, (hipStream_t)stream);
}

extern "C" int adamvs_clean_area(const double* area, long nf, const long long* order, const long long* seg_of, const long long* seg_start,
                                 long ncomp, double* lead, double* first, double* out, void* stream) {
  if (int rc = smooth_check_counts(1, nf, "clean_area")) return rc;
  ADAMVS_CHECK_ARG(ncomp >= 1 && ncomp <= nf, "clean_area: ncomp=%ld (1 .. nf = %ld)", ncomp, nf);
  ADAMVS_CHECK_ARG(area && order && seg_of && seg_start && lead && first && out, "clean_area: null pointer");
  ADAMVS_CHECK_ARG(lead != first && lead != out && first != out && area != out && area != lead && area != first, "clean_area: aliased buffers");
  return launch_clean_area(area, nf, order, seg_of, seg_start, ncomp, lead, first, out, (hipStream_t)stream);
}

extern "C" int adamvs_clean_boundary(const long long* keys_sorted, const long long* entry, long ns, unsigned char* bnd, void* stream) {
  if (int rc = smooth_check_counts(1, ns, "clean_boundary")) return rc;
  ADAMVS_CHECK_ARG(keys_sorted && entry && bnd, "clean_boundary: null pointer");
  ADAMVS_CHECK_ARG(keys_sorted != entry, "clean_boundary: keys_sorted == entry");
  return launch_clean_boundary(keys_sorted, entry, 3 * ns, bnd, (hipStream_t)stream);
}

extern "C" int adamvs_clean_successor(const unsigned* faces, long ns, long nv, const unsigned char* bnd, int* out_count, int* in_count,
                                      int* out_edge, int* succ, int* lab, int* nxt, unsigned char* broken, void* stream) {
  if (int rc = smooth_check_counts(nv, ns, "clean_successor")) return rc;
  ADAMVS_CHECK_ARG(faces && bnd && out_count && in_count && out_edge && succ && lab && nxt && broken, "clean_successor: null pointer");
  ADAMVS_CHECK_ARG(out_count != in_count && out_count != out_edge && in_count != out_edge && succ != lab && succ != nxt && lab != nxt &&
                   bnd != broken, "clean_successor: aliased buffers");
  return launch_clean_successor(faces, ns, nv, bnd, out_count, in_count, out_edge, succ, lab, nxt, broken, (hipStream_t)stream);
}

extern "C" int adamvs_clean_double(const unsigned char* bnd, long ns, const int* lab_in, const int* nxt_in, const unsigned char* broken_in,
                                   int* lab_out, int* nxt_out, unsigned char* broken_out, void* stream) {
  if (int rc = smooth_check_counts(1, ns, "clean_double")) return rc;
  ADAMVS_CHECK_ARG(bnd && lab_in && nxt_in && broken_in && lab_out && nxt_out && broken_out, "clean_double: null pointer");
  ADAMVS_CHECK_ARG(lab_in != lab_out && nxt_in != nxt_out && broken_in != broken_out && lab_out != nxt_out && lab_out != nxt_in &&
                   nxt_out != lab_in && bnd != broken_out, "clean_double: the round is double-buffered, an output aliases an input");
  return launch_clean_double(bnd, 3 * ns, lab_in, nxt_in, broken_in, lab_out, nxt_out, broken_out, (hipStream_t)stream);
}

extern "C" int adamvs_clean_validate(const unsigned char* bnd, const int* succ, const int* lab, const unsigned char* broken, long ns,
                                     int max_hole_edges, int* count, unsigned char* bad, int* loop, unsigned char* closed, void* stream) {
  if (int rc = smooth_check_counts(1, ns, "clean_validate")) return rc;
  ADAMVS_CHECK_ARG(max_hole_edges >= 0 && max_hole_edges <= ADAMVS_CLEAN_MAX_HOLE_EDGES, "clean_validate: max_hole_edges=%d (0 .. %d)",
                   max_hole_edges, ADAMVS_CLEAN_MAX_HOLE_EDGES);
  ADAMVS_CHECK_ARG(bnd && succ && lab && broken && count && bad && loop && closed, "clean_validate: null pointer");
  ADAMVS_CHECK_ARG(count != loop && count != succ && count != lab && loop != succ && loop != lab && bad != closed && bad != bnd &&
                   bad != broken && closed != bnd && closed != broken, "clean_validate: aliased buffers");
  return launch_clean_validate(bnd, succ, lab, broken, 3 * ns, max_hole_edges, count, bad, loop, closed, (hipStream_t)stream);
}

extern "C" int adamvs_clean_accumulate(const double* p, const unsigned char* rgb, long nv, const unsigned* faces, long ns, const int* members,
                                       long nm, const long long* start, long nl, const double* origin, double* centre,
                                       unsigned char* colour, void* stream) {
  if (int rc = smooth_check_counts(nv, ns, "clean_accumulate")) return rc;
  ADAMVS_CHECK_ARG(nl >= 1 && nl <= ns, "clean_accumulate: nl=%ld (1 .. ns = %ld)", nl, ns);
  ADAMVS_CHECK_ARG(nm >= 3 * nl && nm <= 3 * ns, "clean_accumulate: nm=%ld members (3 nl = %ld .. 3 ns = %ld)", nm, 3 * nl, 3 * ns);
  ADAMVS_CHECK_ARG(p && rgb && faces && members && start && origin && centre && colour, "clean_accumulate: null pointer");
  ADAMVS_CHECK_ARG(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), "clean_accumulate: the origin is not finite");
  ADAMVS_CHECK_ARG(p != centre && rgb != colour, "clean_accumulate: aliased buffers");
  return launch_clean_accumulate(p, rgb, nv, faces, ns, members, start, nl, nm, origin, centre, colour, (hipStream_t)stream);
}

extern "C" int adamvs_clean_emit(const double* xyz, const unsigned char* rgb, long nv, const int* new_index, const unsigned* faces, long ns,
                                 const int* fill_edge, const int* loop_of, long nfill, const double* centre, const unsigned char* colour,
                                 long nl, long nvs, double* xyz_out, unsigned char* rgb_out, unsigned* faces_out, void* stream) {
  if (int rc = smooth_check_counts(nv, ns, "clean_emit")) return rc;
  ADAMVS_CHECK_ARG(nvs >= 1 && nvs <= nv, "clean_emit: nvs=%ld (1 .. nv = %ld)", nvs, nv);
  ADAMVS_CHECK_ARG(nl >= 0 && nl <= ns && nfill >= 0 && nfill <= 3 * ns && (nl == 0) == (nfill == 0) && nfill >= 3 * nl,
                   "clean_emit: nl=%ld loops, nfill=%ld fill faces", nl, nfill);
  ADAMVS_CHECK_ARG(nvs + nl <= SIMPLIFY_MAX && ns + nfill <= SMOOTH_MAX_FACES, "clean_emit: the output exceeds 2^31 - 1 vertices or (2^31 - 1) / 3 faces");
  ADAMVS_CHECK_ARG(xyz && rgb && new_index && faces && xyz_out && rgb_out && faces_out, "clean_emit: null pointer");
  ADAMVS_CHECK_ARG(nl == 0 || (fill_edge && loop_of && centre && colour), "clean_emit: null fill input");
  ADAMVS_CHECK_ARG(xyz != xyz_out && rgb != rgb_out && faces != faces_out && centre != xyz_out && colour != rgb_out, "clean_emit: aliased buffers");
  return launch_clean_emit(xyz, rgb, nv, new_index, faces, ns, fill_edge, loop_of, nfill, centre, colour, nl, nvs, xyz_out, rgb_out, faces_out,
                           (hipStream_t)stream);
}

// ---- cloud distance (cloud_dist.hip): every argument is checked here, before any launch
extern "C" int adamvs_cloud_nearest(const double* origin, double D, const long long* ukeys, const long long* tstart, int nc,
                                    const double* targets, const int* tindex, long nt, const double* queries, long nq,
                                    const long long* qorder, long nqs, const long long* item_key, const long long* item_first,
                                    const int* item_count, long ni, float* d2, int* index, unsigned long long* pairs, void* stream) {
  if (int rc = check_lattice(origin, D, "cloud_nearest")) return rc;
  if (int rc = check_count(nt, "nt", "cloud_nearest")) return rc;
  if (int rc = check_count(nq, "nq", "cloud_nearest")) return rc;
  if (int rc = check_count(nqs, "nqs", "cloud_nearest")) return rc;
  if (int rc = check_count(ni, "ni", "cloud_nearest")) return rc;
  ADAMVS_CHECK_ARG(nc >= 1 && nc <= nt, "cloud_nearest: nc=%d (1 .. nt = %ld)", nc, nt);
  ADAMVS_CHECK_ARG(nqs <= nq && ni <= nqs, "cloud_nearest: nqs=%ld, ni=%ld (ni <= nqs <= nq = %ld)", nqs, ni, nq);
  ADAMVS_CHECK_ARG(ukeys && tstart && targets && tindex && queries && qorder && item_key && item_first && item_count && d2 && index && pairs,
                   "cloud_nearest: null pointer");
  return launch_cloud_nearest(origin, D, ukeys, tstart, nc, targets, tindex, nt, queries, nq, qorder, nqs, item_key, item_first, item_count,
                              ni, d2, index, pairs, (hipStream_t)stream);
}

extern "C" int adamvs_cloud_nearest_host(const double* origin, double D, const double* targets, long nt, const double* queries, long nq,
                                         float* d2, int* index, unsigned long long* pairs) {
  if (int rc = check_lattice(origin, D, "cloud_nearest_host")) return rc;
  if (int rc = check_count(nt, "nt", "cloud_nearest_host")) return rc;
  if (int rc = check_count(nq, "nq", "cloud_nearest_host")) return rc;
  ADAMVS_CHECK_ARG(targets && queries && d2 && index, "cloud_nearest_host: null pointer");
  return cloud_nearest_host(origin, D, targets, nt, queries, nq, d2, index, pairs);
}

extern "C" int adamvs_cloud_sample_count(const double* xyz, long nv, const unsigned* faces, long nf, double spacing, int* subdiv,
                                         void* stream) {
  if (int rc = check_count(nv, "nv", "cloud_sample_count")) return rc;
  if (int rc = check_count(nf, "nf", "cloud_sample_count")) return rc;
  ADAMVS_CHECK_ARG(std::isfinite(spacing) && spacing > 0, "cloud_sample_count: spacing=%g must be finite and > 0", spacing);
  ADAMVS_CHECK_ARG(xyz && faces && subdiv, "cloud_sample_count: null pointer");
  return launch_cloud_sample_count(xyz, nv, faces, nf, spacing, subdiv, (hipStream_t)stream);
}

extern "C" int adamvs_cloud_sample_emit(const double* xyz, long nv, const unsigned* faces, long nf, const int* subdiv,
                                        const long long* offsets, double* points, long capacity, void* stream) {
  if (int rc = check_count(nv, "nv", "cloud_sample_emit")) return rc;
  if (int rc = check_count(nf, "nf", "cloud_sample_emit")) return rc;
  ADAMVS_CHECK_ARG(nf <= SIMPLIFY_MAX / 64, "cloud_sample_emit: nf=%ld (one wave per face: at most (2^31 - 1) / 64)", nf);
  ADAMVS_CHECK_ARG(capacity >= 0, "cloud_sample_emit: capacity < 0");
  ADAMVS_CHECK_ARG(xyz && faces && subdiv && offsets && (points || capacity == 0), "cloud_sample_emit: null pointer");
  return launch_cloud_sample_emit(xyz, nv, faces, nf, subdiv, offsets, points, capacity, (hipStream_t)stream);
}

// ---- cloud neighbourhoods (cloud_knn.hip): every argument is checked here, before any launch
static int knn_check_k(int k, const char* what) {
  ADAMVS_CHECK_ARG(k >= 1 && k <= ADAMVS_KNN_MAX_K, "%s: k=%d (1 .. %d)", what, k, ADAMVS_KNN_MAX_K);
  return 0;
}

extern "C" int adamvs_knn_search(const double* origin, double R, int k, const long long* ukeys, const long long* tstart, int nc,
                                 const double* sorted, const int* pindex, long n, const long long* item_key, const long long* item_first,
                                 const int* item_count, long ni, long long row_base, long rows, float* d2, int* index, int* count,
                                 unsigned long long* pairs, void* stream) {
  if (int rc = check_lattice(origin, R, "knn_search")) return rc;
  if (int rc = knn_check_k(k, "knn_search")) return rc;
  if (int rc = check_count(n, "n", "knn_search")) return rc;
  if (int rc = check_count(ni, "ni", "knn_search")) return rc;
  if (int rc = check_count(rows, "rows", "knn_search")) return rc;
  ADAMVS_CHECK_ARG(nc >= 1 && nc <= n, "knn_search: nc=%d (1 .. n = %ld)", nc, n);
  ADAMVS_CHECK_ARG(ni <= n && rows <= n && row_base >= 0 && row_base <= n - rows, "knn_search: ni=%ld, rows=%ld from row_base=%lld (within n = %ld)",
                   ni, rows, row_base, n);
  ADAMVS_CHECK_ARG(ukeys && tstart && sorted && pindex && item_key && item_first && item_count && d2 && index && count && pairs,
                   "knn_search: null pointer");
  return launch_knn_search(origin, R, k, ukeys, tstart, nc, sorted, pindex, n, item_key, item_first, item_count, ni, row_base, rows, d2, index,
                           count, pairs, (hipStream_t)stream);
}

extern "C" int adamvs_knn_search_host(const double* origin, double R, int k, const double* points, long n, float* d2, int* index, int* count,
                                      unsigned long long* pairs) {
  if (int rc = check_lattice(origin, R, "knn_search_host")) return rc;
  if (int rc = knn_check_k(k, "knn_search_host")) return rc;
  if (int rc = check_count(n, "n", "knn_search_host")) return rc;
  ADAMVS_CHECK_ARG(points && d2 && index && count, "knn_search_host: null pointer");
  return knn_search_host(origin, R, k, points, n, d2, index, count, pairs);
}

extern "C" int adamvs_knn_normals(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                                  double* normal, float* curvature, unsigned char* flag, void* stream) {
  if (int rc = knn_check_k(k, "knn_normals")) return rc;
  if (int rc = check_count(n, "n", "knn_normals")) return rc;
  if (int rc = check_count(rows, "rows", "knn_normals")) return rc;
  ADAMVS_CHECK_ARG(points && index && count && normal && curvature && flag, "knn_normals: null pointer");
  return launch_knn_normals(points, n, index, count, k, rows, row_point, normal, curvature, flag, (hipStream_t)stream);
}

extern "C" int adamvs_knn_normals_host(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                                       double* normal, float* curvature, unsigned char* flag) {
  if (int rc = knn_check_k(k, "knn_normals_host")) return rc;
  if (int rc = check_count(n, "n", "knn_normals_host")) return rc;
  if (int rc = check_count(rows, "rows", "knn_normals_host")) return rc;
  ADAMVS_CHECK_ARG(points && index && count && normal && curvature && flag, "knn_normals_host: null pointer");
  return knn_normals_host(points, n, index, count, k, rows, row_point, normal, curvature, flag);
}

// ---- cloud registration (cloud_register.hip): every argument is checked here, before any launch
static int register_check_motion(const double* R, const double* c, const double* u, const char* what) {
  ADAMVS_CHECK_ARG(R && c && u, "%s: null R, c or u", what);
  for (int k = 0; k < 9; ++k) ADAMVS_CHECK_ARG(std::isfinite(R[k]), "%s: R is not finite", what);
  for (int k = 0; k < 3; ++k) ADAMVS_CHECK_ARG(std::isfinite(c[k]) && std::isfinite(u[k]), "%s: c or u is not finite", what);
  return 0;
}

static int register_check_frame(const double* c, double L, double delta, const char* what) {
  ADAMVS_CHECK_ARG(c && std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]), "%s: the pivot c is null or not finite", what);
  ADAMVS_CHECK_ARG(std::isfinite(L) && L > 0, "%s: L=%g must be finite and > 0", what, L);
  ADAMVS_CHECK_ARG(!std::isnan(delta), "%s: delta is NaN (<= 0: Huber off)", what);
  return 0;
}

extern "C" int adamvs_rigid_apply(const double* R, const double* c, const double* u, const double* x, long n, double* y, void* stream) {
  if (int rc = register_check_motion(R, c, u, "rigid_apply")) return rc;
  if (int rc = check_count(n, "n", "rigid_apply", 0)) return rc;
  ADAMVS_CHECK_ARG((x && y) || n == 0, "rigid_apply: null pointer");
  return launch_rigid_apply(R, c, u, x, n, y, (hipStream_t)stream);
}

extern "C" int adamvs_rigid_apply_host(const double* R, const double* c, const double* u, const double* x, long n, double* y) {
  if (int rc = register_check_motion(R, c, u, "rigid_apply_host")) return rc;
  if (int rc = check_count(n, "n", "rigid_apply_host", 0)) return rc;
  ADAMVS_CHECK_ARG((x && y) || n == 0, "rigid_apply_host: null pointer");
  return rigid_apply_host(R, c, u, x, n, y);
}

extern "C" int adamvs_icp_accumulate(const double* y, const int* index, long nq, const double* targets, const double* normals,
                                     const unsigned char* flag, long nt, const double* c, double L, double delta, double* partial,
                                     void* stream) {
  if (int rc = register_check_frame(c, L, delta, "icp_accumulate")) return rc;
  if (int rc = check_count(nq, "nq", "icp_accumulate", 0)) return rc;
  if (int rc = check_count(nt, "nt", "icp_accumulate", 0)) return rc;
  ADAMVS_CHECK_ARG((y && index && partial) || nq == 0, "icp_accumulate: null pointer");
  ADAMVS_CHECK_ARG((targets && normals && flag) || nt == 0, "icp_accumulate: null pointer");
  return launch_icp_accumulate(y, index, nq, targets, normals, flag, nt, c, L, delta, partial, (hipStream_t)stream);
}

extern "C" int adamvs_icp_accumulate_host(const double* y, const int* index, long nq, const double* targets, const double* normals,
                                          const unsigned char* flag, long nt, const double* c, double L, double delta, double* partial) {
  if (int rc = register_check_frame(c, L, delta, "icp_accumulate_host")) return rc;
  if (int rc = check_count(nq, "nq", "icp_accumulate_host", 0)) return rc;
  if (int rc = check_count(nt, "nt", "icp_accumulate_host", 0)) return rc;
  ADAMVS_CHECK_ARG((y && index && partial) || nq == 0, "icp_accumulate_host: null pointer");
  ADAMVS_CHECK_ARG((targets && normals && flag) || nt == 0, "icp_accumulate_host: null pointer");
  return icp_accumulate_host(y, index, nq, targets, normals, flag, nt, c, L, delta, partial);
}

extern "C" int adamvs_icp_reduce(const double* partial, long nb, double* sums, void* stream) {
  if (int rc = check_count(nb, "nb", "icp_reduce", 0)) return rc;
  ADAMVS_CHECK_ARG((partial || nb == 0) && sums, "icp_reduce: null pointer");
  return launch_icp_reduce(partial, nb, sums, (hipStream_t)stream);
}

extern "C" int adamvs_icp_reduce_host(const double* partial, long nb, double* sums) {
  if (int rc = check_count(nb, "nb", "icp_reduce_host", 0)) return rc;
  ADAMVS_CHECK_ARG((partial || nb == 0) && sums, "icp_reduce_host: null pointer");
  return icp_reduce_host(partial, nb, sums);
}

// ---- image orthophoto (ortho.hip): every argument is checked here, before any launch
static int ortho_check_grid(const adamvs_ortho_grid* g, const char* what) {
  ADAMVS_CHECK_ARG(g, "%s: null grid", what);
  ADAMVS_CHECK_ARG(g->W >= 1 && g->H >= 1, "%s: grid %d x %d", what, g->W, g->H);
  ADAMVS_CHECK_ARG(g->K >= 1 && g->K <= ADAMVS_ORTHO_MAX_UPSAMPLE, "%s: upsample K=%d (1 .. %d)", what, g->K, ADAMVS_ORTHO_MAX_UPSAMPLE);
  ADAMVS_CHECK_ARG((long)g->W * g->K * (long)g->H * g->K <= ADAMVS_ORTHO_MAX_CELLS, "%s: %d x %d cells at K=%d exceed %ld", what, g->W,
                   g->H, g->K, (long)ADAMVS_ORTHO_MAX_CELLS);
  ADAMVS_CHECK_ARG(std::isfinite(g->x0) && std::isfinite(g->y_top) && std::isfinite(g->gsd) && g->gsd > 0.0,
                   "%s: x0 %g, y_top %g, gsd %g (finite, gsd > 0)", what, g->x0, g->y_top, g->gsd);
  return 0;
}

static int ortho_check_view(const adamvs_ortho_view* v, const char* what) {
  ADAMVS_CHECK_ARG(v && v->rgba, "%s: null view or image", what);
  ADAMVS_CHECK_ARG(v->H >= 1 && v->W >= 1, "%s: image %d x %d", what, v->H, v->W);
  for (int k = 0; k < 9; ++k)
    ADAMVS_CHECK_ARG(std::isfinite(v->K[k]) && std::isfinite(v->R[k]), "%s: K or R_cw not finite", what);
  for (int k = 0; k < 3; ++k) ADAMVS_CHECK_ARG(std::isfinite(v->C[k]), "%s: C not finite", what);
  ADAMVS_CHECK_ARG(v->K[6] == 0.f && v->K[7] == 0.f && v->K[8] == 1.f, "%s: K's last row is not 0 0 1", what);
  return 0;
}

extern "C" int adamvs_ortho_surface(const adamvs_ortho_grid* grid, const float* dsm, double* height, void* stream) {
  if (int rc = ortho_check_grid(grid, "ortho_surface")) return rc;
  ADAMVS_CHECK_ARG(dsm && height, "ortho_surface: null pointer");
  return launch_ortho_surface(*grid, dsm, height, (hipStream_t)stream);
}

extern "C" int adamvs_ortho_zbuf(const adamvs_ortho_grid* grid, const float* dsm, const adamvs_ortho_view* view, unsigned* zbuf,
                                 unsigned* big_count, unsigned* big_list, long big_capacity, void* stream) {
  if (int rc = ortho_check_grid(grid, "ortho_zbuf")) return rc;
  if (int rc = ortho_check_view(view, "ortho_zbuf")) return rc;
  ADAMVS_CHECK_ARG(dsm && zbuf && big_count && big_list, "ortho_zbuf: null pointer");
  const long need = 2L * (grid->W - 1) * (grid->H - 1);
  ADAMVS_CHECK_ARG(big_capacity >= need, "ortho_zbuf: big_capacity %ld < 2 (W-1)(H-1) = %ld", big_capacity, need);
  return launch_ortho_zbuf(*grid, dsm, *view, zbuf, big_count, big_list, (hipStream_t)stream);
}

extern "C" int adamvs_ortho_compose(const adamvs_ortho_grid* grid, const adamvs_ortho_view* view, int view_id, const double* height,
                                    const unsigned* zbuf, int mode, float border, float feather_px, float occlusion_tol, float* acc,
                                    float* wmax, int* view_state, int* nvis, void* stream) {
  if (int rc = ortho_check_grid(grid, "ortho_compose")) return rc;
  if (int rc = ortho_check_view(view, "ortho_compose")) return rc;
  ADAMVS_CHECK_ARG(height && zbuf && acc && wmax && view_state && nvis, "ortho_compose: null pointer");
  ADAMVS_CHECK_ARG(mode == ADAMVS_ORTHO_BEST || mode == ADAMVS_ORTHO_FEATHER, "ortho_compose: mode=%d", mode);
  ADAMVS_CHECK_ARG(std::isfinite(border) && border >= 0.f, "ortho_compose: border=%g (finite, >= 0)", (double)border);
  ADAMVS_CHECK_ARG(std::isfinite(feather_px) && feather_px > 0.f, "ortho_compose: feather_px=%g (finite, > 0)", (double)feather_px);
  ADAMVS_CHECK_ARG(std::isfinite(occlusion_tol) && occlusion_tol >= 0.f, "ortho_compose: occlusion_tol=%g (finite, >= 0)",
                   (double)occlusion_tol);
  return launch_ortho_compose(*grid, *view, view_id, height, zbuf, mode, border, feather_px, occlusion_tol, acc, wmax, view_state, nvis,
                              (hipStream_t)stream);
}

extern "C" int adamvs_ortho_finalize(const adamvs_ortho_grid* grid, const float* acc, const int* view_state, const int* nvis,
                                     unsigned char* rgba, int* view_out, unsigned short* nvis_out, void* stream) {
  if (int rc = ortho_check_grid(grid, "ortho_finalize")) return rc;
  ADAMVS_CHECK_ARG(acc && view_state && nvis && rgba && view_out && nvis_out, "ortho_finalize: null pointer");
  return launch_ortho_finalize(*grid, acc, view_state, nvis, rgba, view_out, nvis_out, (hipStream_t)stream);
}

// ---- image orthophoto, radiometric balance (ortho_balance.hip): every argument is checked here, before any launch
extern "C" int adamvs_ortho_observe(const adamvs_ortho_grid* grid, const float* dsm, const adamvs_ortho_view* view, const unsigned* zbuf,
                                    int S, float border, float occlusion_tol, unsigned short* obs, void* stream) {
  ADAMVS_CHECK_ARG(grid, "ortho_observe: null grid");
  adamvs_ortho_grid g = *grid;
  g.K = 1;                                                          // the lattice samples the DSM's own cells
  if (int rc = ortho_check_grid(&g, "ortho_observe")) return rc;
  if (int rc = ortho_check_view(view, "ortho_observe")) return rc;
  ADAMVS_CHECK_ARG(dsm && zbuf && obs, "ortho_observe: null pointer");
  ADAMVS_CHECK_ARG(S >= 1, "ortho_observe: stride S=%d (>= 1)", S);
  const long ns = (long)((g.W + (long)S - 1) / S) * ((g.H + (long)S - 1) / S);
  ADAMVS_CHECK_ARG(ns <= ADAMVS_ORTHO_BAL_MAX_SAMPLES, "ortho_observe: %ld lattice cells at S=%d exceed %ld", ns, S,
                   (long)ADAMVS_ORTHO_BAL_MAX_SAMPLES);
  ADAMVS_CHECK_ARG(std::isfinite(border) && border >= 0.f, "ortho_observe: border=%g (finite, >= 0)", (double)border);
  ADAMVS_CHECK_ARG(std::isfinite(occlusion_tol) && occlusion_tol >= 0.f, "ortho_observe: occlusion_tol=%g (finite, >= 0)",
                   (double)occlusion_tol);
  return launch_ortho_observe(g, dsm, *view, zbuf, S, border, occlusion_tol, obs, (hipStream_t)stream);
}

extern "C" int adamvs_ortho_pair_stats(const unsigned short* obs, int V, long N_s, const int* pairs, int P, int max_diff_q,
                                       long long* stats, void* stream) {
  ADAMVS_CHECK_ARG(V >= 1 && P >= 0, "ortho_pair_stats: V=%d (>= 1), P=%d (>= 0)", V, P);
  ADAMVS_CHECK_ARG(N_s >= 1 && N_s <= ADAMVS_ORTHO_BAL_MAX_SAMPLES, "ortho_pair_stats: N_s=%ld (1 .. %ld)", N_s,
                   (long)ADAMVS_ORTHO_BAL_MAX_SAMPLES);
  ADAMVS_CHECK_ARG(max_diff_q >= 0 && max_diff_q <= ADAMVS_ORTHO_BAL_MAX_Q, "ortho_pair_stats: max_diff_q=%d (0 .. %d)", max_diff_q,
                   ADAMVS_ORTHO_BAL_MAX_Q);
  const long nchunk = (N_s + ADAMVS_ORTHO_BAL_CHUNK - 1) / ADAMVS_ORTHO_BAL_CHUNK;
  ADAMVS_CHECK_ARG(nchunk * P < (1L << 31), "ortho_pair_stats: %d pairs of %ld chunks exceed 2^31 workgroups", P, nchunk);
  if (P == 0) return 0;
  ADAMVS_CHECK_ARG(obs && pairs && stats, "ortho_pair_stats: null pointer");
  return launch_ortho_pair_stats(obs, N_s, pairs, P, max_diff_q, stats, (hipStream_t)stream);
}

extern "C" int adamvs_ortho_adjust_image(const unsigned char* rgba_in, int H, int W, const float* gain, unsigned char* rgba_out,
                                         void* stream) {
  ADAMVS_CHECK_ARG(rgba_in && gain && rgba_out, "ortho_adjust_image: null pointer");
  ADAMVS_CHECK_ARG(rgba_in != rgba_out, "ortho_adjust_image: rgba_out may not alias rgba_in");
  ADAMVS_CHECK_ARG(H >= 1 && W >= 1 && (long)H * W <= ADAMVS_ORTHO_MAX_CELLS, "ortho_adjust_image: image %d x %d", H, W);
  for (int k = 0; k < 3; ++k)
    ADAMVS_CHECK_ARG(std::isfinite(gain[k]) && gain[k] > 0.f, "ortho_adjust_image: gain[%d]=%g (finite, > 0)", k, (double)gain[k]);
  return launch_ortho_adjust_image(rgba_in, (long)H * W, gain, rgba_out, (hipStream_t)stream);
}

extern "C" int adamvs_ortho_seam_stats(const adamvs_ortho_grid* grid, const int* view_out, const unsigned char* rgba, long long* stats,
                                       void* stream) {
  if (int rc = ortho_check_grid(grid, "ortho_seam_stats")) return rc;
  ADAMVS_CHECK_ARG(view_out && rgba && stats, "ortho_seam_stats: null pointer");
  return launch_ortho_seam_stats(*grid, view_out, rgba, stats, (hipStream_t)stream);
}

// ---- mesh texturing (texture.hip): every argument is checked here, before any launch
static int texture_check_mesh(long nv, long nf, const char* what) {
  ADAMVS_CHECK_ARG(nv >= 1, "%s: nv=%ld (>= 1)", what, nv);
  ADAMVS_CHECK_ARG(nf >= 0 && nf <= ADAMVS_TEXTURE_MAX_FACES, "%s: nf=%ld (0 .. %ld)", what, nf, (long)ADAMVS_TEXTURE_MAX_FACES);
  return 0;
}

static int texture_check_page(int P, long npages, const char* what) {
  ADAMVS_CHECK_ARG(P >= ADAMVS_TEXTURE_MIN_PAGE && P <= ADAMVS_TEXTURE_MAX_PAGE && (P & (P - 1)) == 0, "%s: page %d (a power of two %d .. %d)",
                   what, P, ADAMVS_TEXTURE_MIN_PAGE, ADAMVS_TEXTURE_MAX_PAGE);
  ADAMVS_CHECK_ARG(npages >= 1, "%s: npages=%ld (>= 1)", what, npages);
  return 0;
}

extern "C" int adamvs_texture_project(const adamvs_ortho_view* view, const double* xyz, long nv, float* uvz, void* stream) {
  if (int rc = ortho_check_view(view, "texture_project")) return rc;
  if (int rc = texture_check_mesh(nv, 0, "texture_project")) return rc;
  ADAMVS_CHECK_ARG(xyz && uvz, "texture_project: null pointer");
  return launch_tex_project(*view, xyz, nv, uvz, (hipStream_t)stream);
}

extern "C" int adamvs_texture_zbuf(const adamvs_ortho_view* view, const float* uvz, long nv, const unsigned* faces, long nf, unsigned* zbuf,
                                   unsigned* big_count, unsigned* big_list, long big_capacity, void* stream) {
  if (int rc = ortho_check_view(view, "texture_zbuf")) return rc;
  if (int rc = texture_check_mesh(nv, nf, "texture_zbuf")) return rc;
  ADAMVS_CHECK_ARG(uvz && faces && zbuf && big_count && big_list, "texture_zbuf: null pointer");
  ADAMVS_CHECK_ARG(big_capacity >= nf, "texture_zbuf: big_capacity %ld < nf = %ld", big_capacity, nf);
  return launch_tex_zbuf(view->W, view->H, uvz, nv, faces, nf, zbuf, big_count, big_list, (hipStream_t)stream);
}

extern "C" int adamvs_texture_score(const adamvs_ortho_view* view, int view_index, const float* uvz, long nv, const unsigned* faces, long nf,
                                    const unsigned* zbuf, float border, float tol, float* best, int* label, int* nvis, float* uv,
                                    void* stream) {
  if (int rc = ortho_check_view(view, "texture_score")) return rc;
  if (int rc = texture_check_mesh(nv, nf, "texture_score")) return rc;
  ADAMVS_CHECK_ARG(uvz && faces && zbuf && best && label && nvis && uv, "texture_score: null pointer");
  ADAMVS_CHECK_ARG(view_index >= 0, "texture_score: view_index=%d (>= 0)", view_index);
  ADAMVS_CHECK_ARG(std::isfinite(border) && border >= 0.f, "texture_score: border=%g (finite, >= 0)", (double)border);
  ADAMVS_CHECK_ARG(std::isfinite(tol) && tol >= 0.f, "texture_score: tol=%g (finite, >= 0)", (double)tol);
  return launch_tex_score(view->W, view->H, view_index, uvz, nv, faces, nf, zbuf, border, tol, best, label, nvis, uv, (hipStream_t)stream);
}

extern "C" int adamvs_texture_edge_keys(const unsigned* faces, long nf, long long* keys, void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_edge_keys")) return rc;
  ADAMVS_CHECK_ARG(faces && keys, "texture_edge_keys: null pointer");
  return launch_mesh_edge_keys(faces, nf, keys, "texture_edge_keys", (hipStream_t)stream);
}

extern "C" int adamvs_texture_components(const long long* keys_sorted, const long long* entry, long nf, const int* label, int* parent,
                                         unsigned* changed, void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_components")) return rc;
  ADAMVS_CHECK_ARG(keys_sorted && entry && label && parent && changed, "texture_components: null pointer");
  return launch_tex_components_round(keys_sorted, entry, 3 * nf, label, parent, nf, changed, (hipStream_t)stream);
}

extern "C" int adamvs_texture_rank(const int* label, const int* parent, long nf, unsigned* block_roots, unsigned* block_untex,
                                   unsigned* root_off, unsigned* untex_off, int* root_chart, int* pal, void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_rank")) return rc;
  ADAMVS_CHECK_ARG(label && parent && block_roots && block_untex && root_off && untex_off && root_chart && pal, "texture_rank: null pointer");
  return launch_tex_rank(label, parent, nf, block_roots, block_untex, root_off, untex_off, root_chart, pal, (hipStream_t)stream);
}

extern "C" int adamvs_texture_boxes(const int* label, const int* parent, const int* root_chart, const float* uv, long nf, int* chart, int* box,
                                    void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_boxes")) return rc;
  ADAMVS_CHECK_ARG(label && parent && root_chart && uv && chart && box, "texture_boxes: null pointer");
  return launch_tex_boxes(label, parent, root_chart, uv, nf, chart, box, (hipStream_t)stream);
}

extern "C" int adamvs_texture_fill(const adamvs_ortho_view* view, const int* items, const long long* prefix, int n, long texels, int P,
                                   long npages, unsigned char* atlas, void* stream) {
  if (int rc = ortho_check_view(view, "texture_fill")) return rc;
  if (int rc = texture_check_page(P, npages, "texture_fill")) return rc;
  ADAMVS_CHECK_ARG(n >= 0 && texels >= 0, "texture_fill: n=%d, texels=%ld (>= 0)", n, texels);
  ADAMVS_CHECK_ARG((items && prefix && atlas) || n == 0, "texture_fill: null pointer");
  return launch_tex_fill(*view, items, prefix, n, texels, P, npages, atlas, (hipStream_t)stream);
}

extern "C" int adamvs_texture_coords(const int* label, const int* chart, const int* pal, const float* uv, long nf, const int* charts,
                                     int pal_ox, int pal_oy, int pal_page, int P, long npages, const unsigned* faces, long nv,
                                     const unsigned char* vrgb, unsigned char* atlas, float* tc, int* texnum, void* stream) {
  if (int rc = texture_check_mesh(nv, nf, "texture_coords")) return rc;
  if (int rc = texture_check_page(P, npages, "texture_coords")) return rc;
  ADAMVS_CHECK_ARG(label && chart && pal && uv && faces && vrgb && atlas && tc && texnum, "texture_coords: null pointer");
  ADAMVS_CHECK_ARG(pal_ox >= 0 && pal_oy >= 0 && pal_page >= 0, "texture_coords: palette at (%d, %d) of page %d", pal_ox, pal_oy, pal_page);
  return launch_tex_coords(label, chart, pal, uv, nf, charts, pal_ox, pal_oy, pal_page, P, npages, faces, nv, vrgb, atlas, tc, texnum,
                           (hipStream_t)stream);
}

// ---- seam levelling (texture_level.hip)
static int level_check_graph(const int* rowptr, const unsigned* col, long nnz, long n, const char* what) {
  ADAMVS_CHECK_ARG(n >= 0 && n <= ADAMVS_TEXTURE_LEVEL_MAX_NODES, "%s: n=%ld (0 .. %ld)", what, n, (long)ADAMVS_TEXTURE_LEVEL_MAX_NODES);
  ADAMVS_CHECK_ARG(nnz >= 0 && nnz <= 2147483647L, "%s: nnz=%ld (0 .. 2^31 - 1)", what, nnz);
  ADAMVS_CHECK_ARG(rowptr && (col || nnz == 0), "%s: null pointer", what);
  return 0;
}

extern "C" int adamvs_texture_level_observe(const long long* view_tab, int nviews, const int* rowptr, const unsigned* col, long nnz,
                                            const int* node_view, const float* pos, long n, float* f, void* stream) {
  if (int rc = level_check_graph(rowptr, col, nnz, n, "texture_level_observe")) return rc;
  ADAMVS_CHECK_ARG(nviews >= 1, "texture_level_observe: nviews=%d (>= 1)", nviews);
  ADAMVS_CHECK_ARG(view_tab && node_view && pos && f, "texture_level_observe: null pointer");
  return launch_lvl_observe(view_tab, nviews, rowptr, col, nnz, node_view, pos, n, f, (hipStream_t)stream);
}

extern "C" int adamvs_texture_level_rhs(const int* rowptr, const unsigned* col, long nnz, const float* f, long n, double* b, void* stream) {
  if (int rc = level_check_graph(rowptr, col, nnz, n, "texture_level_rhs")) return rc;
  ADAMVS_CHECK_ARG(f && b, "texture_level_rhs: null pointer");
  return launch_lvl_rhs(rowptr, col, nnz, f, n, b, (hipStream_t)stream);
}

extern "C" int adamvs_texture_level_cg_init(const double* b, long n, double tol, double* g, double* r, double* p, double* partials,
                                            double* state, void* stream) {
  ADAMVS_CHECK_ARG(n >= 0 && n <= ADAMVS_TEXTURE_LEVEL_MAX_NODES, "texture_level_cg_init: n=%ld (0 .. %ld)", n,
                   (long)ADAMVS_TEXTURE_LEVEL_MAX_NODES);
  ADAMVS_CHECK_ARG(std::isfinite(tol) && tol >= 0.0, "texture_level_cg_init: tol=%g (finite, >= 0)", tol);
  ADAMVS_CHECK_ARG(b && g && r && p && partials && state, "texture_level_cg_init: null pointer");
  return launch_lvl_cg_init(b, n, tol, g, r, p, partials, state, (hipStream_t)stream);
}

extern "C" int adamvs_texture_level_cg(const int* rowptr, const unsigned* col, long nnz, long n, double lambda, int iters, double* g,
                                       double* r, double* p, double* ap, double* partials, double* state, void* stream) {
  if (int rc = level_check_graph(rowptr, col, nnz, n, "texture_level_cg")) return rc;
  ADAMVS_CHECK_ARG(std::isfinite(lambda) && lambda > 0.0, "texture_level_cg: lambda=%g (finite, > 0)", lambda);
  ADAMVS_CHECK_ARG(iters >= 0, "texture_level_cg: iters=%d (>= 0)", iters);
  ADAMVS_CHECK_ARG(g && r && p && ap && partials && state, "texture_level_cg: null pointer");
  ADAMVS_CHECK_ARG(((uintptr_t)g | (uintptr_t)r | (uintptr_t)p | (uintptr_t)ap) % 16 == 0, "texture_level_cg: g, r, p, ap must be 16-byte aligned");
  return launch_lvl_cg(rowptr, col, nnz, n, lambda, iters, g, r, p, ap, partials, state, (hipStream_t)stream);
}

static int level_check_charts(const int* charts, const long long* prefix, int nc, long texels, const char* what) {
  ADAMVS_CHECK_ARG(nc >= 0 && texels >= 0, "%s: nc=%d, texels=%ld (>= 0)", what, nc, texels);
  ADAMVS_CHECK_ARG(prefix && (charts || nc == 0), "%s: null pointer", what);
  return 0;
}

extern "C" int adamvs_texture_level_owner(const float* uv, const int* chart, long nf, const int* charts, const long long* prefix, int nc,
                                          long texels, int* owner, unsigned* big_count, unsigned* big_list, long big_capacity,
                                          void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_level_owner")) return rc;
  if (int rc = level_check_charts(charts, prefix, nc, texels, "texture_level_owner")) return rc;
  ADAMVS_CHECK_ARG(uv && chart && big_count && big_list && (owner || texels == 0), "texture_level_owner: null pointer");
  ADAMVS_CHECK_ARG(big_capacity >= nf, "texture_level_owner: big_capacity %ld < nf = %ld", big_capacity, nf);
  return launch_lvl_owner(uv, chart, nf, charts, prefix, nc, texels, owner, big_count, big_list, (hipStream_t)stream);
}

extern "C" int adamvs_texture_level_dilate(const int* charts, const long long* prefix, int nc, long texels, const int* owner_in,
                                           int* owner_out, void* stream) {
  if (int rc = level_check_charts(charts, prefix, nc, texels, "texture_level_dilate")) return rc;
  ADAMVS_CHECK_ARG((owner_in && owner_out) || texels == 0, "texture_level_dilate: null pointer");
  ADAMVS_CHECK_ARG(owner_in != owner_out || texels == 0, "texture_level_dilate: the round is double-buffered (owner_in == owner_out)");
  return launch_lvl_dilate(charts, prefix, nc, texels, owner_in, owner_out, (hipStream_t)stream);
}

extern "C" int adamvs_texture_level_apply(const float* uv, const int* corner_node, long nf, const double* g, long n, const int* charts,
                                          const long long* prefix, int nc, long texels, const int* owner, int P, long npages,
                                          unsigned char* atlas, void* stream) {
  if (int rc = texture_check_mesh(1, nf, "texture_level_apply")) return rc;
  if (int rc = texture_check_page(P, npages, "texture_level_apply")) return rc;
  if (int rc = level_check_charts(charts, prefix, nc, texels, "texture_level_apply")) return rc;
  ADAMVS_CHECK_ARG(n >= 0 && n <= ADAMVS_TEXTURE_LEVEL_MAX_NODES, "texture_level_apply: n=%ld (0 .. %ld)", n,
                   (long)ADAMVS_TEXTURE_LEVEL_MAX_NODES);
  ADAMVS_CHECK_ARG(uv && corner_node && atlas && (g || n == 0) && (owner || texels == 0), "texture_level_apply: null pointer");
  return launch_lvl_apply(uv, corner_node, nf, g, n, charts, prefix, nc, texels, owner, P, npages, atlas, (hipStream_t)stream);
}
