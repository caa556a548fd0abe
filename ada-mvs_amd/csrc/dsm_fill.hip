// Bounded harmonic gap fill of a finalised DSM and its orthophoto (the step after k_dsm_finalize).
// include/adamvs_hip.h "DSM gap fill" states the result; this file computes it in two parts:
//
//   distance   k_fill_cols   one lane per cell: rows to the nearest valid cell of its column, searched out to R = ceil(r)
//                            (clamped to R + 1: "none within R")
//              k_fill_rows   one workgroup per 256-cell row segment, the segment and R columns either side of g in LDS:
//                            dist2 = min over |dx| <= R of dx^2 + g(j + dx)^2, stopping once dx^2 reaches the best so far;
//                            also the class byte, `filled`, the initial fine state and the integer cell counts
//   solve      geometric multigrid V-cycles on the masked grid, height (fp64) and R, G, B (fp32) in the same passes:
//              k_fill_residual  fine level: the stopping residual (exact max through an integer atomicMax on the bits of the
//                               non-negative value) and the residual scaled for the restriction
//              k_fill_restrict  transpose of the prolongation, gathered over the 4 x 4 children of a coarse cell
//              k_fill_smooth    one colour of a red-black Gauss-Seidel sweep (k_fill_zero_red: the first one from e = 0)
//              k_fill_prolong   masked bilinear prolongation, added to the unknown cells
//              k_fill_coarsest  one 64-lane workgroup iterates the coarsest level (<= 8 x 8 cells) in LDS
//              k_fill_output    the rasters
//
// Every reduction is an integer max or sum and every update reads only values of the other colour: the output is
// bit-identical from run to run.
#include "common.h"
#include "kernels.h"

namespace adamvs {

// Class of a cell on a level: excluded (stays empty; on a coarse level: neither kind of child), Dirichlet (V; on a coarse
// level: any Dirichlet child, e = 0) or unknown (F; on a coarse level: an unknown child and no Dirichlet child).  A coarse
// cell with children tied to V stays out of the coarse problem: the unscaled 5-point operator would take such a cell for
// a weakly held one (a lone F cell between V cells is pure diagonal on the fine level) and the correction would overshoot;
// the smoother settles those cells within a sweep or two.  Every coarse unknown component still touches a Dirichlet cell:
// a fine path from F to V leaves the component through a coarse cell with a child in V (one without would be unknown and
// in the component), so every coarse system is positive definite.
enum : uint8_t { FC_EXCL = 0, FC_DIR = 1, FC_UNK = 2 };

constexpr int FILL_TILE = 256;
constexpr int FILL_COARSE_SWEEPS = 300;   // red-black sweeps of the coarsest level per V-cycle
constexpr int FILL_MAX_LEVELS = 32;       // a side of 2^28 cells halves to <= 8 in 26 steps

struct FillLevel {
  int W, H;
  uint8_t* cls;
  double* uh;          // fine: the heights; coarse: the correction
  float4* uc;          // R, G, B (w unused)
  const double* fh;    // coarse: right-hand side (restricted residual); null on the fine level (f = 0)
  const float4* fc;
};

__device__ __forceinline__ bool fill_valid(float h) { return __builtin_isfinite(h); }

// ---- exact squared distance to V, bounded by R -------------------------------------------------------------------------
__global__ __launch_bounds__(FILL_TILE) void k_fill_cols(int W, int H, int R, const float* __restrict__ dsm, int* __restrict__ g) {
  const int j = blockIdx.x * FILL_TILE + threadIdx.x;
  if (j >= W) return;
  for (int i = blockIdx.y; i < H; i += gridDim.y) {
    int d = 0;
    if (!fill_valid(dsm[(long)i * W + j])) {
      d = R + 1;
      for (int k = 1; k <= R; ++k) {
        if ((i - k >= 0 && fill_valid(dsm[(long)(i - k) * W + j])) || (i + k < H && fill_valid(dsm[(long)(i + k) * W + j]))) {
          d = k;
          break;
        }
      }
    }
    g[(long)i * W + j] = d;
  }
}

__global__ __launch_bounds__(FILL_TILE) void k_fill_rows(int W, int H, int R, double r2, const int* __restrict__ g,
                                                         const float* __restrict__ dsm, const unsigned* __restrict__ rgba,
                                                         int* __restrict__ dist2, uint8_t* __restrict__ filled, uint8_t* __restrict__ cls,
                                                         double* __restrict__ uh, float4* __restrict__ uc,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ int s_g[FILL_TILE + 2 * ADAMVS_DSM_FILL_MAX_RADIUS];
  const int j0 = blockIdx.x * FILL_TILE;
  for (int i = blockIdx.y; i < H; i += gridDim.y) {       // block-uniform: the barriers below are reached by every lane
  const long row = (long)i * W;
  for (int k = threadIdx.x; k < FILL_TILE + 2 * R; k += FILL_TILE) {
    const int j = j0 - R + k;
    s_g[k] = (j >= 0 && j < W) ? g[row + j] : R + 1;
  }
  __syncthreads();
  const int j = j0 + threadIdx.x;
  bool v = false, f = false;
  if (j < W) {
    const int* c = s_g + R + threadIdx.x;
    int best = c[0] * c[0];
    for (int dx = 1; dx <= R && dx * dx < best; ++dx) {
      const int m = min(c[-dx], c[dx]);
      best = min(best, dx * dx + m * m);
    }
    v = best == 0;
    f = !v && (double)best <= r2;
    const long p = row + j;
    dist2[p] = (v || f) ? best : 0x7fffffff;
    filled[p] = f;
    cls[p] = v ? FC_DIR : f ? FC_UNK : FC_EXCL;
    const unsigned c4 = rgba[p];
    uh[p] = v ? (double)dsm[p] : 0.0;
    uc[p] = v ? make_float4((float)(c4 & 255u), (float)((c4 >> 8) & 255u), (float)((c4 >> 16) & 255u), 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int nv = __syncthreads_count(v), nf = __syncthreads_count(f);
  if (threadIdx.x == 0) {
    if (nv) atomicAdd(counts + 0, (unsigned long long)nv);
    if (nf) atomicAdd(counts + 1, (unsigned long long)nf);
  }
  }
}

// ---- multigrid ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FILL_TILE) void k_fill_coarsen(int Wf, int Hf, const uint8_t* __restrict__ cf, int Wc, int Hc, uint8_t* __restrict__ cc) {
  const int I = blockIdx.x * FILL_TILE + threadIdx.x;
  if (I >= Wc) return;
  for (int J = blockIdx.y; J < Hc; J += gridDim.y) {
  bool unk = false, dir = false;
  for (int b = 0; b < 2; ++b)
    for (int a = 0; a < 2; ++a) {
      const int x = 2 * I + a, y = 2 * J + b;
      if (x < Wf && y < Hf) {
        const uint8_t k = cf[(long)y * Wf + x];
        unk |= k == FC_UNK;
        dir |= k == FC_DIR;
      }
    }
  cc[(long)J * Wc + I] = dir ? FC_DIR : unk ? FC_UNK : FC_EXCL;
  }
}

// Sum over the non-excluded 4-neighbours of the cell; deg = their number.
struct FillSum {
  double h;
  float3 c;
  int deg;
};

__device__ __forceinline__ FillSum fill_neighbours(const FillLevel& L, int x, int y) {
  FillSum s{0.0, make_float3(0.f, 0.f, 0.f), 0};
  const long p = (long)y * L.W + x;
  const int dx[4] = {-1, 1, 0, 0}, dy[4] = {0, 0, -1, 1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xn = x + dx[k], yn = y + dy[k];
    if (xn < 0 || xn >= L.W || yn < 0 || yn >= L.H) continue;
    const long q = p + dy[k] * (long)L.W + dx[k];
    if (L.cls[q] == FC_EXCL) continue;
    const float4 c = L.uc[q];
    s.h += L.uh[q];
    s.c.x += c.x;
    s.c.y += c.y;
    s.c.z += c.z;
    ++s.deg;
  }
  return s;
}

// One colour of a red-black Gauss-Seidel sweep: e_c = (f_c + sum of the neighbours) / deg.
template <bool FINE>
__global__ __launch_bounds__(FILL_TILE) void k_fill_smooth(const FillLevel L, int parity) {
  for (int y = blockIdx.y; y < L.H; y += gridDim.y) {
  const int x = 2 * (blockIdx.x * FILL_TILE + threadIdx.x) + ((y + parity) & 1);
  if (x >= L.W) continue;
  const long p = (long)y * L.W + x;
  const uint8_t k = L.cls[p];
  if (k != FC_UNK) continue;
  const FillSum s = fill_neighbours(L, x, y);
  if (FINE) {
    const float inv = 1.f / (float)s.deg;
    L.uh[p] = s.h / (double)s.deg;
    L.uc[p] = make_float4(s.c.x * inv, s.c.y * inv, s.c.z * inv, 0.f);
  } else {
    const double d = (double)s.deg;
    const float df = (float)d;
    const float4 f = L.fc[p];
    L.uh[p] = (L.fh[p] + s.h) / d;
    L.uc[p] = make_float4((f.x + s.c.x) / df, (f.y + s.c.y) / df, (f.z + s.c.z) / df, 0.f);
  }
  }
}

// The red colour of the first sweep of a coarse level from e = 0; writes every cell (0 where not unknown or black).
__global__ __launch_bounds__(FILL_TILE) void k_fill_zero_red(const FillLevel L) {
  const int x = blockIdx.x * FILL_TILE + threadIdx.x;
  if (x >= L.W) return;
  for (int y = blockIdx.y; y < L.H; y += gridDim.y) {
  const long p = (long)y * L.W + x;
  const uint8_t k = L.cls[p];
  double eh = 0.0;
  float4 ec = make_float4(0.f, 0.f, 0.f, 0.f);
  if (k == FC_UNK && ((x + y) & 1) == 0) {
    int deg = 0;
    if (x > 0) deg += L.cls[p - 1] != FC_EXCL;
    if (x + 1 < L.W) deg += L.cls[p + 1] != FC_EXCL;
    if (y > 0) deg += L.cls[p - L.W] != FC_EXCL;
    if (y + 1 < L.H) deg += L.cls[p + L.W] != FC_EXCL;
    const float4 f = L.fc[p];
    const float df = (float)deg;
    eh = L.fh[p] / (double)deg;
    ec = make_float4(f.x / df, f.y / df, f.z / df, 0.f);
  }
  L.uh[p] = eh;
  L.uc[p] = ec;
  }
}

// Cell-centred bilinear weights from the 2 x 2 coarse cells around fine cell (x, y): its parent (9/16), the two side
// neighbours towards it (3/16) and the diagonal one (1/16).  Coarse cells outside the grid or excluded are left out and
// the rest renormalised (wsum); the prolongation is  e_f = sum w e_c / wsum_f  and the restriction is its transpose,
// f_c = sum over the fine cells of w rs_f  with  rs_f = res_f / wsum_f.
__device__ __forceinline__ void fill_parents(int x, int y, int Wc, int Hc, int X[2], int Y[2], double wx[2], double wy[2]) {
  X[0] = x >> 1;
  X[1] = (x & 1) ? X[0] + 1 : X[0] - 1;
  Y[0] = y >> 1;
  Y[1] = (y & 1) ? Y[0] + 1 : Y[0] - 1;
  wx[0] = 0.75;
  wx[1] = (X[1] >= 0 && X[1] < Wc) ? 0.25 : 0.0;
  wy[0] = 0.75;
  wy[1] = (Y[1] >= 0 && Y[1] < Hc) ? 0.25 : 0.0;
}

__device__ __forceinline__ unsigned long long fill_max_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// Residual of the unknown cells, scaled for the restriction.  On the fine level (FINE) also the exact maxima of |res| of the
// height and over the three colours: a wave reduction, then one integer atomicMax per workgroup on the bits.
template <bool FINE>
__global__ __launch_bounds__(FILL_TILE) void k_fill_residual(const FillLevel L, const uint8_t* __restrict__ cls_c, int Wc, int Hc,
                                                             double* __restrict__ rs_h, float4* __restrict__ rs_c,
                                                             unsigned long long* __restrict__ max_h, unsigned* __restrict__ max_c) {
  const int x = blockIdx.x * FILL_TILE + threadIdx.x;
  double ah = 0.0;
  float ac = 0.f;
  for (int y = blockIdx.y; y < L.H && x < L.W; y += gridDim.y) {
    const long p = (long)y * L.W + x;
    const uint8_t k = L.cls[p];
    double rh = 0.0;
    float4 rc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (k == FC_UNK) {
      const FillSum s = fill_neighbours(L, x, y);
      const double d = (double)s.deg;
      const float df = (float)d;
      const float4 u = L.uc[p];
      rh = s.h - d * L.uh[p];
      rc = make_float4(s.c.x - df * u.x, s.c.y - df * u.y, s.c.z - df * u.z, 0.f);
      if (!FINE) {
        const float4 f = L.fc[p];
        rh += L.fh[p];
        rc.x += f.x;
        rc.y += f.y;
        rc.z += f.z;
      }
      if (FINE) {                               // NaN (a diverged solve) counts as +inf, not as 0
        const float m = fmaxf(fmaxf(fabsf(rc.x), fabsf(rc.y)), fabsf(rc.z));
        ah = fmax(ah, rh == rh ? fabs(rh) : (double)INFINITY);
        ac = fmaxf(ac, (rc.x == rc.x && rc.y == rc.y && rc.z == rc.z) ? m : INFINITY);
      }
      int X[2], Y[2];
      double wx[2], wy[2];
      fill_parents(x, y, Wc, Hc, X, Y, wx, wy);
      double ws = 0.0;
      for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a)
          if (wx[a] * wy[b] > 0.0 && cls_c[(long)Y[b] * Wc + X[a]] != FC_EXCL) ws += wx[a] * wy[b];
      const double inv = 1.0 / ws;
      const float invf = (float)inv;
      rh *= inv;
      rc = make_float4(rc.x * invf, rc.y * invf, rc.z * invf, 0.f);
    }
    rs_h[p] = rh;
    rs_c[p] = rc;
  }
  if (FINE) {
    for (int off = 32; off; off >>= 1) {
      ah = fmax(ah, __shfl_xor(ah, off));
      ac = fmaxf(ac, __shfl_xor(ac, off));
    }
    __shared__ double s_h[FILL_TILE / 64];
    __shared__ float s_c[FILL_TILE / 64];
    if ((threadIdx.x & 63) == 0) {
      s_h[threadIdx.x >> 6] = ah;
      s_c[threadIdx.x >> 6] = ac;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < FILL_TILE / 64; ++w) {
        ah = fmax(ah, s_h[w]);
        ac = fmaxf(ac, s_c[w]);
      }
      if (ah > 0.0) atomicMax(max_h, fill_max_bits(ah));
      if (ac > 0.f) atomicMax(max_c, __float_as_uint(ac));
    }
  }
}

__global__ __launch_bounds__(FILL_TILE) void k_fill_restrict(int Wf, int Hf, const double* __restrict__ rs_h, const float4* __restrict__ rs_c,
                                                             int Wc, int Hc, const uint8_t* __restrict__ cls_c, double* __restrict__ fh,
                                                             float4* __restrict__ fc) {
  const int X = blockIdx.x * FILL_TILE + threadIdx.x;
  if (X >= Wc) return;
  for (int Y = blockIdx.y; Y < Hc; Y += gridDim.y) {
  const long q = (long)Y * Wc + X;
  double sh = 0.0;
  float4 sc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cls_c[q] >= FC_UNK) {
    const double w[4] = {0.25, 0.75, 0.75, 0.25};
    for (int b = 0; b < 4; ++b) {
      const int y = 2 * Y - 1 + b;
      if (y < 0 || y >= Hf) continue;
      for (int a = 0; a < 4; ++a) {
        const int x = 2 * X - 1 + a;
        if (x < 0 || x >= Wf) continue;
        const long p = (long)y * Wf + x;
        const double ww = w[a] * w[b];
        const float wf = (float)ww;
        const float4 r = rs_c[p];
        sh += ww * rs_h[p];
        sc.x += wf * r.x;
        sc.y += wf * r.y;
        sc.z += wf * r.z;
      }
    }
  }
  fh[q] = sh;
  fc[q] = sc;
  }
}

__global__ __launch_bounds__(FILL_TILE) void k_fill_prolong(const FillLevel F, const FillLevel C) {
  const int x = blockIdx.x * FILL_TILE + threadIdx.x;
  if (x >= F.W) return;
  for (int y = blockIdx.y; y < F.H; y += gridDim.y) {
  const long p = (long)y * F.W + x;
  if (F.cls[p] != FC_UNK) continue;
  int X[2], Y[2];
  double wx[2], wy[2];
  fill_parents(x, y, C.W, C.H, X, Y, wx, wy);
  double ws = 0.0, eh = 0.0;
  float3 ec = make_float3(0.f, 0.f, 0.f);
  for (int b = 0; b < 2; ++b)
    for (int a = 0; a < 2; ++a) {
      const double w = wx[a] * wy[b];
      if (w == 0.0) continue;
      const long q = (long)Y[b] * C.W + X[a];
      if (C.cls[q] == FC_EXCL) continue;
      const float wf = (float)w;
      const float4 c = C.uc[q];
      ws += w;
      eh += w * C.uh[q];
      ec.x += wf * c.x;
      ec.y += wf * c.y;
      ec.z += wf * c.z;
    }
  const double inv = 1.0 / ws;
  const float invf = (float)inv;
  float4 u = F.uc[p];
  F.uh[p] += eh * inv;
  u.x += ec.x * invf;
  u.y += ec.y * invf;
  u.z += ec.z * invf;
  F.uc[p] = u;
  }
}

// The coarsest level (<= 64 cells), one lane per cell, FILL_COARSE_SWEEPS red-black sweeps from e = 0 in LDS.
__global__ __launch_bounds__(64) void k_fill_coarsest(const FillLevel L) {
  __shared__ double s_h[64];
  __shared__ float4 s_c[64];
  __shared__ uint8_t s_k[64];
  const int t = threadIdx.x, n = L.W * L.H;
  const int x = t % L.W, y = t / L.W;
  uint8_t k = FC_EXCL;
  double fh = 0.0;
  float4 fc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (t < n) {
    k = L.cls[t];
    if (k == FC_UNK) {
      fh = L.fh[t];
      fc = L.fc[t];
    }
  }
  s_k[t] = k;
  s_h[t] = 0.0;
  s_c[t] = make_float4(0.f, 0.f, 0.f, 0.f);
  __syncthreads();
  int nb[4], deg = 0;
  if (t < n && k == FC_UNK) {
    const int cand[4] = {x > 0 ? t - 1 : -1, x + 1 < L.W ? t + 1 : -1, y > 0 ? t - L.W : -1, y + 1 < L.H ? t + L.W : -1};
    for (int m = 0; m < 4; ++m)
      if (cand[m] >= 0 && s_k[cand[m]] != FC_EXCL) nb[deg++] = cand[m];
  }
  const double d = (double)deg;
  const float df = (float)d;
  for (int it = 0; it < 2 * FILL_COARSE_SWEEPS; ++it) {
    if (t < n && k == FC_UNK && ((x + y) & 1) == (it & 1)) {
      double sh = fh;
      float4 sc = fc;
      for (int m = 0; m < deg; ++m) {
        const float4 c = s_c[nb[m]];
        sh += s_h[nb[m]];
        sc.x += c.x;
        sc.y += c.y;
        sc.z += c.z;
      }
      s_h[t] = sh / d;
      s_c[t] = make_float4(sc.x / df, sc.y / df, sc.z / df, 0.f);
    }
    __syncthreads();
  }
  if (t < n) {
    L.uh[t] = s_h[t];
    L.uc[t] = s_c[t];
  }
}

__global__ __launch_bounds__(FILL_TILE) void k_fill_output(long n, const float* __restrict__ dsm, const unsigned* __restrict__ rgba,
                                                           const uint8_t* __restrict__ cls, const double* __restrict__ uh,
                                                           const float4* __restrict__ uc, float* __restrict__ dsm_out,
                                                           unsigned* __restrict__ rgba_out) {
  const long p = (long)blockIdx.x * FILL_TILE + threadIdx.x;
  if (p >= n) return;
  const uint8_t k = cls[p];
  if (k == FC_DIR) {
    dsm_out[p] = dsm[p];
    rgba_out[p] = rgba[p];
  } else if (k == FC_UNK) {
    const float4 c = uc[p];
    const auto q = [](float v) { return (unsigned)fminf(fmaxf(rintf(v), 0.f), 255.f); };
    dsm_out[p] = (float)uh[p];
    rgba_out[p] = q(c.x) | (q(c.y) << 8) | (q(c.z) << 16) | 0xff000000u;
  } else {
    dsm_out[p] = __uint_as_float(0x7fc00000u);
    rgba_out[p] = 0u;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// Levels: 0 is the grid; level l + 1 halves level l (rounding up) until both sides are <= 8 (at least one coarse level).
static int fill_levels(int W, int H, int* Ws, int* Hs) {
  int n = 0;
  Ws[0] = W;
  Hs[0] = H;
  while (n == 0 || Ws[n] > 8 || Hs[n] > 8) {
    Ws[n + 1] = (Ws[n] + 1) / 2;
    Hs[n + 1] = (Hs[n] + 1) / 2;
    ++n;
  }
  return n + 1;
}


// Workspace: counters (256 B), then per level its class bytes; the fine level's u (fp64) and colours (float4); the residual
// scratch of the fine size (fp64 + float4; the column distances of the distance pass live in it first); per coarse level
// e and f (fp64 + float4 each).
struct FillWs {
  unsigned long long* counts;     // [0] cells valid, [1] cells fillable, [2] max |res| height bits, [3] max |res| colour bits
  int nl;
  FillLevel lv[FILL_MAX_LEVELS];
  double* rs_h;
  float4* rs_c;
};

static long fill_layout(int W, int H, char* base, FillWs* ws) {
  int Ws[FILL_MAX_LEVELS], Hs[FILL_MAX_LEVELS];
  const int nl = fill_levels(W, H, Ws, Hs);
  long off = 0;
  auto take = [&](long bytes) -> char* { char* p = base ? base + off : nullptr; off += align256(bytes); return p; };
  char* counts = take(256);
  if (ws) {
    ws->counts = (unsigned long long*)counts;
    ws->nl = nl;
  }
  const long n0 = (long)W * H;
  char* rs_h = take(8 * n0);
  char* rs_c = take(16 * n0);
  if (ws) {
    ws->rs_h = (double*)rs_h;
    ws->rs_c = (float4*)rs_c;
  }
  for (int l = 0; l < nl; ++l) {
    const long n = (long)Ws[l] * Hs[l];
    FillLevel L{Ws[l], Hs[l], (uint8_t*)take(n), (double*)take(8 * n), (float4*)take(16 * n), nullptr, nullptr};
    if (l > 0) {
      L.fh = (const double*)take(8 * n);
      L.fc = (const float4*)take(16 * n);
    }
    if (ws) ws->lv[l] = L;
  }
  return off;
}

long dsm_fill_workspace_bytes(int W, int H) { return fill_layout(W, H, nullptr, nullptr); }

// x: 256-cell segments of a row; y: rows, strided by the kernels past 65535
static dim3 fill_rows_grid(int W, int H) { return dim3((unsigned)cdiv(W, FILL_TILE), (unsigned)min(H, 65535)); }

// One V-cycle correction below level l (whose residual is already scaled into rs), added to level l's unknowns.
static int fill_coarse_correction(FillWs& w, int l, hipStream_t st) {
  const FillLevel& F = w.lv[l];
  const FillLevel& C = w.lv[l + 1];
  hipLaunchKernelGGL(k_fill_restrict, fill_rows_grid(C.W, C.H), dim3(FILL_TILE), 0, st, F.W, F.H, (const double*)w.rs_h,
                     (const float4*)w.rs_c, C.W, C.H, (const uint8_t*)C.cls, const_cast<double*>(C.fh), const_cast<float4*>(C.fc));
  if (l + 2 == w.nl) {
    hipLaunchKernelGGL(k_fill_coarsest, dim3(1), dim3(64), 0, st, C);
  } else {
    const dim3 half = fill_rows_grid((C.W + 1) / 2, C.H);
    hipLaunchKernelGGL(k_fill_zero_red, fill_rows_grid(C.W, C.H), dim3(FILL_TILE), 0, st, C);
    hipLaunchKernelGGL(k_fill_smooth<false>, half, dim3(FILL_TILE), 0, st, C, 1);
    const FillLevel& D = w.lv[l + 2];
    hipLaunchKernelGGL(k_fill_residual<false>, fill_rows_grid(C.W, C.H), dim3(FILL_TILE), 0, st, C, (const uint8_t*)D.cls, D.W, D.H,
                       w.rs_h, w.rs_c, (unsigned long long*)nullptr, (unsigned*)nullptr);
    if (int rc = fill_coarse_correction(w, l + 1, st)) return rc;
    hipLaunchKernelGGL(k_fill_smooth<false>, half, dim3(FILL_TILE), 0, st, C, 0);
    hipLaunchKernelGGL(k_fill_smooth<false>, half, dim3(FILL_TILE), 0, st, C, 1);
  }
  hipLaunchKernelGGL(k_fill_prolong, fill_rows_grid(F.W, F.H), dim3(FILL_TILE), 0, st, F, C);
  ADAMVS_CHECK_LAUNCH("dsm_fill: V-cycle");
  return 0;
}

int launch_dsm_fill(int W, int H, const float* dsm, const uint8_t* rgba, double r_cells, double tol_height, double tol_colour,
                    int max_cycles, void* workspace, float* dsm_out, uint8_t* rgba_out, int* dist2, uint8_t* filled,
                    adamvs_dsm_fill_stats* stats, hipStream_t st) {
  FillWs w;
  fill_layout(W, H, (char*)workspace, &w);
  const long n = (long)W * H;
  const int R = (int)ceil(r_cells);
  FillLevel& F0 = w.lv[0];
  if (hipMemsetAsync(w.counts, 0, 4 * sizeof(unsigned long long), st) != hipSuccess) return set_error(1, "dsm_fill: memset failed");
  int* g = (int*)w.rs_h;
  hipLaunchKernelGGL(k_fill_cols, fill_rows_grid(W, H), dim3(FILL_TILE), 0, st, W, H, R, dsm, g);
  hipLaunchKernelGGL(k_fill_rows, fill_rows_grid(W, H), dim3(FILL_TILE), 0, st, W, H, R, r_cells * r_cells, (const int*)g, dsm,
                     (const unsigned*)rgba, dist2, filled, F0.cls, F0.uh, F0.uc, w.counts);
  ADAMVS_CHECK_LAUNCH("dsm_fill: distance");
  unsigned long long host[4];
  hipError_t e = hipMemcpyAsync(host, w.counts, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "dsm_fill: %s", hipGetErrorString(e));
  *stats = adamvs_dsm_fill_stats{0, 1, 0.0, 0.0, (long)host[0], (long)host[1], n - (long)host[0] - (long)host[1]};
  if (host[1] > 0) {
    for (int l = 0; l + 1 < w.nl; ++l)
      hipLaunchKernelGGL(k_fill_coarsen, fill_rows_grid(w.lv[l + 1].W, w.lv[l + 1].H), dim3(FILL_TILE), 0, st, w.lv[l].W, w.lv[l].H,
                         (const uint8_t*)w.lv[l].cls, w.lv[l + 1].W, w.lv[l + 1].H, w.lv[l + 1].cls);
    ADAMVS_CHECK_LAUNCH("dsm_fill: coarse classes");
    const FillLevel& C1 = w.lv[1];
    const dim3 half = fill_rows_grid((W + 1) / 2, H);
    stats->converged = 0;
    for (int cyc = 0;; ++cyc) {
      if (hipMemsetAsync(w.counts + 2, 0, 2 * sizeof(unsigned long long), st) != hipSuccess) return set_error(1, "dsm_fill: memset failed");
      hipLaunchKernelGGL(k_fill_residual<true>, fill_rows_grid(W, H), dim3(FILL_TILE), 0, st, F0, (const uint8_t*)C1.cls, C1.W, C1.H,
                         w.rs_h, w.rs_c, w.counts + 2, (unsigned*)(w.counts + 3));
      ADAMVS_CHECK_LAUNCH("dsm_fill: residual");
      e = hipMemcpyAsync(host + 2, w.counts + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) return set_error((int)e, "dsm_fill: %s", hipGetErrorString(e));
      double rh, rc;
      float rcf;
      const unsigned rcb = (unsigned)host[3];
      memcpy(&rh, &host[2], 8);
      memcpy(&rcf, &rcb, 4);
      rc = rcf;
      stats->cycles = cyc;
      stats->residual_height = rh;
      stats->residual_colour = rc;
      if (rh <= tol_height && rc <= tol_colour) {
        stats->converged = 1;
        break;
      }
      if (cyc == max_cycles) break;
      if (int r = fill_coarse_correction(w, 0, st)) return r;
      for (int s = 0; s < 2; ++s) {
        hipLaunchKernelGGL(k_fill_smooth<true>, half, dim3(FILL_TILE), 0, st, F0, 0);
        hipLaunchKernelGGL(k_fill_smooth<true>, half, dim3(FILL_TILE), 0, st, F0, 1);
      }
      ADAMVS_CHECK_LAUNCH("dsm_fill: smooth");
    }
  }
  hipLaunchKernelGGL(k_fill_output, dim3((unsigned)((n + FILL_TILE - 1) / FILL_TILE)), dim3(FILL_TILE), 0, st, n, dsm, (const unsigned*)rgba,
                     (const uint8_t*)F0.cls, (const double*)F0.uh, (const float4*)F0.uc, dsm_out, (unsigned*)rgba_out);
  ADAMVS_CHECK_LAUNCH("dsm_fill: output");
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "dsm_fill: %s", hipGetErrorString(e));
  return 0;
}

}  // namespace adamvs
