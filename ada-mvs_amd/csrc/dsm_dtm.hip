// Ground filter of a finalised DSM: grey-scale openings with square windows and the progressive morphological filter built
// on them.  include/adamvs_hip.h "DSM ground filter" states the result; this file computes it with two kernels:
//
//   k_dtm_row<MAX, MODE>  the running min (MAX = false) or max (MAX = true) of a row over the window [x - r, x + r].  One
//                         workgroup per DTM_TILE-cell segment of a row: the segment and r cells either side go into LDS
//                         (cells outside the grid and cells without a value as the operator's neutral element, +inf / -inf),
//                         then windows are formed by doubling, m_j(x) = op(m_{j-1}(x), m_{j-1}(x + 2^(j-1))), ping-ponged
//                         between two LDS arrays, p = floor(log2(2r + 1)) steps; the window of 2r + 1 cells is the two
//                         overlapping m_p(x) and m_p(x + 2r + 1 - 2^p).  log2(r) LDS steps per cell instead of r reads, one
//                         form for every 1 <= r <= 1024 (no switch-over radius), 2 (DTM_TILE + 2 r_max) floats = 24 KB of LDS.
//                         MODE: DTM_PASS writes the running value for the next pass; DTM_OPEN is the last pass of an opening
//                         (O on valid cells, NaN on empty ones); DTM_FLAG is DTM_OPEN plus the flag / count step of a level.
//   k_dtm_transpose       64 x 64 tiles through LDS.  The column passes are row passes on the transposed raster: lanes run
//                         along the window, so the same doubling serves both axes and every global access is coalesced.
//
// One opening is  row min, transpose, row min, row max, transpose, row max: six passes of 8 bytes per cell (the halo adds
// 2r / DTM_TILE to the reads of a row pass; those re-reads hit in L2).  Min and max only select input values: the result is
// exact, and the counts are integer sums, so the output is bit-identical from run to run.
// Plain launches in stream order; every loop is bounded by W, H or r.
#include "common.h"
#include "kernels.h"

namespace adamvs {

constexpr int DTM_THREADS = 256;
constexpr int DTM_LDS = DTM_TILE + 2 * ADAMVS_DTM_MAX_RADIUS;      // the longest segment with its halo
constexpr int DTM_TT = 64;                                         // side of a transpose tile
constexpr int DTM_FLAG_ROWS = 512;                                 // most rows of workgroups in the pass that counts
enum : int { DTM_PASS = 0, DTM_OPEN = 1, DTM_FLAG = 2 };

// counters in the workspace: [0] valid cells, [k] cells flagged at level k (1 <= k <= ADAMVS_DTM_MAX_LEVELS)
constexpr int DTM_COUNTERS = ADAMVS_DTM_MAX_LEVELS + 1;

struct DtmFlag {
  const float* zprev;      // DTM_OPEN / DTM_FLAG: Z_{k-1}; the cell's own value decides valid / empty (may be the buffer `out`)
  uint8_t* level;          // DTM_FLAG
  unsigned long long* counts;
  double dh;
  int k;
};

template <bool MAX> __device__ __forceinline__ float dtm_op(float a, float b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }

// in [rows][width] -> out [rows][width].  grid: x = segments of a row, y = rows (strided past 65535).
template <bool MAX, int MODE>
__global__ __launch_bounds__(DTM_THREADS) void k_dtm_row(int width, int rows, int r, const float* __restrict__ in, float* out,
                                                         const DtmFlag f) {
  __shared__ float s_a[DTM_LDS], s_b[DTM_LDS];
  const float neutral = MAX ? -INFINITY : INFINITY;
  const int x0 = blockIdx.x * DTM_TILE;
  const int n_out = min(DTM_TILE, width - x0);
  const int w = 2 * r + 1;
  const int N = n_out + 2 * r;                      // <= DTM_LDS; entry k is column x0 - r + k
  const int p = 31 - __clz(w);                      // 2^p <= w < 2^(p+1), p >= 1
  const int tail = w - (1 << p);                    // the second m_p starts here: 0 <= tail < 2^p
  unsigned n_valid = 0, n_flag = 0;
  for (int row = blockIdx.y; row < rows; row += gridDim.y) {       // block-uniform: every lane reaches the barriers
    const long base = (long)row * width;
    for (int k = threadIdx.x; k < N; k += DTM_THREADS) {
      const int x = x0 - r + k;
      float v = neutral;
      if (x >= 0 && x < width) {
        v = in[base + x];
        if (!__builtin_isfinite(v)) v = neutral;
      }
      s_a[k] = v;
    }
    __syncthreads();
    float* src = s_a;
    float* dst = s_b;
    for (int j = 1; j <= p; ++j) {
      const int half = 1 << (j - 1);
      const int lim = N - 2 * half + 1;             // m_j exists for k in [0, lim); lim >= n_out + tail >= 1
      for (int k = threadIdx.x; k < lim; k += DTM_THREADS) dst[k] = dtm_op<MAX>(src[k], src[k + half]);
      __syncthreads();
      float* t = src;
      src = dst;
      dst = t;
    }
    for (int k = threadIdx.x; k < n_out; k += DTM_THREADS) {
      const float m = dtm_op<MAX>(src[k], src[k + tail]);          // k + tail <= N - 2^p: inside m_p
      const long c = base + x0 + k;
      if (MODE == DTM_PASS) {
        out[c] = m;
      } else {
        const float z = f.zprev[c];
        const bool valid = __builtin_isfinite(z);
        out[c] = valid ? m : __uint_as_float(0x7fc00000u);
        if (MODE == DTM_FLAG) {
          uint8_t lv = valid ? 0 : 255;
          if (f.k > 1) lv = f.level[c];
          if (lv == 0 && (double)z - (double)m > f.dh) {
            lv = (uint8_t)f.k;
            ++n_flag;
          }
          if (f.k == 1 || lv == f.k) f.level[c] = lv;
          n_valid += valid;
        }
      }
    }
    __syncthreads();                                 // the next row overwrites both arrays
  }
  if (MODE == DTM_FLAG) {
    // wave sums, then one integer atomicAdd per workgroup and counter (the grid of this pass is capped, see dtm_open)
    __shared__ unsigned s_n[2][DTM_THREADS / 64];
    for (int off = 32; off; off >>= 1) {
      n_valid += __shfl_xor(n_valid, off);
      n_flag += __shfl_xor(n_flag, off);
    }
    if ((threadIdx.x & 63) == 0) {
      s_n[0][threadIdx.x >> 6] = n_valid;
      s_n[1][threadIdx.x >> 6] = n_flag;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int wv = 1; wv < DTM_THREADS / 64; ++wv) {
        n_valid += s_n[0][wv];
        n_flag += s_n[1][wv];
      }
      if (f.k == 1 && n_valid) atomicAdd(f.counts, (unsigned long long)n_valid);
      if (n_flag) atomicAdd(f.counts + f.k, (unsigned long long)n_flag);
    }
  }
}

// in [rows][cols] -> out [cols][rows].  One workgroup per 64 x 64 tile, tiles numbered row-major along x of a 1-D grid.
__global__ __launch_bounds__(DTM_THREADS) void k_dtm_transpose(int cols, int rows, int tiles_x, const float* __restrict__ in,
                                                               float* __restrict__ out) {
  __shared__ float s_t[DTM_TT][DTM_TT + 1];
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int lx = threadIdx.x & (DTM_TT - 1), ly = threadIdx.x / DTM_TT;      // 64 x 4 lanes
  const int c0 = tx * DTM_TT, r0 = ty * DTM_TT;
  for (int i = ly; i < DTM_TT; i += DTM_THREADS / DTM_TT) {
    const int y = r0 + i, x = c0 + lx;
    if (y < rows && x < cols) s_t[i][lx] = in[(long)y * cols + x];
  }
  __syncthreads();
  for (int i = ly; i < DTM_TT; i += DTM_THREADS / DTM_TT) {
    const int x = c0 + i, y = r0 + lx;                // out row x, out column y
    if (x < cols && y < rows) out[(long)x * rows + y] = s_t[lx][i];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------

// Workspace: the counters (256 B), then two rasters of fp32.
long dtm_workspace_bytes(int W, int H) { return 256 + 2 * align256(4L * W * H); }

struct DtmWs {
  unsigned long long* counts;
  float *a, *b;
};

static DtmWs dtm_layout(int W, int H, void* workspace) {
  char* base = (char*)workspace;
  return DtmWs{(unsigned long long*)base, (float*)(base + 256), (float*)(base + 256 + align256(4L * W * H))};
}

static dim3 dtm_row_grid(int width, int rows) { return dim3((unsigned)cdiv(width, DTM_TILE), (unsigned)min(rows, 65535)); }

static void dtm_transpose(int cols, int rows, const float* in, float* out, hipStream_t st) {
  const int tiles_x = cdiv(cols, DTM_TT), tiles_y = cdiv(rows, DTM_TT);
  hipLaunchKernelGGL(k_dtm_transpose, dim3((unsigned)((long)tiles_x * tiles_y)), dim3(DTM_THREADS), 0, st, cols, rows, tiles_x, in, out);
}

// One opening of src into dst (which may be src: the last pass reads and writes a cell's own entry only).
template <int MODE>
static void dtm_open(int W, int H, const float* src, int r, const DtmWs& ws, float* dst, DtmFlag f, hipStream_t st) {
  const DtmFlag none{nullptr, nullptr, nullptr, 0.0, 0};
  const dim3 rows_g = dtm_row_grid(W, H), cols_g = dtm_row_grid(H, W), blk(DTM_THREADS);
  f.zprev = src;
  hipLaunchKernelGGL((k_dtm_row<false, DTM_PASS>), rows_g, blk, 0, st, W, H, r, src, ws.a, none);
  dtm_transpose(W, H, ws.a, ws.b, st);
  hipLaunchKernelGGL((k_dtm_row<false, DTM_PASS>), cols_g, blk, 0, st, H, W, r, (const float*)ws.b, ws.a, none);
  hipLaunchKernelGGL((k_dtm_row<true, DTM_PASS>), cols_g, blk, 0, st, H, W, r, (const float*)ws.a, ws.b, none);
  dtm_transpose(H, W, ws.b, ws.a, st);
  dim3 last_g = rows_g;                              // the counting pass: fewer workgroups, each striding over rows, so that
  if (MODE == DTM_FLAG) last_g.y = min(last_g.y, (unsigned)DTM_FLAG_ROWS);      // the counters see few atomics
  hipLaunchKernelGGL((k_dtm_row<true, MODE>), last_g, blk, 0, st, W, H, r, (const float*)ws.a, dst, f);
}

int launch_dsm_open(int W, int H, const float* src, int r, void* workspace, float* dst, hipStream_t st) {
  const DtmWs ws = dtm_layout(W, H, workspace);
  dtm_open<DTM_OPEN>(W, H, src, r, ws, dst, DtmFlag{nullptr, nullptr, nullptr, 0.0, 0}, st);
  ADAMVS_CHECK_LAUNCH("dsm_open");
  return 0;
}

int launch_dtm_classify(int W, int H, const float* dsm, int levels, const int* radius, const double* dh, void* workspace,
                        uint8_t* level, float* opened, adamvs_dtm_stats* stats, hipStream_t st) {
  const DtmWs ws = dtm_layout(W, H, workspace);
  if (hipMemsetAsync(ws.counts, 0, DTM_COUNTERS * sizeof(unsigned long long), st) != hipSuccess)
    return set_error(1, "dtm_classify: memset failed");
  for (int k = 1; k <= levels; ++k) {
    dtm_open<DTM_FLAG>(W, H, k == 1 ? dsm : (const float*)opened, radius[k - 1], ws, opened, DtmFlag{nullptr, level, ws.counts, dh[k - 1], k},
                       st);
    ADAMVS_CHECK_LAUNCH("dtm_classify");
  }
  unsigned long long host[DTM_COUNTERS];
  hipError_t e = hipMemcpyAsync(host, ws.counts, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "dtm_classify: %s", hipGetErrorString(e));
  memset(stats, 0, sizeof(*stats));
  stats->levels = levels;
  stats->cells_valid = (long)host[0];
  for (int k = 1; k <= levels; ++k) {
    stats->cells_level[k] = (long)host[k];
    stats->cells_object += (long)host[k];
  }
  stats->cells_ground = stats->cells_valid - stats->cells_object;
  stats->cells_level[0] = stats->cells_ground;
  stats->cells_empty = (long)W * H - stats->cells_valid;
  return 0;
}

}  // namespace adamvs
