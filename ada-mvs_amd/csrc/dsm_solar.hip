// The sun exposure of a height raster: the horizon of every cell in K lattice directions, the sky-view factor, the minutes of sun
// and the direct-beam energy per cell, and their sums per roof plane.  include/adamvs_hip.h "Solar" states the result; this file
// computes it with these kernels:
//
//   k_sol_horizon       one lane per lattice line, the lines of all K directions in one grid (blockIdx.y is the direction, a
//                       workgroup is one wave of 64 lines that start next to one another).  The lane finds its start cell in closed
//                       form, walks the line along w = -d and keeps the upper convex hull of the cells passed as a stack of
//                       (m, height): the pops that find the tangent from the cell to the hull are the pops that maintain the
//                       hull, so a line costs a push per cell and at most a pop per push (Dozier, Bruno and Downey 1981).  The top
//                       SOL_WIN entries of a lane's stack are a ring in LDS, [slot][lane] so that the lanes of a wave never share a
//                       bank; entry e of a line always sits in slot e mod SOL_WIN.  A push into a full ring first writes the
//                       oldest entry to the workspace, at the line's e-th cell (lines partition the raster: no offsets, no
//                       collision); when pops leave fewer than two entries in the ring the one below comes back.  No register array
//                       is indexed at run time.  The heights of four steps are loaded before the first of them is walked: the
//                       loads do not depend on the stack.
//   k_sol_svf           one lane per cell, the k loop of step 4 in fp64, operation by operation.
//   k_sol_expose        one lane per cell: per sector the cell's (n, h) once, then that sector's rows of the sample table, read
//                       with wave-uniform addresses (scalar loads).
//   k_sol_planes        one lane per cell: a run of equal labels in a wave (raster_prims.h wave_run) is summed into its first lane,
//                       which issues three integer atomics.
//
// Known weaknesses of this first form, measured by tools/solar_bench.py: the lines of a direction with dj != 0 that start in a
// column are a row apart, so the lanes of their waves read and write with a stride of W; every cell's pops are a dependent
// chain; the lines of the directions differ in length.  Integer atomics only (add, max), which commute; every other store goes to
// a slot that one lane owns: every output is bit-identical from run to run.  No workgroup waits on another.
#include <limits.h>
#include <string.h>

#include <vector>

#include "bld_union.h"
#include "block_prims.h"
#include "common.h"
#include "kernels.h"
#include "raster_prims.h"

#pragma clang fp contract(off)

namespace adamvs {

constexpr int SOL_WIN = ADAMVS_SOLAR_STACK_WINDOW;
constexpr int SOL_LANES = 64;                    // lines per workgroup of the horizon: one wave
constexpr int SOL_AHEAD = 4;                     // heights loaded before they are walked
constexpr int SOL_THREADS = RASTER_THREADS;
constexpr int SOL_NONE = INT_MIN;                // s outside V
constexpr int SOL_MAX_K = 32;
constexpr long long SOL_DOT_MAX = 1LL << 30;
static_assert((SOL_WIN & (SOL_WIN - 1)) == 0 && SOL_WIN >= 2, "the ring's slot is e & (SOL_WIN - 1) and holds the top two");

// the head of the workspace: control words, then the sample table
constexpr long SOL_OFF_SPILLS = 0;               // unsigned long long
constexpr long SOL_OFF_DEEPEST = 8;              // unsigned
constexpr long SOL_OFF_BAD = 16;                 // unsigned long long: labels outside 0 .. P
constexpr long SOL_OFF_TABLE = 512;
struct SolRow {
  double thr;
  int m, e, sx, sy, sz, k;
};
static_assert(sizeof(SolRow) == 32 && SOL_OFF_TABLE + 32L * ADAMVS_SOLAR_MAX_SAMPLES == ADAMVS_SOLAR_HEAD_BYTES, "the head of the workspace");

long solar_workspace_bytes(int W, int H, int K) { return ADAMVS_SOLAR_HEAD_BYTES + align256(8L * K * W * H); }

static const signed char SOL_DIRS_8[8][2] = ADAMVS_SOLAR_DIRS_8;
static const signed char SOL_DIRS_16[16][2] = ADAMVS_SOLAR_DIRS_16;
static const signed char SOL_DIRS_32[32][2] = ADAMVS_SOLAR_DIRS_32;

struct SolDirs {
  int di[SOL_MAX_K], dj[SOL_MAX_K];
};
static SolDirs sol_dirs(int K) {
  const signed char(*t)[2] = K == 8 ? SOL_DIRS_8 : K == 16 ? SOL_DIRS_16 : SOL_DIRS_32;
  SolDirs d;
  memset(&d, 0, sizeof(d));
  for (int k = 0; k < K; ++k) d.di[k] = t[k][0], d.dj[k] = t[k][1];
  return d;
}
static inline int sol_abs(int v) { return v < 0 ? -v : v; }
static inline int sol_min(int a, int b) { return a < b ? a : b; }
// the lines of look direction (di, dj): the cells whose predecessor lies outside the raster
static long sol_lines(int W, int H, int di, int dj) {
  const int a = sol_min(sol_abs(di), H), b = sol_min(sol_abs(dj), W);
  return (long)a * W + (long)(H - a) * b;
}

// ---- the horizon ------------------------------------------------------------------------------------------------------------
// One cell of a line: the lane's stack holds entries 0 .. sp - 1, the top `in` of them in the ring; c0 and step address the line's
// cells in the spill (entry e at the line's e-th cell).
__device__ __forceinline__ void sol_cell(int m, int v, long cell, int* __restrict__ on, int* __restrict__ oh, int2* spill, long c0, long step,
                                         int* ring_m, int* ring_v, int lane, int& sp, int& in, int& deepest, unsigned& spills) {
  if (v == SOL_NONE) {
    on[cell] = 0;
    oh[cell] = 0;
    return;
  }
  bool collinear = false;                                            // the top two entries and this cell lie on one line
  while (sp >= 2) {
    if (in < 2) {                                                    // the entry below the ring comes back: sp - in >= 1
      const int e = sp - in - 1;
      const int2 t = spill[c0 + (long)e * step];
      ring_m[(e & (SOL_WIN - 1)) * SOL_LANES + lane] = t.x;
      ring_v[(e & (SOL_WIN - 1)) * SOL_LANES + lane] = t.y;
      ++in;
      continue;
    }
    const int a1 = ((sp - 1) & (SOL_WIN - 1)) * SOL_LANES + lane, a2 = ((sp - 2) & (SOL_WIN - 1)) * SOL_LANES + lane;
    const int m1 = ring_m[a1], v1 = ring_v[a1], m2 = ring_m[a2], v2 = ring_v[a2];
    const long long far = (long long)(v2 - v) * (m - m1), near = (long long)(v1 - v) * (m - m2);
    if (far > near) {
      --sp;
      --in;
    } else {
      collinear = far == near;
      break;
    }
  }
  int n = 0, h = 0;
  if (sp >= 1) {                                                     // the top is in the ring: a pop leaves in >= 1, a push in >= 1
    const int a1 = ((sp - 1) & (SOL_WIN - 1)) * SOL_LANES + lane;
    const int m1 = ring_m[a1], v1 = ring_v[a1];
    if (v1 > v) n = m - m1, h = v1 - v;
  }
  on[cell] = n;
  oh[cell] = h;
  if (collinear) {                                                   // the top lies between its neighbours on the hull: the cell takes its place
    const int a1 = ((sp - 1) & (SOL_WIN - 1)) * SOL_LANES + lane;
    ring_m[a1] = m;
    ring_v[a1] = v;
    return;
  }
  if (in == SOL_WIN) {                                               // the oldest entry of the ring goes out: its slot is the push's
    const int e = sp - SOL_WIN;
    const int a = (e & (SOL_WIN - 1)) * SOL_LANES + lane;
    spill[c0 + (long)e * step] = make_int2(ring_m[a], ring_v[a]);
    --in;
    ++spills;
  }
  const int a = (sp & (SOL_WIN - 1)) * SOL_LANES + lane;
  ring_m[a] = m;
  ring_v[a] = v;
  ++sp;
  ++in;
  deepest = sp > deepest ? sp : deepest;
}

__global__ __launch_bounds__(SOL_LANES) void k_sol_horizon(int W, int H, SolDirs dirs, const int* __restrict__ s, int2* spill, int* __restrict__ hz_n,
                                                           int* __restrict__ hz_h, unsigned long long* spilled, unsigned* deepest_out) {
  __shared__ int ring_m[SOL_WIN * SOL_LANES];
  __shared__ int ring_v[SOL_WIN * SOL_LANES];
  const int k = blockIdx.y, lane = threadIdx.x;
  const int di = dirs.di[k], dj = dirs.dj[k], wi = -di, wj = -dj;
  const int a = min(abs(di), H), b = min(abs(dj), W);
  const long lines = (long)a * W + (long)(H - a) * b, n = (long)W * H;
  const long l = (long)blockIdx.x * SOL_LANES + lane;
  int deepest = 0;
  unsigned spills = 0;
  if (l < lines) {
    int i, j;
    if (l < (long)a * W) {                                           // the full rows on the side the lines enter from
      const int r = (int)(l / W);
      j = (int)(l - (long)r * W);
      i = wi > 0 ? r : H - a + r;
    } else {                                                         // the first or last b columns of the remaining rows
      const long t = l - (long)a * W;
      const int r = (int)(t / b), cc = (int)(t - (long)r * b);
      i = wi > 0 ? a + r : r;
      j = wj > 0 ? cc : W - b + cc;
    }
    int len = INT_MAX;                                               // the cells of the line: both coordinates stay inside
    if (wi > 0) len = min(len, (H - 1 - i) / wi + 1);
    if (wi < 0) len = min(len, i / -wi + 1);
    if (wj > 0) len = min(len, (W - 1 - j) / wj + 1);
    if (wj < 0) len = min(len, j / -wj + 1);
    const long step = (long)wi * W + wj, c0 = (long)i * W + j;
    int* on = hz_n + (long)k * n;
    int* oh = hz_h + (long)k * n;
    int2* sp_line = spill + (long)k * n;
    int sp = 0, in = 0;
    long c = c0;
    for (int m = 0; m < len; m += SOL_AHEAD, c += SOL_AHEAD * step) {
      int v[SOL_AHEAD];
#pragma unroll
      for (int u = 0; u < SOL_AHEAD; ++u) v[u] = m + u < len ? s[c + u * step] : SOL_NONE;
#pragma unroll
      for (int u = 0; u < SOL_AHEAD; ++u)
        if (m + u < len) sol_cell(m + u, v[u], c + u * step, on, oh, sp_line, c0, step, ring_m, ring_v, lane, sp, in, deepest, spills);
    }
  }
  for (int off = 32; off; off >>= 1) {
    deepest = max(deepest, __shfl_down(deepest, off, 64));
    spills += __shfl_down(spills, off, 64);
  }
  if (lane == 0) {
    if (spills) atomicAdd(spilled, (unsigned long long)spills);
    if (deepest) atomicMax(deepest_out, (unsigned)deepest);
  }
}

// ---- the sky-view factor ------------------------------------------------------------------------------------------------------
struct SolWeights {
  double w[SOL_MAX_K];
  int len2[SOL_MAX_K];
};

__global__ __launch_bounds__(SOL_THREADS) void k_sol_svf(int W, int H, int K, SolWeights wt, double q, const int* __restrict__ s,
                                                         const int* __restrict__ hz_n, const int* __restrict__ hz_h, double* __restrict__ svf) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * SOL_THREADS + threadIdx.x;
  if (c >= n) return;
  if (s[c] == SOL_NONE) {
    svf[c] = 0.0;
    return;
  }
  double acc = 0.0;
  for (int k = 0; k < K; ++k) {
    const int nn = hz_n[(long)k * n + c], h = hz_h[(long)k * n + c];
    double t = 1.0;
    if (h != 0) {
      const double L2 = ((double)nn * (double)nn) * ((double)wt.len2[k] * q);
      t = L2 / (L2 + (double)h * (double)h);
    }
    acc = acc + wt.w[k] * t;
  }
  svf[c] = acc;
}

// ---- the exposure -------------------------------------------------------------------------------------------------------------
struct SolFirst {
  int first[SOL_MAX_K + 1];                                          // the rows of sector k: first[k] .. first[k + 1] - 1
};

__global__ __launch_bounds__(SOL_THREADS) void k_sol_expose(int W, int H, int K, SolFirst f, const int* __restrict__ s, const int* __restrict__ hz_n,
                                                            const int* __restrict__ hz_h, const SolRow* __restrict__ rows,
                                                            const int* __restrict__ label, long P, const int* __restrict__ normal,
                                                            int* __restrict__ minutes, int* __restrict__ direct, unsigned long long* bad) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * SOL_THREADS + threadIdx.x;
  if (c >= n) return;
  if (s[c] == SOL_NONE) {
    minutes[c] = 0;
    direct[c] = 0;
    return;
  }
  int nx = 0, ny = 0, nz = 32768;
  if (label) {
    int lab = label[c];
    if (lab < 0 || (long)lab > P) {
      atomicAdd(bad, 1ull);
      lab = 0;
    }
    if (lab) nx = normal[3L * lab], ny = normal[3L * lab + 1], nz = normal[3L * lab + 2];
  }
  int mi = 0, dr = 0;
  for (int k = 0; k < K; ++k) {
    const int nn = hz_n[(long)k * n + c], h = hz_h[(long)k * n + c];
    const double dn = (double)nn, dh = (double)h;
    const int t1 = f.first[k + 1];
    for (int t = f.first[k]; t < t1; ++t) {                          // t is wave-uniform: the row comes through scalar loads
      const SolRow r = rows[t];
      if (h > 0 && dh > r.thr * dn) continue;                        // in shadow; equality is lit
      mi += r.m;
      long long dot = (long long)nx * r.sx + (long long)ny * r.sy + (long long)nz * r.sz;
      dot = dot < 0 ? 0 : dot > SOL_DOT_MAX ? SOL_DOT_MAX : dot;
      dr += (int)(((long long)r.e * dot) >> 30);
    }
  }
  minutes[c] = mi;
  direct[c] = dr;
}

// ---- the plane table ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SOL_THREADS) void k_sol_planes(int W, int H, const int* __restrict__ s, const int* __restrict__ label, long P,
                                                            const int* __restrict__ minutes, const int* __restrict__ direct, long long* table) {
  const long n = (long)W * H;
  const long c = (long)blockIdx.x * SOL_THREADS + threadIdx.x;       // no early return: every lane takes part in the shuffles
  const int lane = threadIdx.x & 63;
  int key = 0, j = 0;                                                // label + 1 on V, 0 elsewhere
  long long sm = 0, sd = 0;
  if (c < n && s[c] != SOL_NONE) {
    const int lab = label ? label[c] : 0;
    if (lab >= 0 && (long)lab <= P) {
      key = lab + 1;
      j = (int)((unsigned)c % (unsigned)W);
      sm = minutes[c];
      sd = direct[c];
    }
  }
  if (__ballot(key != 0) == 0ull) return;                            // wave-uniform
  bool head;
  int end;
  wave_run(key, j, lane, head, end);
  for (int off = 1; off < 64; off <<= 1) {
    const long long t_sm = __shfl_down(sm, off, 64), t_sd = __shfl_down(sd, off, 64);
    if (lane + off <= end) {
      sm += t_sm;
      sd += t_sd;
    }
  }
  if (!head) return;
  const long T = P + 1, k = key - 1;
  add_nonzero(table + k, end - lane + 1);
  add_nonzero(table + T + k, sm);
  add_nonzero(table + 2 * T + k, sd);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int launch_solar_horizon(int W, int H, int K, const int* s, void* workspace, int* hz_n, int* hz_h, adamvs_solar_stats* stats, hipStream_t st) {
  const SolDirs dirs = sol_dirs(K);
  char* p = (char*)workspace;
  memset(stats, 0, sizeof(*stats));
  long most = 0;
  for (int k = 0; k < K; ++k) {
    const long lines = sol_lines(W, H, dirs.di[k], dirs.dj[k]);
    stats->lines += lines;
    most = lines > most ? lines : most;
  }
  BldClock clock;
  clock.mark(0, st);
  hipError_t e = hipMemsetAsync(p, 0, SOL_OFF_BAD, st);
  if (e != hipSuccess) return set_error((int)e, "solar_horizon: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_sol_horizon, dim3((unsigned)((most + SOL_LANES - 1) / SOL_LANES), (unsigned)K), dim3(SOL_LANES), 0, st, W, H, dirs, s,
                     (int2*)(p + ADAMVS_SOLAR_HEAD_BYTES), hz_n, hz_h, (unsigned long long*)(p + SOL_OFF_SPILLS), (unsigned*)(p + SOL_OFF_DEEPEST));
  ADAMVS_CHECK_LAUNCH("solar_horizon");
  clock.mark(1, st);
  unsigned long long host[2] = {0ull, 0ull};
  e = hipMemcpyAsync(host, p, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return set_error((int)e, "solar_horizon: %s", hipGetErrorString(e));
  stats->spills = (long)host[0];
  stats->deepest = (int)(unsigned)host[1];
  stats->ms = clock.ms(0);
  return 0;
}

int launch_solar_svf(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, const double* weight, double q, double* svf,
                     hipStream_t st) {
  const SolDirs dirs = sol_dirs(K);
  SolWeights wt;
  memset(&wt, 0, sizeof(wt));
  for (int k = 0; k < K; ++k) {
    wt.w[k] = weight[k];
    wt.len2[k] = dirs.di[k] * dirs.di[k] + dirs.dj[k] * dirs.dj[k];
  }
  hipLaunchKernelGGL(k_sol_svf, dim3(raster_blocks((long)W * H)), dim3(SOL_THREADS), 0, st, W, H, K, wt, q, s, hz_n, hz_h, svf);
  ADAMVS_CHECK_LAUNCH("solar_svf");
  return 0;
}

int launch_solar_expose(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, int T, const int* sector, const double* thr,
                        const int* minutes_w, const int* energy_w, const int* sun, const int* label, long P, const int* normal, void* workspace,
                        int* minutes, int* direct, hipStream_t st) {
  char* p = (char*)workspace;
  std::vector<SolRow> rows((size_t)T);
  SolFirst f;
  memset(&f, 0, sizeof(f));
  for (int t = 0; t < T; ++t) {
    rows[t] = SolRow{thr[t], minutes_w[t], energy_w[t], sun[3 * t], sun[3 * t + 1], sun[3 * t + 2], sector[t]};
    ++f.first[sector[t] + 1];
  }
  for (int k = 0; k < SOL_MAX_K; ++k) f.first[k + 1] += f.first[k];
  unsigned long long* bad = (unsigned long long*)(p + SOL_OFF_BAD);
  hipError_t e = hipMemsetAsync(bad, 0, 8, st);
  if (e == hipSuccess && T) e = hipMemcpyAsync(p + SOL_OFF_TABLE, rows.data(), sizeof(SolRow) * (size_t)T, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return set_error((int)e, "solar_expose: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_sol_expose, dim3(raster_blocks((long)W * H)), dim3(SOL_THREADS), 0, st, W, H, K, f, s, hz_n, hz_h,
                     (const SolRow*)(p + SOL_OFF_TABLE), label, P, normal, minutes, direct, bad);
  ADAMVS_CHECK_LAUNCH("solar_expose");
  unsigned long long host = 0ull;
  e = hipMemcpyAsync(&host, bad, 8, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);                 // `rows` lives until the copy has been done
  if (e != hipSuccess) return set_error((int)e, "solar_expose: %s", hipGetErrorString(e));
  if (host) return set_error(ADAMVS_SOLAR_BAD_LABEL, "solar_expose: %llu cells carry a label outside 0 .. P=%ld", host, P);
  return 0;
}

int launch_solar_plane_sums(int W, int H, const int* s, const int* label, long P, const int* minutes, const int* direct, long long* table,
                            hipStream_t st) {
  const hipError_t e = hipMemsetAsync(table, 0, 24 * (size_t)(P + 1), st);
  if (e != hipSuccess) return set_error((int)e, "solar_plane_sums: %s", hipGetErrorString(e));
  hipLaunchKernelGGL(k_sol_planes, dim3(raster_blocks((long)W * H)), dim3(SOL_THREADS), 0, st, W, H, s, label, P, minutes, direct, table);
  ADAMVS_CHECK_LAUNCH("solar_planes");
  return 0;
}

}  // namespace adamvs
