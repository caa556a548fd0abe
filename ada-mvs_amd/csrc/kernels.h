// Launchers shared between the kernel translation units and the C-ABI glue.
#pragma once
#include <stdlib.h>

#include "common.h"
#include "options.h"
#include "planes.h"
#include "../../include/adamvs_hip.h"

namespace adamvs {

enum { PRECISION_FP32 = 0, PRECISION_BF16X3 = 1 };

// zero fill / copy as kernels (api.hip: a captured hipGraph must not contain memset / memcpy nodes)
hipError_t zero_floats(float* p, size_t n, hipStream_t st);
hipError_t copy_floats(const float* src, float* dst, size_t n, hipStream_t st);

struct FuseWeights {          // mirrors adamvs_fuse_weights in include/adamvs_hip.h
  const float* conv1;         // [1][9][C/4][64]
  const float* gates1; const float* gates1_b;   // [1][9][4][64], [16]
  const float* cand1;  const float* cand1_b;    // [12][4][64] (two-row form, fp32), [16]
  const float* conv2;                           // [1][9][2][64]
  const float* gates2; const float* gates2_b;   // [2][9][8][64], [32]
  const float* cand2;  const float* cand2_b;    // [1][9][8][64], [16]
  const float* upconv1; const float* upconv1_b; // [1][9][4][64], [16]
  const float* final_w;                         // [73]
  // fp32 only: the GRU convolutions in the F(2x2, 3x3) form (slice_roles_wino.h), U = G g Gt as fragments [NT][4][4][cin/4][64]
  const float* gates1_w; const float* gates2_w; const float* cand2_w; const float* cand1_w;
};
int gru_wino_mask();          // which GRU convolutions run in the F(2x2, 3x3) form in one-role launches (slice_red.hip)
// two more bits of option gru_wino, both SET = the launches of before: conv2 in a launch of its own although the F(2x2, 3x3) gate
// tiles of level 1 hold its window (clear: Gates1Conv2WinoRole); cand1 with a launch of its own on 8 x 16 tiles (clear: 8 x 32)
// and one that is CLEAR by default: slot A of the pipelined schedule 1 as Gates1Conv2WinoRole alone instead of gates1 | conv2 (not
// measured at the sizes that take schedule 1: it stays an opt-in until it is)
enum { GRU_WINO_CONV2_APART = 16, GRU_WINO_CAND1_TILE16 = 32, GRU_WINO_SLOT_A_FUSED = 64 };
inline bool conv2_in_gates1_enabled() { return !(gru_wino_mask() & GRU_WINO_CONV2_APART); }
inline bool cand1_tile32_enabled() { return !(gru_wino_mask() & GRU_WINO_CAND1_TILE16); }

struct StepBuffers {          // all channel-last
  float* h1; float* rh1; float* u1;              // [B][hw][8]
  float* c2; float* h2; float* rh2; float* u2;   // [B][hw/4][16]
};

// State of the software-pipelined recurrence (recurrence.hip): h1 of step t in h1[t % 4]; h2 and conv2's output of step t
// in h2[t % 2], c2[t % 2]
struct GruStateRing {
  float* h1[4]; float* rh1; float* u1;              // [B][hw][8]
  float* c2[2]; float* h2[2]; float* rh2; float* u2;   // [B][hw/4][16]
};
struct RecurLags { int c2, dec; };       // hypotheses by which cand2 / the decoder run behind level 1
int recurrence_mode(int precision, long pixels);
RecurLags recurrence_lags(int schedule, int precision);
int launch_recur_pipeline_step(const GruStateRing& rb, const FuseWeights& fw, int B, int h, int w, int D, int t, const float* c1_t,
                               float* vol_dec, int D_vol, int d_dec, int in_up, int precision, int schedule, hipStream_t st);
// schedule 0 with conv2(t-1) inside the launch of gates1(t) (slice_red.hip): whether it applies, and its step t = 0 .. D
bool conv2_in_gates1_applies(const FuseWeights& fw, int h, int w, int precision);
int launch_lagged_step(const FuseWeights& fw, int B, int h, int w, int D, int t, const float* c1_t, const float* h1_prev, float* h1_new,
                       float* rh1, float* u1, float* c2, const float* h2_prev, float* h2_new, float* rh2, float* u2, float* vol_dec, int D_vol,
                       int d_dec, int in_up, hipStream_t st);
int launch_soft_argmin_chunk(const float* vol, int vol_D, PlaneSrc planes, int D, int d0, int nd, float* acc, int first, int last,
                             float* depth, float* conf, int B, int h, int w, int in_up, hipStream_t st);
int sweep_chunk_planes(int D);
int launch_sweep_conv1_chunk(const float* feat, const float* rt, PlaneSrc planes, const float* vw, const float* w1pk,
                             float* c1_chunk, float* sim_ws, int B, int S, int C, int D, int d0, int d1, int h, int w, int precision,
                             int eps_in_numerator, hipStream_t st);

int launch_conv1(const float* cost, const float* w, float* c1, int B, int C, int h, int w_, int precision, hipStream_t st);
int launch_conv1_bf16x3(const float* cost, const float* w, float* c1, int N, int C, int h, int w_, hipStream_t st);
int launch_gru_convs_bf16x3(const float* c1, const FuseWeights& fw, const StepBuffers& sb, int B, int h, int w, int d,
                            float** h1_now, float** h2_now, hipStream_t st);
// step d of a stage; *h1_now / *h2_now (optional) receive the buffers holding the states afterwards (sb.h1 / sb.h2, or
// sb.rh1 / sb.rh2 after an even step of the split-bf16 path, whose fused GRU kernels alternate the two)
int launch_slice_step(const float* c1, const FuseWeights& fw, const StepBuffers& sb, float* vol, int B, int h, int w, int D,
                      int d, int in_up, int precision, hipStream_t st, float** h1_now = nullptr, float** h2_now = nullptr);
// (csrc/costreg2d.hip, k_conv_dd_resident)
enum { GRU_PRO_NONE = 0, GRU_PRO_GATES = 1, GRU_PRO_OUT = 2 };
struct GruPro {
  int mode;
  const float* f;            // [N][npix][D] (k_conv_dd_resident); k_conv_small: [N][npix][2 hc] + the half's channel offset
  const float* o;            // [N][npix][D] (GRU_PRO_OUT); k_conv_small: [N][npix][hc]
  const double* part_f;      // partial sums of f's group: [(n * 2 + group_f) * parts_f + k][2]
  const double* part_o;      // [(n * parts_o + k)][2]
  int parts_f, group_f, parts_o;
  const float* gn_f;         // [2][hc]: weight, bias of f's norm
  const float* gn_o;         // [2][hc]: output_norm
  float* state_out;          // [N][npix][D]
  float* R; int RW;          // [N][npix][RW] or null
  int hc, count;             // real channels; pixels x real channels of a sample (the norm's population)
  float eps;
};

constexpr int GN_PARTS_LIMIT = 2048;     // partial sums per (sample, group) the GroupNorm buffers of msred.hip hold
// A convolution writes its GroupNorm partials itself (one dependent launch fewer) while the stage is launch-bound: every block
// of the consumer finishes the reduction on its own, which is free for 64 partials and not for 1152 x 16 samples (measured at
// 16 tiles per step: 136 -> 147 ms with epilogue partials everywhere).
inline bool gn_epilogue_partials(long parts, int samples) { return parts > 0 && parts <= GN_PARTS_LIMIT && parts * samples <= 4096; }
int launch_conv_pair(const float* srcA, int CA, const float* srcB, int CB, const float* wpk, const float* bias, float* out,
                     int cout, int B, int h, int w, hipStream_t st, double* gn_part = nullptr, int gn_hc = 0, int gn_groups = 0,
                     int* gn_parts = nullptr, const GruPro* pro = nullptr);
bool conv_pair_epilogue_partials(int B, int h, int w);       // whether launch_conv_pair writes the GroupNorm partials itself
// one stride-1 layer with the GroupNorm partial sums of its output in the epilogue when the small-grid kernel takes it
// (*gn_parts > 0), plain otherwise (*gn_parts = 0): MS-REDNet's deep levels
// Folding pays while a stage is bound by its dependent launches: one or two tiles per step (measured at cfg3's shape: 51.3 ->
// 53.8 maps/s at one tile; 92.2 -> 88.7 at four and 115.4 -> 111.6 at sixteen, where the window halo's recomputed sigmoid /
// tanh and the per-workgroup reductions cost more than the launches they replace).  Option red_fold_applies = 0 / 1 forces.
inline bool gru_fold_enabled(int samples) {
  const int forced = opt(OPT_RED_FOLD_APPLIES);
  return forced >= 0 ? forced != 0 : samples <= 2;
}
bool can_fold_gru_applies(int N, int D, int h, int w);
int launch_conv_dd_gates_gn(const float* in, const float* wpk_r, const float* bias_r, const float* skip_r, float* out_r,
                            const float* wpk_u, const float* bias_u, const float* skip_u, float* out_u, int N, int D, int h, int w,
                            hipStream_t st, double* gn_part, int gn_n, int* gn_parts, const GruPro* pro = nullptr);
int launch_conv_dd_gn(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D, int h, int w,
                      hipStream_t st, double* gn_part, int gn_n, int gn_group, int gn_ngroups, int* gn_parts, const GruPro* pro = nullptr);
int launch_soft_argmin(const float* vol, const float* planes, float* depth, float* conf, int B, int D, int h, int w,
                       int in_up, hipStream_t st);
int launch_sweep_conv1(const float* feat, const float* rt, PlaneSrc planes, const float* vw, const float* w1pk,
                       float* c1, float* sim_ws, int B, int S, int C, int D, int h, int w, int precision, int eps_in_numerator,
                       hipStream_t st);
int launch_sweep_variance(const float* feat, const float* rt, const float* planes, float* out_a, int Da, float* out_b, int Db,
                          int B, int S, int C, int D, int h, int w, hipStream_t st);
size_t sweep_workspace_floats(int B, int C, int D, int h, int w);
int launch_cost_reg_net_2d(const float* x, const float* wpk, float* ws, float* score, int N, int D, int h, int w,
                           int precision, hipStream_t st, float* sm_vw = nullptr, float* sm_pd = nullptr,
                           const PlaneSrc* sm_planes = nullptr, int sm_B = 1, int n_planes = 0, int blocks = -1);
size_t cost_reg_weight_floats(int D, int precision);        // floats of the packed weight blob at width D (0: unsupported)
int costreg_width(int D);            // the width CostRegNet2D runs at for D hypotheses (next supported; 0: none)
int costreg_width_bf16x3(int D);
bool cost_reg_softmax_fusable(int D, int precision, const PlaneSrc& planes);
int launch_conv_dd_bf16x3(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D,
                          int hi, int wi, int ho, int wo, int mode, int relu, hipStream_t st, float* sm_vw = nullptr,
                          float* sm_pd = nullptr, const PlaneSrc* sm_planes = nullptr, int sm_B = 1, int n_planes = 0);
bool costreg_bf16x3_depth_supported(int D);
bool wino_depth_supported(int D);
bool cost_reg_winograd(int D, int precision);
bool wino_softmax_fused();
size_t wino_softmax_part_floats(int N, int D, int h, int w);
int launch_conv_wino_softmax(const float* in, const float* wpk, const float* bias, float* part, const PlaneSrc& planes, float* vw, float* pd,
                             int N, int B, int D, int n_planes, int h, int w, hipStream_t st);
int launch_conv_wino(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D, int h, int w,
                     int relu, hipStream_t st);
// the same two in the F(2x4, 3x3) form (costreg2d_wino24.hip; wpk from packing.pack_reg_layer_wino24)
bool cost_reg_wino24(int D, int h, int w);        // whether conv0 / prob of a network on h x w maps take it
int conv_wino24_fold(int h, int w, int blocks = -1);   // the FOLD (1, 2, 4) of the blocks a layer on h x w maps takes; blocks: -1 by the map, or forced
int cost_reg_wino24_fold(int N, int D, int h, int w);   // conv2 / conv4 of a network on h x w maps at that level: the FOLD, 0 = F(2x2, 3x3)
int launch_conv_wino24_softmax(const float* in, const float* wpk, const float* bias, float* part, const PlaneSrc& planes, float* vw, float* pd,
                               int N, int B, int D, int n_planes, int h, int w, hipStream_t st);
int launch_conv_wino24(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D, int h, int w,
                       int relu, hipStream_t st, int blocks = -1);

// Dw >= D: channels per pixel of sim (the width CostRegNet2D runs at); channels [D, Dw) are written as zeros
int launch_pair_similarity(const float* feat, const float* rt, PlaneSrc planes, float* sim, int B, int S, int C, int D, int h,
                           int w, hipStream_t st, int Dw = 0);
// n_planes <= D hypothesis planes for D score channels (0: D)
int launch_softmax_regress(const float* score, PlaneSrc planes, float* vw, float* pd, int S, int B, int D, int h, int w,
                           hipStream_t st, int n_planes = 0);
bool costreg_depth_supported(int D);

// fusion.hip: geometric-consistency filtering and point emission (include/adamvs_hip.h, "depth-map fusion")
constexpr int FUSION_TILE = ADAMVS_FUSION_TILE;
constexpr int FUSION_MAX_SOURCES = ADAMVS_FUSION_MAX_SOURCES;
int launch_geo_consistency(const float* ref_depth, const float* ref_conf, int H, int W, const adamvs_fusion_source* srcs, int N,
                           float prob_threshold, float pix_threshold, float rel_depth_threshold, int min_consistent, uint8_t* count,
                           float* fused, unsigned* block_kept, hipStream_t st);
int launch_fusion_scan(const unsigned* counts, unsigned* offsets, int nblocks, hipStream_t st);
int launch_fusion_emit(const float* fused, const uint8_t* rgba, int H, int W, const double* camera, const unsigned* offsets, double* xyz,
                       uint8_t* rgb, long capacity, hipStream_t st);

// dsm.hip: rasterisation of a point cloud into a DSM and a true orthophoto (include/adamvs_hip.h, "DSM")
constexpr int DSM_TILE = 256;
int launch_dsm_accumulate(const adamvs_dsm_grid& g, const double* xyz, long n, long seq0, int mode, unsigned long long* key,
                          unsigned* count, long long* sum, hipStream_t st);
int launch_dsm_claim(const adamvs_dsm_grid& g, const double* xyz, const uint8_t* rgb, long n, long seq0, const unsigned long long* key,
                     unsigned* color, hipStream_t st);
int launch_dsm_finalize(const adamvs_dsm_grid& g, const unsigned long long* key, const unsigned* count, const long long* sum,
                        const unsigned* color, int mode, int min_count, float* dsm, uint16_t* count16, unsigned* rgba, hipStream_t st);

// dsm_fill.hip: bounded harmonic gap fill of a finalised DSM (include/adamvs_hip.h, "DSM gap fill")
long dsm_fill_workspace_bytes(int W, int H);
int launch_dsm_fill(int W, int H, const float* dsm, const uint8_t* rgba, double r_cells, double tol_height, double tol_colour,
                    int max_cycles, void* workspace, float* dsm_out, uint8_t* rgba_out, int* dist2, uint8_t* filled,
                    adamvs_dsm_fill_stats* stats, hipStream_t st);

// dsm_dtm.hip: grey-scale opening and the progressive morphological ground filter (include/adamvs_hip.h, "DSM ground filter")
constexpr int DTM_TILE = ADAMVS_DTM_TILE;
long dtm_workspace_bytes(int W, int H);
int launch_dsm_open(int W, int H, const float* src, int r, void* workspace, float* dst, hipStream_t st);
int launch_dtm_classify(int W, int H, const float* dsm, int levels, const int* radius, const double* dh, void* workspace,
                        uint8_t* level, float* opened, adamvs_dtm_stats* stats, hipStream_t st);

// dsm_buildings.hip: candidate mask, flatness flags, component labels and the per-component table (include/adamvs_hip.h,
// "Building extraction")
constexpr int BLD_TILE_W = ADAMVS_BLD_TILE_W, BLD_TILE_H = ADAMVS_BLD_TILE_H;
long bld_workspace_bytes(int W, int H);
int launch_bld_flags(int W, int H, const float* dsm, const float* ndsm, double min_height, int r_open, int s, double smooth_tol,
                     void* workspace, uint8_t* flags, hipStream_t st);
int launch_bld_label(int W, int H, const uint8_t* flags, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st);
int launch_bld_table(int W, int H, const uint8_t* flags, const float* ndsm, const int* label, long N, long long* table, hipStream_t st);

// dsm_roofs.hip: link bits, segments, integer moments, growth rounds and residuals (include/adamvs_hip.h, "Roof planes")
long roof_workspace_bytes(int W, int H);
int launch_roof_links(int W, int H, const float* dsm, const int* building, int s, double smooth_tol, double g_tol, double step_tol,
                      uint8_t* link, hipStream_t st);
int launch_roof_label(int W, int H, const uint8_t* link, void* workspace, int* parent, adamvs_bld_stats* stats, hipStream_t st);
int launch_roof_moments(int W, int H, const float* dsm, const int* label, const int* building, double z_ref, long N, long long* table,
                        hipStream_t st);
int launch_roof_grow(int W, int H, const float* dsm, const int* building, double z_ref, long P, const double* planes, double assign_tol,
                     int round0, int rounds, int* label0, int* label1, unsigned* counts, hipStream_t st);
int launch_roof_residuals(int W, int H, const float* dsm, const int* label, double z_ref, long R, const double* planes, double assign_tol,
                          long long* table, hipStream_t st);

// dsm_lod2.hip: model labels, building table, transpose and the boundary runs (include/adamvs_hip.h, "LoD2 solids")
long lod2_workspace_bytes(int W, int H);
int launch_lod2_fill(int W, int H, const int* building, long P, int round0, int rounds, int* label0, int* label1, unsigned* counts,
                     hipStream_t st);
int launch_lod2_table(int W, int H, const float* dtm, const int* building, const int* label, double z_ref, long B, long P,
                      const long long* planes, long long* table, hipStream_t st);
int launch_lod2_transpose(int W, int H, const int* src, int* dst, hipStream_t st);
int launch_lod2_count(int W, int H, const int* label, const int* label_t, long P, void* workspace, unsigned* total, hipStream_t st);
int launch_lod2_runs(int W, int H, const int* label, const int* label_t, long P, const long long* planes, const int* plane_base, long N,
                     void* workspace, int* records, hipStream_t st);

// dsm_trees.hip: canopy surface, parents, roots, crown labels and the per-tree table (include/adamvs_hip.h, "Trees")
long tree_workspace_bytes(int W, int H);
int launch_tree_surface(int W, int H, const float* ndsm, const int* building, double min_height, int smooth_passes, void* workspace,
                        uint8_t* mask, int* q, int* s, int* s_max, hipStream_t st);
int launch_tree_parents(int W, int H, const int* s, int r_cap, const int* thr, void* workspace, int* parent, adamvs_tree_stats* stats,
                        hipStream_t st);
int launch_tree_roots(int W, int H, const int* parent, void* workspace, int* root, adamvs_tree_stats* stats, hipStream_t st);
int launch_tree_crowns(int W, int H, const int* s, const int* root, const int* number, int ratio_pm, long rc2, int* label,
                       long long* unassigned, hipStream_t st);
int launch_tree_table(int W, int H, const int* label, const int* q, const int* s, const int* root, long T, long long* table, hipStream_t st);

// dsm_contours.hip: integer surface, segments with their links, list ranking, line table and vertices (include/adamvs_hip.h, "Contours")
long contour_workspace_bytes(int W, int H);
long contour_rank_workspace_bytes(long N);
int launch_contour_surface(int W, int H, const float* z, double z_ref, int smooth_passes, void* workspace, int* s, int* info, hipStream_t st);
int launch_contour_count(int W, int H, const int* s, int K, const int* lev, void* workspace, int* count, adamvs_contour_stats* stats,
                         hipStream_t st);
int launch_contour_segments(int W, int H, const int* s, int K, const int* lev, long N, void* workspace, int* seg_entry, int* seg_exit,
                            int* seg_level, int* succ, int* pred, hipStream_t st);
int launch_contour_rank(long N, const int* pred, void* workspace, int* start, int* rank, uint8_t* closed, adamvs_contour_stats* stats,
                        hipStream_t st);
int launch_contour_lines(int W, int H, const int* s, int K, const int* lev, long N, long M, const int* seg_entry, const int* seg_exit,
                         const int* seg_level, const int* succ, const int* start, const int* rank, const uint8_t* closed, void* workspace,
                         long long* line_first, int* line_start, int* line_level, uint8_t* line_closed, long long* vertex, hipStream_t st);

// dsm_drainage.hip: fill, D8 directions, accumulation with roots, stream links (include/adamvs_hip.h, "Drainage")
long drain_workspace_bytes(int W, int H);
int launch_drain_fill(int W, int H, const int* s, int smooth_passes, int max_rounds, void* workspace, int* r, int* F, adamvs_drain_stats* stats,
                      hipStream_t st);
int launch_drain_direction(int W, int H, const int* F, uint8_t* dir, hipStream_t st);
int launch_drain_accumulate(int W, int H, const uint8_t* dir, const int* value, void* workspace, int* acc, int* root, adamvs_drain_stats* stats,
                            hipStream_t st);
int launch_drain_streams(int W, int H, const uint8_t* dir, const int* acc, int min_cells, void* workspace, uint8_t* nd, int* link, int* pos,
                         adamvs_drain_stats* stats, hipStream_t st);
int launch_drain_links(int W, int H, const uint8_t* dir, const uint8_t* nd, const int* link, const int* pos, long L, long P, void* workspace,
                       int* link_first, int* link_head, int* link_end, int* link_to, int* vertex, hipStream_t st);

// dsm_solar.hip: horizon, sky-view factor, exposure, plane sums (include/adamvs_hip.h, "Solar")
long solar_workspace_bytes(int W, int H, int K);
int launch_solar_horizon(int W, int H, int K, const int* s, void* workspace, int* hz_n, int* hz_h, adamvs_solar_stats* stats, hipStream_t st);
int launch_solar_svf(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, const double* weight, double q, double* svf,
                     hipStream_t st);
int launch_solar_expose(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, int T, const int* sector, const double* thr,
                        const int* minutes_w, const int* energy_w, const int* sun, const int* label, long P, const int* normal, void* workspace,
                        int* minutes, int* direct, hipStream_t st);
int launch_solar_plane_sums(int W, int H, const int* s, const int* label, long P, const int* minutes, const int* direct, long long* table,
                            hipStream_t st);

// mesh.hip: TSDF integration and marching-tetrahedra extraction per brick (include/adamvs_hip.h, "TSDF mesh")
constexpr int MESH_TILE = ADAMVS_MESH_TILE;
int launch_tsdf_integrate(const adamvs_mesh_brick& b, const adamvs_mesh_view* views, int nviews, const int* list, int nlist, float* tsdf,
                          uint16_t* weight, unsigned* rgba, hipStream_t st);
int launch_mesh_classify(const adamvs_mesh_brick& b, const float* tsdf, const uint16_t* weight, unsigned* cube_code, unsigned* block_tris,
                         hipStream_t st);
int launch_mesh_count_vertices(const adamvs_mesh_brick& b, const float* tsdf, const unsigned* cube_code, uint8_t* edge_mask,
                               unsigned* block_verts, hipStream_t st);
int launch_mesh_emit(const adamvs_mesh_brick& b, const float* tsdf, const unsigned* rgba, const unsigned* cube_code, const uint8_t* edge_mask,
                     const unsigned* vert_offsets, const unsigned* tri_offsets, unsigned vertex_base, double* xyz, uint8_t* rgb,
                     unsigned* first_vertex, long vert_capacity, unsigned* faces, long tri_capacity, hipStream_t st);

// mesh_simplify.hip: vertex clustering with one quadric per lattice cell (include/adamvs_hip.h, "Mesh simplification")
constexpr int SIMPLIFY_TILE = ADAMVS_SIMPLIFY_TILE;
int launch_simplify_keys(const double* origin, double cell, const double* xyz, long nv, long long* keys, uint8_t* bad, hipStream_t st);
int launch_simplify_corners(const unsigned* faces, long nf, const int* vcell, long nv, int nc, int* fcell, int* entry_cell, uint8_t* survive,
                            hipStream_t st);
int launch_simplify_accumulate(const double* origin, double cell, const long long* keys, int nc, const double* xyz, const uint8_t* rgb,
                               long nv, const unsigned* faces, long nf, const long long* entry, const long long* fstart,
                               const long long* vorder, const long long* vstart, double* quadric, double* member,
                               unsigned long long* colour, hipStream_t st);
int launch_simplify_solve(const double* origin, double cell, double rank_eps, const long long* keys, int nc, const double* quadric,
                          const double* member, const unsigned long long* colour, const long long* vstart, double* pos, uint8_t* col,
                          uint8_t* rank, uint8_t* fallback, double* error, hipStream_t st);
void simplify_solve_host(const double* quadric, const double* mean, double cell, double rank_eps, double* p, int* rank, int* fallback,
                         double* error);
int launch_simplify_triples(const int* fcell, long nf, const long long* surv, long ns, int* tri, hipStream_t st);
int launch_simplify_first(const int* tri, const long long* surv, const long long* order, long ns, long nf, uint8_t* keep, hipStream_t st);
int launch_simplify_mark(const int* fcell, const uint8_t* keep, long nf, int nc, uint8_t* used, hipStream_t st);
int launch_simplify_count(const uint8_t* flags, long n, unsigned* block_count, hipStream_t st);
int launch_simplify_emit(const double* pos, const uint8_t* col, const uint8_t* used, int nc, const unsigned* cell_offsets, const int* fcell,
                         const uint8_t* keep, long nf, const unsigned* face_offsets, double* xyz, uint8_t* rgb, unsigned* new_index,
                         long vert_capacity, unsigned* faces, long face_capacity, hipStream_t st);

// mesh_smooth.hip: bilateral normal filtering of the mesh (include/adamvs_hip.h, "Mesh smoothing")
constexpr int SMOOTH_TILE = ADAMVS_SMOOTH_TILE;
int launch_smooth_faces(const double* p, long nv, const unsigned* faces, long nf, double* rec, hipStream_t st);
// the 3 nf edge keys of a mesh, for smoothing, cleaning and texturing alike; `what` names the entry point in a launch error
int launch_mesh_edge_keys(const unsigned* faces, long nf, long long* keys, const char* what, hipStream_t st);
int launch_smooth_boundary(const long long* keys, long n, long nv, uint8_t* fixed, hipStream_t st);
int launch_smooth_filter(const double* rec, const double* nin, double* nout, const unsigned* faces, long nf, long nv, const int* vface,
                         const long long* vstart, double sigma_s, double sigma_r, hipStream_t st);
int launch_smooth_centroids(const double* p, long nv, const unsigned* faces, long nf, double* cen, hipStream_t st);
int launch_smooth_update(const double* p0, const double* p, double* pout, long nv, const double* nrm, const double* cen, long nf,
                         const int* vface, const long long* vstart, const uint8_t* fixed, double cap, uint8_t* clamped, hipStream_t st);

// mesh_clean.hip: small components dropped, small holes closed (include/adamvs_hip.h, "Mesh cleaning")
constexpr int CLEAN_TILE = ADAMVS_CLEAN_TILE;
constexpr int CLEAN_CHUNK = ADAMVS_CLEAN_CHUNK;
int launch_clean_components(const unsigned* faces, long nf, long nv, const int* parent_in, int* parent_out, unsigned* changed, hipStream_t st);
int launch_clean_area(const double* area, long nf, const long long* order, const long long* seg_of, const long long* seg_start, long ncomp,
                      double* lead, double* first, double* out, hipStream_t st);
int launch_clean_boundary(const long long* keys, const long long* entry, long n, uint8_t* bnd, hipStream_t st);
int launch_clean_successor(const unsigned* faces, long ns, long nv, const uint8_t* bnd, int* out_cnt, int* in_cnt, int* out_he, int* succ,
                           int* lab, int* nxt, uint8_t* broken, hipStream_t st);
int launch_clean_double(const uint8_t* bnd, long n, const int* lab_in, const int* nxt_in, const uint8_t* broken_in, int* lab_out, int* nxt_out,
                        uint8_t* broken_out, hipStream_t st);
int launch_clean_validate(const uint8_t* bnd, const int* succ, const int* lab, const uint8_t* broken, long n, int M, int* cnt, uint8_t* bad,
                          int* loop, uint8_t* closed, hipStream_t st);
int launch_clean_accumulate(const double* p, const uint8_t* rgb, long nv, const unsigned* faces, long ns, const int* members,
                            const long long* start, long nl, long nm, const double* origin, double* centre, uint8_t* colour, hipStream_t st);
int launch_clean_emit(const double* xyz, const uint8_t* rgb, long nv, const int* new_index, const unsigned* faces, long ns, const int* fill_h,
                      const int* loop_of, long nfill, const double* centre, const uint8_t* colour, long nl, long nvs, double* xyz_out,
                      uint8_t* rgb_out, unsigned* faces_out, hipStream_t st);

// cloud_dist.hip: bounded nearest neighbour between two clouds and the surface sampler (include/adamvs_hip.h, "Cloud distance")
constexpr int CLOUD_TILE = ADAMVS_CLOUD_TILE;
int launch_cloud_nearest(const double* origin, double D, const long long* ukeys, const long long* tstart, int nc, const double* targets,
                         const int* tindex, long nt, const double* queries, long nq, const long long* qorder, long nqs,
                         const long long* item_key, const long long* item_first, const int* item_count, long ni, float* d2, int* index,
                         unsigned long long* pairs, hipStream_t st);
int cloud_nearest_host(const double* origin, double D, const double* targets, long nt, const double* queries, long nq, float* d2, int* index,
                       unsigned long long* pairs);
int launch_cloud_sample_count(const double* xyz, long nv, const unsigned* faces, long nf, double spacing, int* subdiv, hipStream_t st);
int launch_cloud_sample_emit(const double* xyz, long nv, const unsigned* faces, long nf, const int* subdiv, const long long* offsets,
                             double* points, long capacity, hipStream_t st);

// cloud_knn.hip: the k nearest neighbours of every point of a cloud and a normal from them (include/adamvs_hip.h, "Cloud neighbourhoods")
constexpr int KNN_MAX_K = ADAMVS_KNN_MAX_K;
int launch_knn_search(const double* origin, double R, int k, const long long* ukeys, const long long* tstart, int nc, const double* sorted,
                      const int* pindex, long n, const long long* item_key, const long long* item_first, const int* item_count, long ni,
                      long long row_base, long rows, float* d2, int* index, int* count, unsigned long long* pairs, hipStream_t st);
int knn_search_host(const double* origin, double R, int k, const double* points, long n, float* d2, int* index, int* count,
                    unsigned long long* pairs);
int launch_knn_normals(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                       double* normal, float* curvature, uint8_t* flag, hipStream_t st);
int knn_normals_host(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point, double* normal,
                     float* curvature, unsigned char* flag);

// cloud_register.hip: the rigid motion of a cloud and the sums of point-to-plane ICP (include/adamvs_hip.h, "Cloud registration")
constexpr int ICP_TERMS = ADAMVS_ICP_TERMS;
int launch_rigid_apply(const double* R, const double* c, const double* u, const double* x, long n, double* y, hipStream_t st);
int rigid_apply_host(const double* R, const double* c, const double* u, const double* x, long n, double* y);
int launch_icp_accumulate(const double* y, const int* index, long nq, const double* targets, const double* normals, const unsigned char* flag,
                          long nt, const double* c, double L, double delta, double* partial, hipStream_t st);
int icp_accumulate_host(const double* y, const int* index, long nq, const double* targets, const double* normals, const unsigned char* flag,
                        long nt, const double* c, double L, double delta, double* partial);
int launch_icp_reduce(const double* partial, long nb, double* sums, hipStream_t st);
int icp_reduce_host(const double* partial, long nb, double* sums);

// ortho.hip: image orthophoto over a DSM, z-buffered per view (include/adamvs_hip.h, "Image orthophoto")
constexpr int ORTHO_TILE = ADAMVS_ORTHO_TILE;
constexpr int ORTHO_SMALL_PX = ADAMVS_ORTHO_SMALL_PX;
constexpr float ORTHO_NEAR = ADAMVS_ORTHO_NEAR;
int launch_ortho_surface(const adamvs_ortho_grid& g, const float* dsm, double* height, hipStream_t st);
int launch_ortho_zbuf(const adamvs_ortho_grid& g, const float* dsm, const adamvs_ortho_view& v, unsigned* zbuf, unsigned* big_count,
                      unsigned* big_list, hipStream_t st);
int launch_ortho_compose(const adamvs_ortho_grid& g, const adamvs_ortho_view& v, int view_id, const double* height, const unsigned* zbuf,
                         int mode, float border, float feather_px, float tol, float* acc, float* wmax, int* view, int* nvis, hipStream_t st);
int launch_ortho_finalize(const adamvs_ortho_grid& g, const float* acc, const int* view, const int* nvis, uint8_t* rgba, int* view_out,
                          uint16_t* nvis_out, hipStream_t st);

// ortho_balance.hip: per-view gains for the mosaic (include/adamvs_hip.h, "Image orthophoto: radiometric balance";
// ortho_sample.h holds the visibility test and bilinear sample it shares with ortho.hip)
constexpr int ORTHO_BAL_CHUNK = ADAMVS_ORTHO_BAL_CHUNK;
int launch_ortho_observe(const adamvs_ortho_grid& g, const float* dsm, const adamvs_ortho_view& v, const unsigned* zbuf, int S, float border,
                         float tol, uint16_t* obs, hipStream_t st);
int launch_ortho_pair_stats(const uint16_t* obs, long Ns, const int* pairs, int P, int max_diff_q, long long* stats, hipStream_t st);
int launch_ortho_adjust_image(const uint8_t* rgba_in, long npx, const float* gain, uint8_t* rgba_out, hipStream_t st);
int launch_ortho_seam_stats(const adamvs_ortho_grid& g, const int* view_out, const uint8_t* rgba, long long* stats, hipStream_t st);

// texture.hip: mesh texture from the source views (include/adamvs_hip.h, "Mesh texturing"; raster.h holds the rasteriser it
// shares with ortho.hip)
constexpr int TEX_TILE = ADAMVS_TEXTURE_TILE;
int launch_tex_project(const adamvs_ortho_view& v, const double* xyz, long nv, float* uvz, hipStream_t st);
int launch_tex_zbuf(int W, int H, const float* uvz, long nv, const unsigned* faces, long nf, unsigned* zbuf, unsigned* big_count,
                    unsigned* big_list, hipStream_t st);
int launch_tex_score(int W, int H, int view, const float* uvz, long nv, const unsigned* faces, long nf, const unsigned* zbuf, float border,
                     float tol, float* best, int* label, int* nvis, float* uv, hipStream_t st);
int launch_tex_components_round(const long long* keys, const long long* entry, long n, const int* label, int* parent, long nf,
                                unsigned* changed, hipStream_t st);
int launch_tex_rank(const int* label, const int* parent, long nf, unsigned* block_roots, unsigned* block_untex, unsigned* root_off,
                    unsigned* untex_off, int* root_chart, int* pal, hipStream_t st);
int launch_tex_boxes(const int* label, const int* parent, const int* root_chart, const float* uv, long nf, int* chart, int* box,
                     hipStream_t st);
int launch_tex_fill(const adamvs_ortho_view& v, const int* items, const long long* prefix, int n, long texels, int P, long pages,
                    unsigned char* atlas, hipStream_t st);
int launch_tex_coords(const int* label, const int* chart, const int* pal, const float* uv, long nf, const int* charts, int pal_ox,
                      int pal_oy, int pal_page, int P, long pages, const unsigned* faces, long nv, const unsigned char* vrgb,
                      unsigned char* atlas, float* tc, int* texnum, hipStream_t st);

// texture_level.hip: global seam levelling of the textured mesh (include/adamvs_hip.h, "Mesh texturing", seam levelling)
constexpr int TEX_LEVEL_BLOCKS = ADAMVS_TEXTURE_LEVEL_BLOCKS;
int launch_lvl_observe(const long long* view_tab, int nviews, const int* rowptr, const unsigned* col, long nnz, const int* node_view,
                       const float* pos, long n, float* f, hipStream_t st);
int launch_lvl_rhs(const int* rowptr, const unsigned* col, long nnz, const float* f, long n, double* b, hipStream_t st);
int launch_lvl_cg_init(const double* b, long n, double tol, double* g, double* r, double* p, double* partials, double* state,
                       hipStream_t st);
int launch_lvl_cg(const int* rowptr, const unsigned* col, long nnz, long n, double lambda, int count, double* g, double* r, double* p,
                  double* ap, double* partials, double* state, hipStream_t st);
int launch_lvl_owner(const float* uv, const int* chart, long nf, const int* charts, const long long* prefix, int nc, long texels,
                     int* owner, unsigned* big_count, unsigned* big_list, hipStream_t st);
int launch_lvl_dilate(const int* charts, const long long* prefix, int nc, long texels, const int* in, int* out, hipStream_t st);
int launch_lvl_apply(const float* uv, const int* corner_node, long nf, const double* g, long n, const int* charts,
                     const long long* prefix, int nc, long texels, const int* owner, int P, long pages, unsigned char* atlas,
                     hipStream_t st);

}  // namespace adamvs
