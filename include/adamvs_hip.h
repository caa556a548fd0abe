/* libadamvs_hip.so -- C ABI of the MI355X (gfx950) Ada-MVS depth-inference hot path.
 *
 * The reference (gpcv-liujin/Ada-MVS) is pure PyTorch and has no native seam;
 * this header IS the seam a maintainer binds (ctypes stub: INTEGRATION.md).
 * Each entry point names the reference code it replaces (paths relative to the
 * reference repository root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless stated otherwise;
 *     the caller (PyTorch) owns all memory, including the workspace; nothing
 *     is allocated, freed or retained by the library;
 *   - all work is enqueued on `stream` (a hipStream_t); no call synchronises,
 *     so every call can be captured into a hipGraph;
 *   - return 0 on success, <0 for an argument/shape error, >0 a hipError_t;
 *     adamvs_last_error_string() describes the last failure on this thread;
 *   - re-entrant; the only global state is the thread-local error string and the option table below (process-wide
 *     integers that select between equivalent kernel forms; read on every call, written only by adamvs_set_option).
 *
 * Layouts ("channel-last"): feature maps [view][B][h*w][C], GRU states
 * [B][h*w][ch], cost-regularisation activations [N][h*w][D]; hypothesis planes
 * and output maps are [B][D][h*w] / [B][h*w] as in the reference.
 */
#ifndef ADAMVS_HIP_H
#define ADAMVS_HIP_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADAMVS_ABI_VERSION 22

int adamvs_version(void);
const char* adamvs_last_error_string(void);

/* ---- OPTIONS ---------------------------------------------------------------
 * Integers that choose between kernel forms of the SAME layer (every form is held to the same oracle; forms differ in the
 * order of their fp32 sums at most) and a few tuning limits.  adamvs_set_option takes effect at the next call of any entry
 * point, for every caller of the process (two callers that need different forms set the option before their calls; the
 * table is atomic integers, not locked state).  When the table is first touched each option is seeded from the environment
 * variable ADAMVS_<NAME IN CAPITALS> if that is set (A/B timing of an unmodified caller); nothing else in the compute path
 * reads the environment (two tuning tables of the recurrence's grid split: ADAMVS_RECUR_COSTS, ADAMVS_RECUR_COSTS_FUSED).
 *
 *   name                  default  meaning
 *   winograd                 1     CostRegNet2D (models/adamvs.py:229-238), fp32, widths that are multiples of 64: the five stride-1
 *                                  layers in the minimal-filtering form F(2x2, 3x3) (16 of 36 products); 0: direct kernels.
 *                                  On wide maps conv0 and prob take the mixed form F(2x4, 3x3) (24 products where F(2x2, 3x3) has
 *                                  32; D >= 128, maps at least 128 pixels wide of which 64-pixel blocks waste at most an eighth); + 2
 *                                  (value 3): F(2x2, 3x3) in every stride-1 layer, the maps of before bit for bit; + 4 (value 5): no
 *                                  folded blocks in any layer ("Folded blocks" below: conv2 / conv4 stay in F(2x2, 3x3), conv3 / conv5
 *                                  on the direct kernel), the maps of before those bit for bit -- the run-time A/B of the whole pipeline
 *   wino_softmax             1     ... its `prob` layer carries the softmax partials, no score volume (stage path); 0: score volume
 *   wino_wps                 0     ... 1 / 2: one / two workgroups per CU for every map size (same bits); 0: by map size
 *   fuse_softmax             1     direct `prob` kernel: softmax / max / depth regression in its epilogue; 0: k_softmax_regress
 *   s2_pairs                 1     CostRegNet2D: large stride-2 and transposed layers in the pair forms along x (15 of 18 products); 0: direct
 *   conv_rows2              -1     CostRegNet2D: 2-row blocks for small grids: 0 never, 1 always, -1 by grid size
 *   t2_fused                -1     transposed layers, the four parity classes in one launch: 0 / 1 / -1 by grid size
 *   t2_kb8                   1     transposed layers at D = 192: two k-steps per chunk; 0: one
 *   costreg_defer_skips      1     the hourglass's skip additions formed by the consuming layer; 0: in the producer's epilogue
 *   conv256_split            1     D = 256 direct layers as two launches of 128 output channels; 0: one
 *   conv_small_grid       1024     MS-REDNet (models/msrednet.py): workgroups up to which a layer takes the resident form; 0: never
 *   red_fold_applies        -1     MS-REDNet: the GRU's element-wise applies folded into the next layer's prologue: 0 / 1 / -1 by batch
 *   conv1_f23                3     conv1 of SliceCostRegNetRED (adamvs.py:417) in the F(2, 3)-along-x form: bit 1 C = 32, bit 2 C = 16 / 8
 *   fconv_f23                1     FeatureNet0's stride-1 3x3 layers in the F(2, 3)-along-x form; 0: k_fconv
 *   gru_wino                 7     fp32 ConvGRU convolutions (module.py:24-52) in the F(2x2, 3x3) form where a role has a launch of
 *                                  its own and in the three-launch schedule: 1 gates1, 2 gates2, 4 cand2, 8 cand1; 0: direct kernels
 *                                  (the software-pipelined schedules 3 and 5 always use the direct / fused roles).
 *                                  Two more bits, both CLEAR by default, give back the launches of before: + 16 conv2 (adamvs.py:418)
 *                                  in a launch of its own (clear: with bit 1, on even maps, conv2 of hypothesis t - 1 runs inside the
 *                                  gate launch of level 1 of hypothesis t, whose tile window holds its inputs; level 2 and the
 *                                  decoder then run one hypothesis behind level 1 and schedule 0 has five launches per hypothesis);
 *                                  + 32 cand1 with a launch of its own on 8 x 16 tiles (clear: 8 x 32).  And one that is clear by
 *                                  default and switches a form ON: + 64 slot A of the three-launch schedule (recur_mode 1) is the
 *                                  level-1 gate role with conv2 inside instead of gates1 | conv2.  Same maps bit for bit.
 *   recur_mode              -1     launches per hypothesis of the recurrence: 0 one role per launch (six, or five: gru_wino; bf16x3:
 *                                  four), 1 three, 3 two, 5 one (both levels one kernel each); -1: by stage size
 *                                  (adamvs_recurrence_schedule)
 */
int adamvs_option_count(void);
const char* adamvs_option_name(int index);                   /* 0 <= index < adamvs_option_count(); NULL outside */
int adamvs_option_default(const char* name, int* value);     /* -1: unknown name */
int adamvs_get_option(const char* name, int* value);
int adamvs_set_option(const char* name, int value);

/* ---- geometry ----------------------------------------------------------- */

/* T = P_src . P_ref^-1 for every (batch, source view); models/module.py:539-541.
 * proj [B][V][4][4] (view 0 = reference) -> rt [B][V-1][12] = {R row-major, t}. */
int adamvs_relative_transforms(const float* proj, float* rt, int B, int V, void* stream);

/* NCHW [B][C][h][w] -> channel-last [B][h*w][C] (one view slot) and back. C % 4 == 0. */
int adamvs_pack_features(const float* nchw, float* nhwc, int B, int C, int h, int w, void* stream);
int adamvs_unpack_features(const float* nhwc, float* nchw, int B, int C, int h, int w, void* stream);

/* get_depth_range_samples, models/module.py:646-663: depth_values [B][2]={min,max}
 * -> out [B][D][h][w], D uniform samples (the interval argument is ignored there). */
int adamvs_depth_range_samples_uniform(const float* depth_values, float* out, int B, int D, int h, int w, void* stream);
/* get_cur_depth_range_samples, models/module.py:628-643: window cur -+ D/2*interval,
 * D samples, no clamping.  cur_depth [B][h][w] -> out [B][D][h][w].  The interval is a double: the reference forms
 * ndepth / 2 * depth_inteval_pixel in Python floats and only the product is rounded to fp32 (module.py:632). */
int adamvs_depth_range_samples_window(const float* cur_depth, double depth_interval_pixel, float* out, int B, int D,
                                      int h, int w, void* stream);

/* F.interpolate(x, [ho,wo], mode='bilinear', align_corners=False) on [N][hi][wi];
 * models/adamvs.py:505 (view weights) and :522 (hypothesis plane). */
int adamvs_resize_bilinear(const float* in, float* out, int N, int hi, int wi, int ho, int wo, void* stream);

/* depth_regression, models/module.py:617-625: prob [B][D][h][w]; depth_values
 * [B][D] (hd = wd = 0) or [B][D][hd][wd] (bilinearly resized to [h][w]) -> out [B][h][w]. */
int adamvs_depth_regression(const float* prob, const float* depth_values, float* out, int B, int D, int h, int w,
                            int hd, int wd, void* stream);

/* homo_warping_float, models/module.py:527-568, on the reference's own layouts:
 * src_fea [B][C][h][w], rt [B][12] (adamvs_relative_transforms of this view),
 * depth_values [B][Nd][h][w] -> out [B][C][Nd][h][w]. */
int adamvs_homo_warp(const float* src_fea, const float* rt, const float* depth_values, float* out, int B, int C,
                     int Nd, int h, int w, void* stream);

/* ---- stage 1, per-view weighting (InferDepthNet0.forward pass A) --------- */

/* models/adamvs.py:464-478: sim[s][b][pix][d] = mean_c(ref[c] * warp_d(src_s)[c]).
 * feat [V][B][h*w][C], rt [B][S][12], planes [B][D][h*w] -> sim [S][B][h*w][D]. C in {8,16,32}. */
int adamvs_pair_similarity(const float* feat, const float* rt, const float* planes, float* sim, int B, int S, int C,
                           int D, int h, int w, void* stream);

/* CostRegNet2D.forward, models/adamvs.py:229-238, on x [N][h*w][D] -> score [N][h*w][D].
 * wpk: 11 layers (conv0..conv6, conv7, conv9, conv11, prob), each 9*D*D floats in
 * A-fragment order [tap][cin/4][cout/16][lane] with value
 * W[cout = 16*tile + (lane&15)][cin = 4*kc + (lane>>4)][tap] * bn_scale[cout]
 * (ConvTranspose2d layers: W[cin][cout][tap]) followed by D bias floats (folded BN shift,
 * or the conv bias for `prob`).  D in {16,32,48,64,96,128,192,256,384,512}; h, w multiples of 8.
 *
 * The reference builds the network for any number of hypotheses (adamvs.py:198-228); here a network of D hypotheses runs at
 * the next width of that list, adamvs_cost_reg_width(D, precision), with zero filters for the extra channels and -1e30 as
 * the bias of `prob`'s extra channels (ada-mvs_amd/packing.py::pack_cost_reg_net_2d): the extra channels stay 0 through the
 * hourglass and weigh exactly 0 in the softmax.  The op-level entry points below take the WIDTH as D (x and score carry
 * that many channels); adamvs_depth_stage_forward takes the number of hypotheses and handles the rest.
 *
 * fp32 with D in {64,128,192,256,384,512}: the 11 blocks are followed by the five stride-1 layers (conv0, conv2, conv4, conv6, prob)
 * in the minimal-filtering form F(2x2, 3x3), 16*D*D floats each, laid out as adamvs_conv3x3_dd_wino takes them; those
 * layers run on that kernel (fp32 throughout, 16 products instead of 36 per 2x2 outputs and channel pair; environment
 * ADAMVS_WINOGRAD=0: on the direct kernel).  ada-mvs_amd/packing.py::pack_cost_reg_net_2d produces exactly this.
 * fp32 with D in {128,192,256,384,512}: behind those 11 + 5 blocks, at unchanged offsets, two more: conv0 and prob in the form
 * F(2x4, 3x3), 24*D*D floats each, laid out as adamvs_conv3x3_dd_wino24 takes them (the two layers that run on the full-size
 * map; option winograd says when they take that kernel).  The blob at D = 64, where that form never wins, is unchanged.
 * fp32 with D in {192,256,384,512}: behind those, again at unchanged offsets, conv2 and conv4 in the same form and layout (the inner
 * levels' stride-1 layers; adamvs_cost_reg_fold says when they take that kernel).  The blobs at D = 64 and 128 are unchanged.
 * wpk_floats = the length of the blob, adamvs_cost_reg_net_2d_weight_floats(D, precision): a blob of another layout
 * (e.g. the 11-block blob of ABI <= 10 at a width that now carries the F(2x2, 3x3) blocks) is refused, not read past its end.
 *
 * precision ADAMVS_PRECISION_FP32 (0): fp32 MFMA.  ADAMVS_PRECISION_BF16X3 (1): bf16 MFMA with every
 * operand split into two bf16 halves, a.b ~ a_hi.b_hi + a_hi.b_lo + a_lo.b_hi, fp32 accumulation (maps agree
 * with the fp32 path to ~1e-5); D must then be a multiple of 32 and each layer's 9*D*D-float block of wpk holds
 * bf16 fragments instead: [hi|lo][tap][cin/32][cout/16][lane][8] with element j of lane l =
 * W[cout = 16*tile + (l&15)][cin = 32*kb + 8*(l>>4) + j][tap] * bn_scale[cout] (same total size). */
#define ADAMVS_PRECISION_FP32 0
#define ADAMVS_PRECISION_BF16X3 1
size_t adamvs_cost_reg_net_2d_workspace_bytes(int N, int D, int h, int w);
int adamvs_cost_reg_width(int D, int precision);                       /* the width the network runs at for D hypotheses; 0: none (D > 512) */
size_t adamvs_cost_reg_net_2d_weight_floats(int D, int precision);     /* floats of wpk at width D; 0: not a supported width */
int adamvs_cost_reg_net_2d(const float* x, const float* wpk, size_t wpk_floats, float* score, int N, int D, int h, int w,
                           int precision, void* workspace, size_t workspace_bytes, void* stream);

/* One layer of CostRegNet2D: ConvBnReLU.forward (models/module.py:254-261) or the
 * ConvTranspose2d-BN-ReLU blocks of models/adamvs.py:212-225, BN folded into wpk/bias.
 * mode 0: 3x3 stride 1; 1: stride 2; 2: transposed stride 2 (k3 p1 op1).
 * in [N][hi*wi][D] -> out [N][ho*wo][D]; wpk as one layer above.  The hourglass's additions
 * (x = conv4 + conv7(x), adamvs.py:233-236) can sit on either side of a layer:
 *   skip [N][ho*wo][D] or NULL: added to this layer's output after the ReLU (producer side);
 *   in2  [N][hi*wi][D] or NULL: the layer convolves in + in2 (consumer side: the sum is formed while the
 *        window is staged, so a transposed layer's epilogue carries no second round of loads).
 * adamvs_cost_reg_net_2d uses in2 in fp32 and skip in bf16x3; the result is the same fp32 sum either way. */
int adamvs_conv3x3_dd(const float* in, const float* in2, const float* wpk, const float* bias, const float* skip, float* out,
                      int N, int D, int hi, int wi, int mode, int relu, int precision, void* stream);

/* A stride-1 layer of CostRegNet2D (conv0, conv2, conv4, conv6, prob: models/adamvs.py:205-227, ConvBnReLU.forward
 * models/module.py:254-261) in the minimal-filtering form F(2x2, 3x3): 16 products per 2x2 output tile and channel pair
 * instead of 36, fp32 throughout (results agree with adamvs_conv3x3_dd mode 0 to a few ulp of the accumulated sums).
 * wpk [D/4][4][D/16][64][4] = the transformed filters U = G w G^T (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1], BN scale folded
 * in) as MFMA A fragments: element j of lane l of fragment (k-step kc, patch row i, channel tile) =
 * U[i][j][cout = 16*tile + (l&15)][cin = 4*kc + (l>>4)].  D a multiple of 64 up to 512; a map at most 2 GiB.  in, out, skip,
 * bias, relu as above. */
int adamvs_conv3x3_dd_wino(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D,
                           int h, int w, int relu, void* stream);

/* The same layer in the mixed form F(2x4, 3x3): F(2, 3) down the rows as above, F(4, 3) along the columns (points 0, +-1, +-2,
 * infinity), 24 products per 2x4 output tile and channel pair where F(2x2, 3x3) needs 32; fp32 throughout, about twice the
 * rounding error of F(2x2, 3x3) (the column transform has the factors 4, 5, 8 and 1/24).
 * wpk = U = G w G4^T (G as above, G4 = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1], BN scale
 * folded in, formed in double precision and rounded once) as two arrays of A fragments, 24*D*D floats in all:
 * [D/4][4][D/16][64][4] with element j of lane l of fragment (k-step kc, patch row i, channel tile) =
 * U[i][j][cout = 16*tile + (l&15)][cin = 4*kc + (l>>4)] for the patch columns j = 0..3, then [D/4][4][D/16][64][2] for j = 4, 5.
 * Everything else as adamvs_conv3x3_dd_wino. */
int adamvs_conv3x3_dd_wino24(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D,
                             int h, int w, int relu, void* stream);

/* models/adamvs.py:481-486 + module.py:617-625: softmax over D, its maximum (view
 * weight) and the expectation of the hypothesis planes (pair depth).
 * score [S*B][h*w][D], planes [B][D][h*w] -> view_weight, pair_depth [S][B][h*w]. */
int adamvs_softmax_max_regress(const float* score, const float* planes, float* view_weight, float* pair_depth,
                               int S, int B, int D, int h, int w, void* stream);

/* The last layer of CostRegNet2D (`prob`, adamvs.py:227, 238) with the view weighting above fused into its epilogue, the
 * way adamvs_depth_stage_forward runs it: score = conv3x3(in) + bias is reduced over D by the workgroup that
 * computes it and never stored.  in [S*B][h*w][D]; wpk / bias: the `prob` block of the packed weights (9*D*D + D floats);
 * planes [B][D][h*w] -> view_weight, pair_depth [S][B][h*w].  precision as adamvs_cost_reg_net_2d (wpk packed accordingly). */
int adamvs_prob_softmax_regress(const float* in, const float* wpk, const float* bias, const float* planes,
                                float* view_weight, float* pair_depth, int S, int B, int D, int h, int w, int precision,
                                void* stream);

/* The same with `prob` in the form F(2x2, 3x3) (what the fp32 stage runs at D a multiple of 64): the channel groups of a pixel
 * are different workgroups, so every lane stores the softmax partial (max, sum of exp, sum of exp * plane) of the 16 scores it
 * holds -- D bytes per pixel instead of the 4 D of the scores -- and a second kernel merges a pixel's D/16 partials.
 * The hypothesis planes are those of stage 1, uniform per tile: depth_range [B][2] = (first, last) plane of tile b, plane d =
 * first + d * ((last - first) / (D - 1)) (get_depth_range_samples, module.py:628-640); with per-pixel planes the stage takes
 * the score volume and adamvs_softmax_max_regress.  wpk as adamvs_conv3x3_dd_wino; workspace:
 * adamvs_prob_softmax_regress_wino_workspace_bytes (S*B*h*w*D bytes). */
size_t adamvs_prob_softmax_regress_wino_workspace_bytes(int S, int B, int D, int h, int w);
int adamvs_prob_softmax_regress_wino(const float* in, const float* wpk, const float* bias, const float* depth_range, float* view_weight,
                                     float* pair_depth, int S, int B, int D, int h, int w, void* workspace, size_t workspace_bytes,
                                     void* stream);
/* ... and with `prob` in the form F(2x4, 3x3): wpk as adamvs_conv3x3_dd_wino24, the same partials, merge kernel and workspace. */
int adamvs_prob_softmax_regress_wino24(const float* in, const float* wpk, const float* bias, const float* depth_range, float* view_weight,
                                       float* pair_depth, int S, int B, int D, int h, int w, void* workspace, size_t workspace_bytes,
                                       void* stream);

/* ---- aggregation + recurrent regularisation (pass B) --------------------- */

/* SliceCostRegNetRED weights (models/adamvs.py:400-413), packed by the host:
 * conv weights as MFMA A fragments [cout tile][tap][cin/4][64 lanes] holding
 * W[cout = 16*tile + (lane&15)][cin = 4*kc + (lane>>4)][tap] (0 beyond cout),
 * biases zero-padded to 16 per tile.  conv1 and cand1 (8 output channels each) use the two-row form: fragment
 * (rr, kx, kc), rr = 0..3, holds for lanes with (lane&15) < 8 the weights of output row y,
 * W[lane&15][cin][ky = rr][kx] (0 if rr = 3), and for the other lanes those of output row y+1,
 * W[(lane&15)-8][cin][ky = rr-1][kx] (0 if rr = 0), so one MFMA feeds two output rows.
 *
 * With precision ADAMVS_PRECISION_BF16X3 the conv1 / gates / cand / conv2 fields point to split-bf16 fragments
 * instead: the contraction index is flattened, k = pos*cin_total + cin (pos = tap ky*3+kx, or rr*3+kx for the
 * two-row conv1 and -- since ABI 15 -- the two-row cand1: 12 positions x 16 channels = 6 k-blocks, rows as in the fp32 two-row
 * form above), zero-padded to a multiple of 32; layout [cout tile][hi|lo][k/32][lane][8 bf16], element j of
 * lane l = W[16*tile + (l&15)][k = 32*kb + 8*(l>>4) + j].  upconv1 / final_w / the biases keep the fp32 form.
 *
 * PRE-SCALED FIELDS (since ABI 13; nothing in the struct's size or layout shows it, so a caller that packs its own blob must
 * do this or gets silently wrong GRU states).  The kernels that consume these fields feed the convolution's accumulator to
 * v_exp_f32 (2^x) directly -- sigmoid(x) = 1 / (1 + 2^(-x log2 e)), tanh(x) = 1 - 2 / (2^(2 x log2 e) + 1) -- so the factor is
 * folded into weights AND bias by the host, in double precision, before the fragments are formed (rounded once):
 *   ADAMVS_PRECISION_BF16X3:  gates1, gates1_b, gates2, gates2_b  = (-log2 e) x the reference tensors;
 *                             cand1, cand1_b, cand2, cand2_b       = (2 log2 e) x the reference tensors;
 *                             and the 16 output rows of gates1 / gates1_b are INTERLEAVED so that every lane of the fused
 *                             level-1 kernel holds two reset- and two update-gate values: MFMA row m = 4 q + e carries
 *                             reset-gate channel 2 q + e for e = 0, 1 and update-gate channel 2 q + e - 2 for e = 2, 3
 *                             (q = 0..3), i.e. rows = conv_gates rows [0, 1, 8, 9, 2, 3, 10, 11, 4, 5, 12, 13, 6, 7, 14, 15]
 *                             (conv_gates rows 0-7 = reset gate, 8-15 = update gate, module.py:35-41).
 *                             gates2 keeps the reference's row order.  conv1, conv2: unscaled.
 *   ADAMVS_PRECISION_FP32:    gates1 / gates2 / cand1 / cand2 and their biases are the UNSCALED reference tensors (the direct
 *                             kernels apply exp themselves); the *_w fields below are U = G (s g) G^T with s = -log2 e for
 *                             gates1_w, gates2_w and s = 2 log2 e for cand1_w, cand2_w, reference row order; the kernels that
 *                             read a *_w field scale the shared, unscaled bias by the same s once per launch.
 * ada-mvs_amd/packing.py::pack_slice_reg_net is the reference implementation of this format
 * (tests/test_host_logic.py::test_gru_prescaled_fields_follow_the_header recomputes it from this text). */
typedef struct adamvs_fuse_weights {
  const float* conv1;                           /* [12][C/4][64] two-row form reg_fuse.conv1.conv.weight */
  const float* gates1; const float* gates1_b;   /* [1][9][4][64], [16]      conv_gru1.conv_gates.0 */
  const float* cand1;  const float* cand1_b;    /* [12][4][64] two-row form like conv1 (fp32), [16]   conv_gru1.convc.0 */
  const float* conv2;                           /* [1][9][2][64]            conv2.conv.weight */
  const float* gates2; const float* gates2_b;   /* [2][9][8][64], [32]      conv_gru2.conv_gates.0 */
  const float* cand2;  const float* cand2_b;    /* [1][9][8][64], [16]      conv_gru2.convc.0 */
  const float* upconv1; const float* upconv1_b; /* [1][9][4][64], [16]      upconv1 (transposed: W[cin][cout][tap]) */
  const float* final_w;                         /* [73]: w[tap*8+c], bias   upconv2d */
  /* fp32 (NULL in bf16x3): the same gate / candidate convolutions as transformed filters U = G (s g) G^T of the minimal-filtering
   * form F(2x2, 3x3) (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]; s = -log2 e for the gates, 2 log2 e for the candidates: "PRE-SCALED
   * FIELDS" above), fragments [cout tile][patch row i][patch column j][cin/4][64]:
   * lane l = U[i][j][cout = 16*tile + (l&15)][cin = 4*kc + (l>>4)] */
  const float* gates1_w;                        /* [1][4][4][4][64]         conv_gru1.conv_gates.0 */
  const float* gates2_w;                        /* [2][4][4][8][64]         conv_gru2.conv_gates.0 */
  const float* cand2_w;                         /* [1][4][4][8][64]         conv_gru2.convc.0 */
  const float* cand1_w;                         /* [1][4][4][4][64]         conv_gru1.convc.0 (8 of 16 rows) */
} adamvs_fuse_weights;

/* ---- FeatureNet0.forward, reference models/adamvs.py:49-152 (blocks models/module.py:164-251,
 * 506-524), for N = B*V images at once.  imgs [N][3][H][W] (the reference's layout); outputs channel-last, the layout
 * every entry point above takes: stage1 [N][(H/4)(W/4)][32], stage2 [N][(H/2)(W/2)][16], stage3 [N][H*W][8].
 * H and W must be multiples of 32.  base_channels = 8 (the only configuration the reference uses).
 *
 * Weights (ada-mvs_amd/packing.py::pack_feature_net): every convolution as fp32 MFMA A fragments with the eval-mode
 * BatchNorm scale folded in, w = [cout tile][tap][cin/4][64 lanes], lane l = W[16*tile + (l&15)][4*kc + (l>>4)][tap]
 * (rows beyond cout zero), and b = the BatchNorm shift padded to 16 per tile (zeros for the plain output convs).
 * conv0_0 (RGB + a zero channel) and conv0_1 run fused in one kernel and are stored as TWO-ROW fragments [12][cin/4][64], the
 * layout of adamvs_fuse_weights.conv1 (rows 0-7: output row y, tap ky = rr; rows 8-15: row y+1, tap ky = rr-1; rr = 0..3).
 * The 5x5 stride-2 convolutions hold 25 taps; conv2_0 is stored as two
 * 16-channel halves.  deconv*_t hold the ConvTranspose2d(k3,s2,p1,op1) weights per output parity class (py,px):
 * 1 + 2 + 2 + 4 taps in the order 00, 01, 10, 11, tap (ty,tx) = kernel index (py ? (ty ? 0 : 2) : 1, same in x) applied
 * to input pixel (i+ty, j+tx).  deconv*_c convolve cat(deconv output, skip); deconv2_c (8 output channels) is stored as
 * two-row fragments [12][4][64] like conv0.  out_k multiply the feature map only;
 * the pooled-context branches br_k_j = {w1 [C/2][C] (BN folded), b1 [C/2], w2 [C][C/2] = columns of out_k for that
 * branch} are applied at pooled resolution and their bilinear upsampling (align_corners=False) is added in the
 * epilogue of out_k (the 1x1 convolution and the upsampling are both linear). */
typedef struct adamvs_fconv_weights { const float* w; const float* b; } adamvs_fconv_weights;
typedef struct adamvs_context_weights { const float* w1; const float* b1; const float* w2; } adamvs_context_weights;
typedef struct adamvs_feature_weights {
  adamvs_fconv_weights conv0_0, conv0_1, conv1_0, conv1_1, conv1_2, conv2_0, conv2_1, conv2_2;
  adamvs_fconv_weights out1, deconv1_t, deconv1_c, out2, deconv2_t, deconv2_c, out3;
  adamvs_context_weights br1_1, br1_2, br2_1, br2_2, br3_1, br3_2;
} adamvs_feature_weights;
size_t adamvs_feature_net0_workspace_bytes(int N, int H, int W);
int adamvs_feature_net0(const float* imgs, const adamvs_feature_weights* weights, float* stage1, float* stage2, float* stage3,
                        int N, int H, int W, void* workspace, size_t workspace_bytes, void* stream);
/* The same network on the images as reference Infer_AdaMVSNet.forward receives them, imgs [B][V][3][H][W] (adamvs.py:574-577
 * runs the net view by view), without the view-major copy: the launch computes images m = n0 .. n0+n-1 of the V*B images in
 * view-major order (m = v * B + b, the order of the feature maps every entry point above takes), reading imgs[b][v] in place;
 * stage1..3 receive those n images.  n0 / n let a caller bound the workspace (adamvs_feature_net0_workspace_bytes(n, H, W)). */
int adamvs_feature_net0_views(const float* imgs, const adamvs_feature_weights* weights, float* stage1, float* stage2, float* stage3,
                              int B, int V, int n0, int n, int H, int W, void* workspace, size_t workspace_bytes, void* stream);

/* The FPN variant of MS-REDNet's FeatureNet, reference models/msrednet.py:74-91 (constructor), 115-125 (forward), arch_mode
 * "fpn" with three stages: stage1 = out1(conv2); t1 = nearest2x(conv2) + inner1(conv1); stage2 = out2(t1);
 * t2 = nearest2x(t1) + inner2(conv0); stage3 = out3(t2).  Same images, outputs and size rule as adamvs_feature_net0.
 * conv* as in adamvs_feature_weights; out1 [32][32] 1x1 (no bias: b = zeros); inner1 [32][16], inner2 [32][8] 1x1 with
 * b = their bias; out2 [16][32], out3 [8][32] 3x3, b = zeros (fragment layout of adamvs_fconv_weights). */
typedef struct adamvs_feature_fpn_weights {
  adamvs_fconv_weights conv0_0, conv0_1, conv1_0, conv1_1, conv1_2, conv2_0, conv2_1, conv2_2;
  adamvs_fconv_weights out1, inner1, out2, inner2, out3;
} adamvs_feature_fpn_weights;
size_t adamvs_feature_net_fpn_workspace_bytes(int N, int H, int W);
int adamvs_feature_net_fpn(const float* imgs, const adamvs_feature_fpn_weights* weights, float* stage1, float* stage2,
                           float* stage3, int N, int H, int W, void* workspace, size_t workspace_bytes, void* stream);

/* models/adamvs.py:495-512 fused with conv1 of SliceCostRegNetRED (adamvs.py:416), for all
 * D hypotheses at once: c1[d][b][pix][8] = ReLU(conv1(sum_v w_v warp_v ref / (1e-5 + sum_v w_v))).
 * view_weight [S][B][h*w].  Hypothesis loop inside the thread, bilinear taps cached in registers
 * across planes; the similarity of a chunk of planes (at most 32) goes through the workspace and conv1 runs
 * over it as a tiled MFMA convolution.  On return the workspace holds the aggregated similarity of the LAST
 * chunk, [planes of the chunk][B][h*w][C] (with D <= 32: of all planes; the parity tests read it there). */
size_t adamvs_aggregate_conv1_workspace_bytes(int B, int C, int D, int h, int w);
int adamvs_aggregate_conv1(const float* feat, const float* rt, const float* planes, const float* view_weight,
                           const float* w1pk, float* c1, int B, int S, int C, int D, int h, int w, int precision,
                           void* workspace, size_t workspace_bytes, void* stream);

/* SliceCostRegNetRED.forward, models/adamvs.py:415-424 (one recurrent step).
 * cost [B][h*w][C]; state1 [B][h*w][8], state2 [B][(h/2)*(w/2)][16] updated in place;
 * reg_cost [B][Ho*Wo] with Ho x Wo = 2h x 2w (in_up) or h x w.
 * scratch: adamvs_slice_reg_step_scratch_bytes(B,h,w) bytes. */
size_t adamvs_slice_reg_step_scratch_bytes(int B, int h, int w);
int adamvs_slice_reg_step(const float* cost, float* state1, float* state2, const adamvs_fuse_weights* weights,
                          float* reg_cost, int B, int C, int h, int w, int in_up, int precision, void* scratch,
                          size_t scratch_bytes, void* stream);

/* ---- whole stage: InferDepthNet0.forward, models/adamvs.py:433-533 -------- */
typedef struct adamvs_stage_desc {
  int B, S, C, h, w, D;   /* batch, source views (any number), feature channels, feature rows/cols, hypotheses (first stage:
                             at most 512; CostRegNet2D runs at adamvs_cost_reg_width(D, precision) channels) */
  int in_up;              /* 1: maps come out at 2h x 2w (stages 1, 2); 0: h x w (stage 3) */
  int first_stage;        /* 1: confidence_map is None -> pass A scores the views (stage 1) */
  int prev_h, prev_w;     /* size of prev_conf maps when !first_stage */
  int precision;          /* ADAMVS_PRECISION_* for CostRegNet2D (w_reg must be packed accordingly) */
  int precision_fuse;     /* ADAMVS_PRECISION_* for conv1 and the ConvGRU convolutions (w_fuse packed accordingly) */
  int eps_in_numerator;   /* where the 1e-5 of the weighted aggregation sits: 0 = InferDepthNet0, sum_v w_v x_v / (1e-5 +
                             sum_v w_v) (adamvs.py:497-512); 1 = the train/test twin DepthNet0, (1e-5 + sum_v w_v x_v) /
                             sum_v w_v (adamvs.py:262-300) */
  int plane_mode;         /* what `planes` points to: ADAMVS_PLANES_EXPLICIT [B][D][h*w] (caller-made depth_values, as
                             InferDepthNet0.forward receives them); ADAMVS_PLANES_UNIFORM [B][2] = (min, max) -> plane d =
                             min + d (max - min)/(D - 1) (module.py:650-658); ADAMVS_PLANES_WINDOW cur_depth [B][h*w] ->
                             lo = cur - half_span, hi = cur + half_span, plane d = lo + d (hi - lo)/(D - 1) (module.py:628-643).
                             Generated planes equal the materialised ones bit for bit and never cross HBM. */
  float half_span;        /* ADAMVS_PLANES_WINDOW: ndepth / 2 * depth_interval_pixel (module.py:632) */
  const float* half_span_dev; /* ADAMVS_PLANES_WINDOW, optional (NULL: half_span above): DEVICE pointer to that one float.  The value
                             is then read by the kernels when they run, not baked into the launch: a captured hipGraph of the
                             stage serves tiles of any depth range (ada_mvs_amd/graphed.py; predict_whu.py's loop) */
} adamvs_stage_desc;
#define ADAMVS_PLANES_EXPLICIT 0
#define ADAMVS_PLANES_UNIFORM  1
#define ADAMVS_PLANES_WINDOW   2

size_t adamvs_depth_stage_workspace_bytes(const adamvs_stage_desc* desc);

/* How a stage of B*h*w pixels runs its recurrence (for accounting: bench.py prices executed flops): the schedule
 * (0: one role per launch, sequential; 1, 3, 5: software-pipelined, see option recur_mode) and, for
 * schedule 0 in fp32, the bit mask of the GRU convolutions that run in the minimal-filtering form F(2x2, 3x3)
 * (1 gates1, 2 gates2, 4 cand2, 8 cand1: 16 of the 36 products of the direct form; option gru_wino, default 7). */
int adamvs_recurrence_schedule(int precision_fuse, long long pixels);
int adamvs_gru_wino_mask(void);

/* Which fp32 kernel a transposed CostRegNet2D layer (adamvs_conv3x3_dd, mode 2) of N maps of hi x wi inputs and D channels takes under
 * the current options: 0 class by class, 1 the four parity classes per chunk (small grids: option t2_fused), 2 the pair form along x
 * (15 of 18 products: D = 192 / 384, even widths whose rows fill blocks of 32 input columns; option s2_pairs).  -1: unsupported D. */
int adamvs_conv_t2_form(int N, int D, int hi, int wi);

/* Folded blocks (no option: the choice rounds differently in the network, so it goes by the maps alone and a tile gives the same bits
 * alone and in a batch).  The 16 matrix columns of an instruction need not lie in one row of the map: with a fold F they are 16 / F
 * pixel groups of each of F rows, and a block is F times narrower and taller with the same sums per pixel.
 *  - F(2x4, 3x3) (adamvs_conv3x3_dd_wino24): blocks of 8 x 32 pixels (F = 2) or 8 x 16 (F = 4) where they tile the map exactly and the
 *    64-pixel blocks do not.  Every block shape gives the same bits.  In adamvs_cost_reg_net_2d, fp32, D >= 192: conv2 and conv4 take
 *    the form on such blocks (widths 96, 48 of cfg2's inner levels); they stay in F(2x2, 3x3) elsewhere and under winograd = 3.
 *  - the stride-2 pair form (option s2_pairs; D = 192, 384): blocks of 6 x 16 (F = 2) or 12 x 8 outputs (F = 4) where they tile the map
 *    and the 32-column block does not divide the row (conv3, conv5 of cfg2), behind the small-grid rule of conv_rows2.
 * adamvs_conv_wino24_fold: the blocks a layer on h x w maps takes, 1 (64 pixels wide), 2 or 4.  adamvs_cost_reg_fold: conv2 / conv4 of
 * the network on h x w maps at that level: 2 or 4, 0 where the layer stays in F(2x2, 3x3) (N does not enter).  adamvs_conv_s2_form:
 * a stride-2 layer (mode 1, no skip) of N maps of hi x wi inputs: 0 a direct kernel, 1 the pair form on blocks of 3 x 32 outputs, 2 / 4
 * on folded blocks.  `blocks` = -1 asks what the plain entry points do; another value what the *_blocks entry points below do with
 * it.  -1: bad arguments / unsupported D.
 * The *_blocks entry points exist for A/B timing and tests: the plain entry point's arguments plus `blocks` --
 * adamvs_conv3x3_dd_wino24_blocks: -1 by the map, 1 the 64-pixel blocks, 2 / 4 that fold wherever the width is a multiple of 32 / 16;
 * adamvs_conv3x3_dd_s2_blocks (fp32, stride 2, no skip): -1 by the map, 0 the selection of before (no folded blocks), 2 / 4 that fold
 * wherever the output width is a multiple of 16 / 8; adamvs_cost_reg_net_2d_blocks (fp32): -1 as adamvs_cost_reg_net_2d, 0 no folded
 * blocks in any layer: the kernels of before, bit for bit. */
int adamvs_conv_wino24_fold(int h, int w, int blocks);
int adamvs_conv_s2_form(int N, int D, int hi, int wi, int blocks);
int adamvs_cost_reg_fold(int N, int D, int h, int w);
int adamvs_conv3x3_dd_wino24_blocks(const float* in, const float* wpk, const float* bias, const float* skip, float* out, int N, int D,
                                    int h, int w, int relu, int blocks, void* stream);
int adamvs_conv3x3_dd_s2_blocks(const float* in, const float* wpk, const float* bias, float* out, int N, int D, int hi, int wi, int relu,
                                int blocks, void* stream);
int adamvs_cost_reg_net_2d_blocks(const float* x, const float* wpk, size_t wpk_floats, float* score, int N, int D, int h, int w, int blocks,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* phases of a stage.  VIEW_WEIGHTS may run in a call of its own: its results are the view_weight / pair_depth OUTPUT
 * tensors, which a later call reads back.  AGGREGATE, RECURRENCE and SOFT_ARGMIN form one chain over chunks of 32
 * hypotheses (the workspace holds one chunk of conv1 outputs and two of cost slices, nothing of it grows with D), so
 * for D > 32 they produce maps only when all three are in ONE call: a call with a proper subset of them returns an
 * argument error (-1).  For D <= 32 (one chunk) every subset is valid, in order. */
#define ADAMVS_PHASE_VIEW_WEIGHTS 1  /* pass A (pair similarity, CostRegNet2D, softmax) or resample of prev_conf */
#define ADAMVS_PHASE_AGGREGATE    2  /* weighted aggregation + conv1 */
#define ADAMVS_PHASE_RECURRENCE   4  /* D sequential ConvGRU encoder-decoder steps */
#define ADAMVS_PHASE_SOFT_ARGMIN  8  /* depth / confidence from the regularised slices */
#define ADAMVS_PHASE_ALL         15

/* feat [V=S+1][B][h*w][C]; rt [B][S][12]; planes: see adamvs_stage_desc.plane_mode;
 * prev_conf [S][B][prev_h*prev_w] (previous stage's view weights; ignored when first_stage);
 * w_reg: packed CostRegNet2D weights at width adamvs_cost_reg_width(D, precision), w_reg_floats of them
 *        (= adamvs_cost_reg_net_2d_weight_floats(width, precision); first_stage only);
 * outputs: view_weight [S][B][h*w] (what the next stage consumes as prev_conf),
 *          pair_depth [S][B][h*w] (first_stage only), depth / confidence [B][Ho*Wo].
 * phases: ADAMVS_PHASE_ALL, or VIEW_WEIGHTS alone followed by the other three together (see above). */
int adamvs_depth_stage_forward(const adamvs_stage_desc* desc, const float* feat, const float* rt, const float* planes,
                               const float* prev_conf, const float* w_reg, size_t w_reg_floats, const adamvs_fuse_weights* w_fuse,
                               float* view_weight, float* pair_depth, float* depth, float* confidence,
                               int phases, void* workspace, size_t workspace_bytes, void* stream);

/* MEASUREMENT ONLY -- not part of the inference path.  The same arguments; runs the selected phases of a stage alone over all
 * chunks on whatever the workspace holds, also where adamvs_depth_stage_forward refuses (a proper subset of
 * AGGREGATE|RECURRENCE|SOFT_ARGMIN at D > 32): the call's duration is the phase's, depth / confidence are NOT valid
 * afterwards.  bench.py's phase-by-phase table uses it, after the timed region. */
int adamvs_bench_stage_phase(const adamvs_stage_desc* desc, const float* feat, const float* rt, const float* planes,
                             const float* prev_conf, const float* w_reg, size_t w_reg_floats, const adamvs_fuse_weights* w_fuse,
                             float* view_weight, float* pair_depth, float* depth, float* confidence,
                             int phases, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MS-REDNet inference (models/msrednet.py:330-436) ------------------------
 * The sibling model of predict_whu.py --model msrednet.  Its 3x3 convolutions run on adamvs_conv3x3_dd with the
 * channel counts zero-padded to a supported width; what follows are the pieces around them.  Maps are
 * channel-last [N][pixels][D]. */

/* Variance cost of the D hypothesis planes of a stage, msrednet.py:396-412: over the reference feature and the S source
 * features warped onto the plane (homo_warping_float, module.py:527-568): E[x^2] - E[x]^2 per channel, negated when
 * `negate` (both consumers take -cost, msrednet.py:351,362).  feat [V=S+1][B][h*w][C], rt [B][S][12],
 * planes [B][D][h*w] -> channels [0,C) of out_a [D][B][h*w][Da] (plane-major) and, when out_b != NULL, of
 * out_b [D][B][h*w][Db]; other channels untouched. */
int adamvs_red_variance_cost(const float* feat, const float* rt, const float* planes, float* out_a, int Da, float* out_b,
                             int Db, int B, int S, int C, int D, int h, int w, int negate, void* stream);

/* dst[b][p][dst_c0 + c] = src[b][p][src_c0 + c], c < n (strides in floats): narrows / widens / concatenates maps. */
int adamvs_channel_copy(const float* src, float* dst, int nbatch, int npix, int n, long src_batch_stride,
                        int src_pix_stride, int src_c0, long dst_batch_stride, int dst_pix_stride, int dst_c0, void* stream);

/* nn.GroupNorm(1, HC) statistics (module.py:63-68), in two deterministic halves.  _partial: for map g in {x0, x1}
 * (x1 may be NULL), over channels [0, n) and fixed pixel ranges of sample b: double-precision partial sums into
 * `partials` (adamvs_group_stats_workspace_bytes(N, ngroups)).  The two epilogues below finish the reduction
 * themselves; _finish does it standalone (same npix and n as _partial): stats[b][g] = {mean, 1/sqrt(biased var + eps)}. */
size_t adamvs_group_stats_workspace_bytes(int N, int ngroups);
int adamvs_group_stats_partial(const float* x0, const float* x1, int N, int npix, int D, int n, void* partials,
                               size_t partials_bytes, void* stream);
int adamvs_group_stats_finish(const void* partials, float* stats, int N, int ngroups, int npix, int n, float eps,
                              void* stream);

/* ConvGRUCell2.gates + the reset product, module.py:72-92.  The gate convolution is linear in cat(x, h):
 * gate_conv(cat(x, h)) = Wx.x + Wh.h + b, and so is the output convolution.  The x halves do not depend on the state
 * and are computed for all planes at once; per plane only the h halves remain, with the x halves added through the
 * `skip` operand of adamvs_conv3x3_dd.  fr, fu [N][npix][Wf]: reset / update halves (HC real channels each; two maps,
 * or fu = fr + HC inside one 2HC-wide map as adamvs_conv3x3_pair writes it);
 * partials from adamvs_group_stats_partial(fr, fu); gn [4][HC] = reset_gate_norm weight, bias, update_gate_norm
 * weight, bias; h [N][npix][W] the state.  -> rh = sigmoid(GN(fr)) * h [N][npix][W], u = sigmoid(GN(fu)) [N][npix][HC]. */
int adamvs_gru2_gates_apply(const float* fr, const float* fu, int Wf, const void* partials, const float* gn, const float* h,
                            float* rh, float* u, int N, int npix, int W, int HC, float eps, void* stream);

/* ConvGRUCell2.output + forward, module.py:91-106.  o [N][npix][W] = output_conv(cat(x, r*h)) (HC real channels);
 * partials from adamvs_group_stats_partial(o, NULL); gn [2][HC] = output_norm weight, bias.
 * h' = u*h + (1-u)*tanh(GN(o)) replaces h [N][npix][W] and goes to channels [0, HC) of out [N][npix][Wo] (may be NULL). */
int adamvs_gru2_out_apply(const float* o, const void* partials, const float* gn, const float* u, float* h, float* out,
                          int Wo, int N, int npix, int W, int HC, float eps, void* stream);

/* out = conv3x3(cat(srcA, srcB)) + bias, stride 1, zero padding, on COMPACT channel-last maps: srcA [B][h*w][CA],
 * srcB [B][h*w][CB] -> out [B][h*w][cout].  gate_conv / output_conv of ConvGRUCell2 (module.py:62-67) for the two shallow
 * levels of MS-REDNet, whose 8/16-channel states would waste a 16-wide k_conv_dd tile: weights stay in registers as
 * A fragments wpk [ceil(cout/16)][9][(CA+CB)/4][64] (value W[cout = 16*tile + (lane&15)][cin = 4*kc + (lane>>4)][tap]),
 * bias [16*ceil(cout/16)] zero padded.  (CA, CB, cout) in (32|16|8, 8, <=16) or (16, 16, <=32). */
int adamvs_conv3x3_pair(const float* srcA, int CA, const float* srcB, int CB, const float* wpk, const float* bias,
                        float* out, int cout, int B, int h, int w, void* stream);

/* One level's whole recurrence over the D planes of a stage (the loop of slice_RED_Regularization.forward restricted to
 * one ConvGRUCell2, msrednet.py:349-366), launched from native code: per plane the convolutions, the two GroupNorm
 * reductions and the two epilogues above (small maps: the partial sums come out of the convolutions' own epilogues, the
 * two gate convolutions of _split are one launch and, at one or two samples, the elementwise kernels are folded into the
 * window fill of the convolution that follows them -- two dependent launches per plane; ADAMVS_RED_FOLD_APPLIES=0 / 1
 * forces); the state starts at zero; h' of plane d goes to channels [0, HC) of
 * R [D][B][h*w][RW] (plane-major).  gn [6][HC] = reset / update / output norm weight, bias.
 * _pair (levels 1, 2): x [D][B][h*w][Cx] compact, wg / wc + bg / bc as for adamvs_conv3x3_pair (gate_conv with 2 HC
 * rows, output_conv).  _split (levels 3, 4): gxr, gxu, cx [D][B][h*w][W] = the x halves (+ bias) of the reset / update /
 * candidate convolutions, w_ghr / w_ghu / w_ch = the h halves as adamvs_conv3x3_dd blocks (9 W W fragment floats + W
 * zero bias floats each).  workspace: adamvs_red_recur_workspace_bytes(B, h, w, W, Wf, HC) with (W, Wf) = (HC, 2 HC)
 * for _pair and (W, W) for _split. */
size_t adamvs_red_recur_workspace_bytes(int B, int h, int w, int W, int Wf, int HC);
int adamvs_red_recur_pair(const float* x, int Cx, const float* wg, const float* bg, const float* wc, const float* bc,
                          const float* gn, float* R, int RW, int B, int D, int h, int w, int HC, float eps, void* workspace,
                          size_t workspace_bytes, void* stream);
int adamvs_red_recur_split(const float* gxr, const float* gxu, const float* cx, const float* w_ghr, const float* w_ghu,
                           const float* w_ch, const float* gn, float* R, int RW, int B, int D, int h, int w, int W, int HC,
                           float eps, void* workspace, size_t workspace_bytes, void* stream);

/* The running exp-sum / max / weighted-depth update of msrednet.py:415-436 (same as adamvs.py:512-531) in one pass over
 * the stored slices: vol [B][D][h*w] = reg_cost of every plane, planes [B][D][h*w] -> depth, confidence [B][h*w]. */
int adamvs_soft_argmin(const float* vol, const float* planes, float* depth, float* confidence, int B, int D, int h, int w,
                       void* stream);

/* ---- depth-map fusion (after predict_whu.py; the reference stops at writing the maps, predict_whu.py "step1") -------------
 * Geometric-consistency filtering of one reference view against up to ADAMVS_FUSION_MAX_SOURCES source views and the kept
 * pixels as world points (ada-mvs_amd/fusion.py drives it per view; fuse_whu.py is the CLI).  Pixel centres sit at integer
 * coordinates (the convention of homo_warping, models/module.py:527-568).  Three calls per view, enqueued on `stream`:
 * _geo_consistency -> _fusion_scan -> _fusion_emit; no atomics, output bit-identical from run to run, points in row-major
 * pixel order.  Workgroups cover ADAMVS_FUSION_TILE consecutive row-major pixels: nblocks = ceil(H W / ADAMVS_FUSION_TILE). */
#define ADAMVS_FUSION_MAX_SOURCES 16
#define ADAMVS_FUSION_TILE 256
int adamvs_fusion_max_sources(void);

/* One source view, host memory (copied into the kernel arguments).  depth: device pointer to its depth map [H][W] fp32.
 * fwd = {A row-major, b}: the source's homogeneous pixel of reference pixel (x, y) at depth d is d A [x y 1]^T + b
 * (A = K_s R_sr K_r^-1, b = K_s t_sr); back = {B, c}: the reference's homogeneous pixel of source pixel (u, v) at depth d_s
 * is d_s B [u v 1]^T + c (B = K_r R_rs K_s^-1, c = K_r t_rs).  The third component is the depth in that camera.  Formed
 * in fp64 by the caller and rounded to fp32: camera-frame magnitudes are depths and baselines, not world coordinates. */
typedef struct {
  const float* depth;
  int H, W;
  float fwd[12];
  float back[12];
} adamvs_fusion_source;

/* Per reference pixel p = (x, y) with d = ref_depth[p]: a candidate iff d is finite and > 0 and ref_conf[p] >= prob_threshold
 * (NaN is not).  Source s is consistent iff the projection has z > 0, lands in 0 <= u < W_s - 1, 0 <= v < H_s - 1, its four
 * bilinear taps of depth_s are finite and > 0, and the bilinear depth projected back gives |(x', y') - (x, y)| < pix_threshold
 * and |d' - d| < rel_depth_threshold d.  count[p] = number of consistent sources n (uint8); fused[p] = (d + sum d') / (1 + n)
 * if a candidate with n >= min_consistent, else 0; block_kept[nblocks] = number of kept pixels per workgroup.
 * ref_depth, ref_conf [H][W]; 1 <= N <= ADAMVS_FUSION_MAX_SOURCES; thresholds finite, pix / rel > 0, min_consistent >= 0. */
int adamvs_geo_consistency(const float* ref_depth, const float* ref_conf, int H, int W, const adamvs_fusion_source* sources,
                           int N, float prob_threshold, float pix_threshold, float rel_depth_threshold, int min_consistent,
                           unsigned char* count, float* fused, unsigned* block_kept, void* stream);

/* Exclusive scan: offsets[i] = sum of block_kept[0 .. i), offsets[nblocks] = the total (uint32, nblocks + 1 entries). */
int adamvs_fusion_scan(const unsigned* block_kept, unsigned* offsets, int nblocks, void* stream);

/* Every pixel with fused[p] > 0 becomes point offsets[block] + (its rank among the kept pixels of the block):
 * xyz[q] = R_wc (fused[p] K^-1 [x y 1]^T) + C in fp64 (world coordinates of aerial scenes reach 1e6 m: fp32 would lose
 * decimetres), rgb[q] = the first three bytes of rgba[p] (reference image [H][W][4] uint8).  camera: HOST pointer to 21
 * doubles {K^-1 row-major (9), R_wc row-major (9), C (3)}, camera axes x right / y down / z forward.  xyz [capacity][3],
 * rgb [capacity][3]; capacity >= H W is required (a view has at most H W points; none is written at or past capacity). */
int adamvs_fusion_emit(const float* fused, const unsigned char* rgba, int H, int W, const double* camera, const unsigned* offsets,
                       double* xyz, unsigned char* rgb, long capacity, void* stream);

/* ---- DSM (after fuse_whu.py): a point cloud rasterised into a digital surface model and a true orthophoto ----------------
 * ada-mvs_amd/dsm.py streams the points in chunks; dsm_whu.py is the CLI.  World axes: x east, y north, z up.
 *
 * Grid: column i, row j (row 0 is the northern edge).  A point (x, y, z) falls in  i = floor((x - x0) / gsd),
 * j = floor((y_top - y) / gsd),  both in fp64 with exactly these operations (cell (i, j) holds x0 + i gsd <= x < x0 + (i + 1) gsd
 * and y_top - (j + 1) gsd < y <= y_top - j gsd, up to the rounding of those operations),
 * and is USED iff 0 <= i < W, 0 <= j < H and |z - z_ref| < 65536 (all in fp64; NaN / inf coordinates are never used).
 * Point k of a call has the sequence number seq = seq0 + k (uint32; the stream holds fewer than 2^32 points).
 * Per used point  h = (float)(z - z_ref),  o(h) = the order-preserving uint32 of h's bits (-0 taken as +0: equal heights, equal
 * o), and the 64-bit key  o(h) << 32 | (0xFFFFFFFF - seq):  the highest point has the largest key, and among equal fp32 heights
 * the earliest point.  A used point's key is never 0; key 0 marks an empty cell.
 * Per cell: key = max over its used points, count = their number (uint32), and in ADAMVS_DSM_MEAN mode
 * sum = the int64 sum of q = rint((z - z_ref) * 65536.0) (exact while count * max|q| < 2^63, i.e. 2^31 points at +-65536 m).
 * Then for count >= min_count
 *   ADAMVS_DSM_MAX:  dsm = (float)(z_ref + (double)h of the max-key point)                     (the first-surface DSM)
 *   ADAMVS_DSM_MEAN: dsm = (float)(z_ref + ((double)sum / (double)count) / 65536.0)
 *   rgba = the RGB of the max-key point, alpha 255 (both modes);
 * and dsm = NaN (0x7fc00000), rgba = 0 for count < min_count.  count16 = min(count, 65535) for every cell.
 * Every reduction is an integer max or sum: the output is bit-identical from run to run, and in mean mode (dsm, count) under
 * any permutation or chunking of the points.
 *
 * Cell state (device, row-major [H][W], zeroed by the caller before the first chunk): key (uint64), count (uint32), color
 * (uint32 RGBA, little-endian r g b a), and sum (int64, mean mode only; may be NULL in max mode): 16 bytes per cell in max
 * mode, 24 in mean mode; the finalize outputs add 10 (dsm fp32, count16 uint16, rgba 4 x uint8).  W H <= ADAMVS_DSM_MAX_CELLS.
 * Per chunk: _dsm_accumulate, then _dsm_claim with the same points and seq0 (the lane whose key is the cell's key writes its
 * colour; a later chunk that wins the cell overwrites it in its own claim), in stream order; _dsm_finalize once at the end.
 * grid: HOST pointer (copied into the kernel arguments); xyz: device [n][3] fp64; rgb: device [n][3] uint8; the finalize
 * outputs dsm [H][W] fp32, count16 [H][W] uint16, rgba [H][W][4] uint8 (4-byte aligned: written as one uint32 per cell).
 * Argument errors (<0, before any launch): a null pointer, n < 0, seq0 < 0 or seq0 + n > 2^32, gsd <= 0 or not finite,
 * x0 / y_top / z_ref not finite, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, a mode other than the two below, min_count < 1.
 * n = 0 is valid and launches nothing. */
#define ADAMVS_DSM_MAX 0
#define ADAMVS_DSM_MEAN 1
#define ADAMVS_DSM_MAX_CELLS (1 << 28)

typedef struct {
  double x0, y_top, gsd, z_ref;
  int W, H;
} adamvs_dsm_grid;

int adamvs_dsm_accumulate(const adamvs_dsm_grid* grid, const double* xyz, long n, long seq0, int mode, unsigned long long* key,
                          unsigned* count, long long* sum, void* stream);
int adamvs_dsm_claim(const adamvs_dsm_grid* grid, const double* xyz, const unsigned char* rgb, long n, long seq0,
                     const unsigned long long* key, unsigned* color, void* stream);
int adamvs_dsm_finalize(const adamvs_dsm_grid* grid, const unsigned long long* key, const unsigned* count, const long long* sum,
                        const unsigned* color, int mode, int min_count, float* dsm, unsigned short* count16, unsigned char* rgba,
                        void* stream);

/* ---- DSM gap fill (after _dsm_finalize): bounded harmonic interpolation of the empty cells -----------------------------
 * ada-mvs_amd/dsm.py fill_gaps(); dsm_whu.py --fill_max_dist METRES (r = max_dist / gsd).
 * Input: a finalised raster as _dsm_finalize writes it, dsm [H][W] fp32 (NaN where empty) and rgba [H][W][4] uint8, and a
 * radius r in cells (fp64).  Cells (i, j) are row i, column j; N4(c) are the (up to) 4 edge neighbours of c inside the grid.
 *   V        the valid cells: dsm finite.
 *   dist2    int32, the exact squared Euclidean distance in cells to the nearest valid cell, min over (k, l) in V of
 *            (i - k)^2 + (j - l)^2, wherever (double)dist2 <= r * r; INT32_MAX everywhere else (every cell when V is empty).
 *            0 on V.
 *   F        the fillable cells: not in V and (double)dist2 <= r * r.  Every other empty cell stays empty (dsm NaN
 *            0x7fc00000, rgba 0).
 *   height   for every c in F:  sum over n in N4(c) & (V | F) of (u_n - u_c) = 0,  u = dsm on V.  Neighbours outside the grid
 *            or left empty are left out of the sum (zero flux: a Neumann boundary).  Every F cell has a 4-connected path
 *            through F to V: take its nearest valid cell (k, l); a step from (i, j) that shrinks |i - k| or |j - l| by one
 *            strictly lowers the squared distance to (k, l), so it lands in V or in a cell whose dist2 is smaller, hence in
 *            F (or V); repeat.  So every connected component of F touches V (a Dirichlet boundary), the matrix of the system
 *            (diagonal = the number of neighbours in V | F, -1 per neighbour in F) is symmetric, irreducibly diagonally
 *            dominant with an M-matrix structure per component, hence positive definite: the solution is unique.  Solved in
 *            fp64; dsm_out = (float)u on F, and V cells are copied bit for bit (dsm and rgba).
 *   colour   R, G and B each solve the same equation with the colours of V as boundary values (fp32);
 *            rgba_out = (uint8)clamp(rint(u), 0, 255) per channel and alpha 255 on F.
 *   filled   uint8: 1 on F, 0 elsewhere.
 * Stopping rule: the residual of a cell of F is |left side of the height (colour) equation|.  Multigrid V-cycles run until
 * the largest residual over F is <= tol_height for the height and <= tol_colour for every colour channel (both checked
 * after each cycle from an exact integer max reduction: the output is bit-identical from run to run), or until
 * max_cycles cycles.  stats (a HOST pointer): cycles run, converged (0 when max_cycles ended the solve: the caller must
 * not take the result as the solution), the largest residuals reached, and the cells in V, in F and left empty.
 * An empty V or an empty F is valid input: the outputs equal the inputs, cells_filled = 0, converged = 1, cycles = 0.
 * Kernels (csrc/dsm_fill.hip): the distance in two windowed passes (per column, then per row with the row segment in LDS),
 * both bounded by R = ceil(r) per cell; multigrid V-cycles with red-black Gauss-Seidel smoothing, levels halved down to
 * <= 8 x 8 cells (a coarse cell is Dirichlet if a child is, unknown if a child is and none is Dirichlet, excluded otherwise),
 * the unscaled 5-point operator on every level, cell-centred bilinear prolongation over the coarse cells that are not
 * excluded and its transpose as restriction.
 * The call runs on `stream` and blocks: it reads the two residual maxima back once per cycle.
 * workspace: device memory of at least _dsm_fill_workspace_bytes(W, H) bytes (about 66 bytes per cell), 256-byte aligned.
 * dsm, rgba, dsm_out, rgba_out (4-byte aligned), dist2, filled: device [H][W]; outputs must not alias the inputs.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, r not finite or <= 0
 * or > ADAMVS_DSM_FILL_MAX_RADIUS, a tolerance not finite or <= 0, max_cycles < 1, workspace_bytes below the query.
 * _dsm_fill_workspace_bytes returns < 0 for W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS. */
#define ADAMVS_DSM_FILL_MAX_RADIUS 1024

typedef struct {
  int cycles, converged;
  double residual_height, residual_colour;
  long cells_valid, cells_filled, cells_empty;
} adamvs_dsm_fill_stats;

long adamvs_dsm_fill_workspace_bytes(int W, int H);
int adamvs_dsm_fill(int W, int H, const float* dsm, const unsigned char* rgba, double r_cells, double tol_height, double tol_colour,
                    int max_cycles, void* workspace, long workspace_bytes, float* dsm_out, unsigned char* rgba_out, int* dist2,
                    unsigned char* filled, adamvs_dsm_fill_stats* stats, void* stream);

/* ---- DSM ground filter (after _dsm_finalize or _dsm_fill): which cells of the DSM are bare earth -----------------------------
 * ada-mvs_amd/dtm.py ground_filter(); dtm_whu.py is the CLI.  A progressive morphological filter (Zhang et al. 2003, the
 * raster method behind PCL's and PDAL's `pmf`) with square windows.
 * Input: dsm [H][W] fp32 as _dsm_finalize / _dsm_fill write it.  A cell is VALID iff its value is finite; NaN and +-inf are
 * empty.  W H <= ADAMVS_DSM_MAX_CELLS.
 *
 * Opening open(Z, r), integer radius 1 <= r <= ADAMVS_DTM_MAX_RADIUS.  The window of cell c = (i, j) is the square
 * |i' - i| <= r, |j' - j| <= r; cells outside the grid and empty cells are ignored.
 *   E(c) = min of Z over the valid cells of the window of c (none if it holds no valid cell);
 *   O(c) = max of E over the cells of the window of c that have an E;
 *   output = O(c) on valid c, NaN (0x7fc00000) on empty c.
 * On a valid c, O is finite and O(c) <= Z(c): every window that holds c has E <= Z(c), and c's own window has an E.  Square
 * windows are separable (the row pass followed by the column pass is the 2-D result), and min / max select input values, so
 * the result is exact: equal to a restatement value for value (-0 and +0 compare equal; which of the two is selected is not
 * specified).
 *
 * Schedule (computed by the caller, ada-mvs_amd/dtm.py schedule(), and passed in as HOST arrays, so the kernel and a reference
 * use the same doubles): R = floor(max_radius / gsd), 1 <= R <= ADAMVS_DTM_MAX_RADIUS; radii r_k = 1, 2, 4, ... while below R,
 * then R: K <= ADAMVS_DTM_MAX_LEVELS levels; w_k = 2 r_k + 1, w_0 = 1;
 *   dh_k = min(dh_max, dh0 + slope * gsd * (w_k - w_{k-1}))   in fp64.
 * The entry point takes any strictly ascending radii and any finite dh > 0.
 *
 * Filter.  Z_0 = dsm.  For k = 1 .. K:  O_k = open(Z_{k-1}, r_k); a valid cell that is not yet flagged gets level = k iff
 *   (double)Z_{k-1}(c) - (double)O_k(c) > dh_k    (strictly);
 * Z_k = O_k.  Empty cells stay NaN at every level.
 *   level   uint8 [H][W]: 0 ground, k the level at which the cell was flagged as object, 255 empty.
 *   opened  fp32 [H][W]: Z_K.
 *   stats   (a HOST pointer) integer counts: cells valid, ground, object, empty, and cells_level[k] flagged at level k
 *           (cells_level[0] = ground; entries above `levels` are 0).
 * The products built on it (ada-mvs_amd/dtm.py): ground = dsm where level == 0, else NaN; dtm = the gap fill of ground
 * (_dsm_fill, unchanged: ground cells bit for bit, object and empty cells within the fill radius of ground by harmonic
 * interpolation, NaN farther away); ndsm = (float)((double)dsm - (double)dtm) where both are finite, NaN elsewhere.
 * Limits: an object wider than 2 R + 1 cells in both axes survives every opening and is kept as ground; an object lower than
 * dh_k is not flagged; a plane with gradients (gx, gy) per metre is left alone only while |gx| + |gy| < slope (the L1 norm:
 * the window is a square); at the high edge of a slope the dh_max cap can flag ground.
 *
 * Kernels (csrc/dsm_dtm.hip): a running min / max along rows (the segment and r halo cells in LDS, windows formed by doubling:
 * log2 r steps per cell, one form for every r) and a tiled transpose; the column passes are row passes on the transposed
 * raster.  _dtm_classify enqueues all K levels on `stream` with no host round trip between them, the flag and count step
 * folded into the last pass of each level, then reads the counts back once: it blocks.  _dsm_open does not block.
 * Every count is an integer sum: level, opened and the counts are bit-identical from run to run.
 * src / dsm, dst / opened: device [H][W] fp32; level: device [H][W] uint8; radius, dh: HOST arrays of `levels` entries.
 * workspace: device memory of at least _dtm_workspace_bytes(W, H) bytes (about 8 bytes per cell), 256-byte aligned.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, r or a radius outside
 * 1 .. ADAMVS_DTM_MAX_RADIUS, levels outside 1 .. ADAMVS_DTM_MAX_LEVELS, radii not strictly ascending, a dh not finite or
 * not > 0, any two of the buffers (workspace included) overlapping, workspace_bytes below the query.
 * _dtm_workspace_bytes returns < 0 for W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS. */
#define ADAMVS_DTM_MAX_RADIUS 1024
#define ADAMVS_DTM_MAX_LEVELS 16
#define ADAMVS_DTM_TILE 1024 /* cells of a row per workgroup of the running min / max */

typedef struct {
  int levels;
  long cells_valid, cells_ground, cells_object, cells_empty;
  long cells_level[ADAMVS_DTM_MAX_LEVELS + 1];
} adamvs_dtm_stats;

long adamvs_dtm_workspace_bytes(int W, int H);
int adamvs_dsm_open(int W, int H, const float* src, int r, void* workspace, long workspace_bytes, float* dst, void* stream);
int adamvs_dtm_classify(int W, int H, const float* dsm, int levels, const int* radius, const double* dh, void* workspace,
                        long workspace_bytes, unsigned char* level, float* opened, adamvs_dtm_stats* stats, void* stream);

/* ---- Building extraction (after the ground filter): which cells of the nDSM belong to a building, as labelled components ----
 * ada-mvs_amd/buildings.py extract(); buildings_whu.py is the CLI.  Inputs: dsm [H][W] fp32 (Z) and ndsm [H][W] fp32 as
 * dtm_whu.py writes them (NaN where there is no value).  W H <= ADAMVS_DSM_MAX_CELLS.  A cell is c = (i, j), its index i W + j.
 *
 * 1. Candidate mask.  M0(c) iff ndsm(c) is finite and (double)ndsm(c) >= min_height.
 * 2. Opening.  M = (open(M0 as 0.0 / 1.0, r_open) == 1.0) with _dsm_open above, unchanged: every cell of the 0 / 1 raster is
 *    valid and the window is clipped at the grid.  r_open = 0 skips it (M = M0).  The caller computes
 *    r_open = floor(min_width / (2 gsd)) cells; 0 <= r_open <= ADAMVS_DTM_MAX_RADIUS.  M is a subset of M0.
 * 3. Flatness flag of every cell of M, at the stride 1 <= s <= ADAMVS_BLD_MAX_STRIDE cells (the caller computes
 *    s = max(1, round(smooth_span / gsd))).  Directions d in {(0, 1), (1, 0), (1, 1), (1, -1)}.  A direction COUNTS iff
 *    c - s d and c + s d are both inside the grid, both in M, and both have a finite Z.  For a counting direction
 *      D = fabs(((double)Z(c - s d) + (double)Z(c + s d)) - 2.0 * (double)Z(c))
 *    every operation in fp64, in this order, no contraction.  A cell with no counting direction is undetermined; otherwise
 *    it is smooth iff D <= smooth_tol holds for every counting direction (a NaN D, from a non-finite Z(c), fails it), else
 *    rough.  flags uint8 [H][W]: 0 not a candidate, 1 removed by the opening, 2 undetermined, 3 smooth, 4 rough.
 *    A planar roof of any pitch has D = 0; a ridge is rough only across the ridge line; a crown is rough everywhere.
 * 4. Components: the 4-connected components of M (cells that touch only at a corner are not joined).
 *    _bld_label writes parent int32 [H][W]: -1 outside M, otherwise the smallest cell index of the cell's component.  The
 *    components are numbered 1 .. N in ascending order of that index (the caller scans the cells with parent == own index);
 *    label int32 [H][W] holds that number, 0 outside M.  The numbering follows from the mask alone.
 * 5. Table, int64 [ADAMVS_BLD_COLUMNS][N], row k - 1 for component k: cells; smooth, rough, undetermined (counts of the flags
 *    3, 4, 2); row_min, row_max, col_min, col_max; height_sum = the integer sum of llrint(min((double)ndsm, 65535.0) * 1024.0)
 *    (round to nearest, ties to even); height_max_bits = the largest fp32 bit pattern of ndsm (the values are positive, so
 *    the order of the patterns is the order of the values).  Integer sums, minima and maxima only.
 * 6. Selection and 7. vectorising run on the host (ada-mvs_amd/buildings.py select(), polygons()).
 *
 * Kernels (csrc/dsm_buildings.hip).  _bld_flags: the mask, the opening's six passes, then one pass that reads up to eight
 * neighbours of M and of Z at the stride directly (each such read is a coalesced row segment served by L2; a tile with an
 * s-cell halo in LDS would load (1 + 2 s / T)^2 times the tile to use nine points of it).  _bld_label: one workgroup resolves a
 * tile of ADAMVS_BLD_TILE_W x ADAMVS_BLD_TILE_H cells in LDS (row runs from wave ballots, unions by atomicMin on LDS labels
 * until a pass changes nothing), then rounds over the pairs of adjacent cells on tile borders only: read both roots (one
 * kernel), hook the larger root to the smaller by integer atomicMin (the next kernel, so every read saw the previous round's
 * state), walk the border cells to their roots (a third), until a round finds no pair with two roots; at most
 * ADAMVS_BLD_MAX_ROUNDS rounds, more is an error return (ADAMVS_BLD_NOT_CONVERGED), never a longer loop.  No workgroup waits
 * on another; visibility between rounds comes from the kernel boundaries.  _bld_table: one pass; the lanes of a wave that
 * follow one another in a row with the same label are summed in registers and one lane issues the atomics of the run.
 * flags, parent, label and the table are bit-identical from run to run: no floating-point atomic, no floating-point sum.
 * _bld_flags and _bld_table do not block; _bld_label reads one word per round back and blocks.
 * dsm, ndsm, flags, parent, label, table, workspace: device memory; workspace of at least _bld_workspace_bytes(W, H) bytes
 * (about 16 bytes per cell), 256-byte aligned; stats: a HOST pointer.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, min_height not finite or
 * <= 0, r_open outside 0 .. ADAMVS_DTM_MAX_RADIUS, s outside 1 .. ADAMVS_BLD_MAX_STRIDE, smooth_tol not finite or < 0,
 * N < 0 or N > W H, workspace_bytes below the query, any two of the buffers (workspace included) overlapping.
 * _bld_workspace_bytes returns < 0 for W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS. */
#define ADAMVS_BLD_TILE_W 64 /* cells of a row per tile of the labelling: one wave */
#define ADAMVS_BLD_TILE_H 64
#define ADAMVS_BLD_MAX_STRIDE 64
#define ADAMVS_BLD_MAX_ROUNDS 64
#define ADAMVS_BLD_NOT_CONVERGED (-2)
#define ADAMVS_BLD_COLUMNS 10
enum {
  ADAMVS_BLD_CELLS = 0, ADAMVS_BLD_SMOOTH = 1, ADAMVS_BLD_ROUGH = 2, ADAMVS_BLD_UNDETERMINED = 3, ADAMVS_BLD_ROW_MIN = 4,
  ADAMVS_BLD_ROW_MAX = 5, ADAMVS_BLD_COL_MIN = 6, ADAMVS_BLD_COL_MAX = 7, ADAMVS_BLD_HEIGHT_SUM = 8, ADAMVS_BLD_HEIGHT_MAX_BITS = 9
};

typedef struct {
  int rounds;      /* border rounds that hooked something (<= ADAMVS_BLD_MAX_ROUNDS) */
  int converged;   /* 1 unless the cap was hit */
  long tiles;      /* workgroups of the tile phase */
  long pairs;      /* pairs of adjacent cells on tile borders examined per round */
  float ms_tile, ms_rounds, ms_compress; /* device time of the tile phase, of the border rounds (their read-backs included)
                                            and of the final walk to the roots, in milliseconds; -1 if the events failed */
} adamvs_bld_stats;

long adamvs_bld_workspace_bytes(int W, int H);
int adamvs_bld_flags(int W, int H, const float* dsm, const float* ndsm, double min_height, int r_open, int s, double smooth_tol,
                     void* workspace, long workspace_bytes, unsigned char* flags, void* stream);
int adamvs_bld_label(int W, int H, const unsigned char* flags, void* workspace, long workspace_bytes, int* parent,
                     adamvs_bld_stats* stats, void* stream);
int adamvs_bld_table(int W, int H, const unsigned char* flags, const float* ndsm, const int* label, long N, long long* table,
                     void* stream);

/* ---- Roof planes (after the building extraction): the roof of every building cut into planar faces --------------------------
 * ada-mvs_amd/roofs.py extract(); roofs_whu.py is the CLI.  Inputs: dsm [H][W] fp32 (Z, NaN where there is no value) and
 * building [H][W] int32 (0 = none, 1 .. B, the label raster of buildings_whu.py).  W, H <= ADAMVS_ROOF_MAX_SIDE and
 * W H <= ADAMVS_DSM_MAX_CELLS.  A cell is c = (i, j), its index i W + j, rows running south; u = j, v = i.  Smoothness-constraint
 * region growing (Rabbani et al. 2006) restated without a visiting order.  The caller derives s = max(1, round(smooth_span / gsd))
 * (1 .. ADAMVS_BLD_MAX_STRIDE), g_tol = slope_tol * (2 s gsd) (metres over 2 s cells) and z_ref = floor(min finite Z).  Every
 * floating-point operation below is fp64 on the fp32 inputs widened first, in the order written, no contraction.
 *
 * 1. Links (_roof_links), uint8 [H][W].  Cell c is CORE iff building(c) = b > 0, the four cells (i, j -+ s), (i -+ s, j) are inside
 *    the grid, carry the label b and have a finite Z, Z(c) is finite, and
 *      fabs((Z(i, j + s) + Z(i, j - s)) - 2.0 * Z(c)) <= smooth_tol   and   fabs((Z(i + s, j) + Z(i - s, j)) - 2.0 * Z(c)) <= smooth_tol.
 *    Gradients of a core cell: gx = Z(i, j + s) - Z(i, j - s), gy = Z(i + s, j) - Z(i - s, j).  Core cell a has an EAST link to
 *    b = (i, j + 1) iff b is inside the grid and core with the same building label, fabs(gx(a) - gx(b)) <= g_tol,
 *    fabs(gy(a) - gy(b)) <= g_tol and fabs((Z(b) - Z(a)) - (gx(a) + gx(b)) / (4.0 * s)) <= step_tol.  The SOUTH link to
 *    b = (i + 1, j) is the same with (gy(a) + gy(b)) in the last test.  Every test is symmetric in a and b.
 *    link(c) = core | east << 1 | south << 2.
 * 2. Segments (_roof_label): the connected components of the graph whose nodes are the cells with bit 0 set and whose edges
 *    are: c - (i, j + 1) iff bit 1 of link(c) is set, c - (i + 1, j) iff bit 2 is set, and in both cases both cells are inside the
 *    grid and have bit 0 set (a link bit on a cell without bit 0, or towards such a cell or the outside, is ignored; bits 3 .. 7
 *    are ignored).  Two adjacent core cells without a link are NOT joined.  parent int32 [H][W]: -1 where bit 0 is clear,
 *    otherwise the smallest cell index of the segment.  Segments are numbered 1 .. S in ascending order of that index.
 * 3. Moments (_roof_moments), int64 [ADAMVS_ROOF_COLUMNS][N], row k - 1 for label k; any label raster (0 or outside 1 .. N =
 *    no label).  q = llrint(min(max((Z - z_ref) * 256.0, 0.0), 524287.0)) (round to nearest, ties to even: 0 .. 2^19 - 1).  Over
 *    the cells with label k and a finite Z: n, su, sv, sq, suu, suv, svv, suq, svq (sums of 1, u, v, q, u u, u v, v v, u q, v q),
 *    sqq_lo = sum of (q q & 0xFFFFF), sqq_hi = sum of (q q >> 20), row_min, row_max, col_min, col_max, q_min, q_max, building
 *    (the largest building(c)).  A label without such a cell: sums 0, minima 2^31 - 1, maxima -1.
 *    Overflow: with u, v < 2^15, q < 2^19 and at most 2^28 cells the largest sums are suq, svq < 2^15 2^19 2^28 = 2^62,
 *    suu, suv, svv < 2^58, sqq_lo < 2^48, sqq_hi < 2^18 2^28 = 2^46: every sum stays below 2^63.
 * 4. Planes (host, exact integers).  With Suu = n suu - su su, Svv = n svv - sv sv, Suv = n suv - su sv, Suq = n suq - su sq,
 *    Svq = n svq - sv sq and D = Suu Svv - Suv Suv: a segment is kept iff n gsd^2 >= min_plane_area and D != 0.  The plane
 *    q ~ a u + b v + c is a = (Suq Svv - Svq Suv) / D, b = (Svq Suu - Suq Suv) / D, c = (sq - a su - b sv) / n as rationals, its
 *    sse = sqq - a suq - b svq - c sq with sqq = sqq_lo + (sqq_hi << 20).  Each of a / 256, b / 256, c / 256 is rounded once to
 *    fp64: metres per cell, metres per cell, metres above z_ref.  Kept segments are renumbered 1 .. P in order.
 * 5. Growth (_roof_grow), rounds over two label buffers.  In a round a cell with building(c) > 0, a finite Z and label 0 looks at
 *    its four neighbours' labels as of the previous round.  Candidates: the labels 1 <= p <= P on neighbours inside the grid with
 *    building(neighbour) == building(c).  e_p = fabs((Z - z_ref) - ((a_p * j + b_p * i) + c_p)).  The cell takes the candidate of
 *    least e_p, ties to the smaller p, iff that e_p <= assign_tol (a NaN e_p is never the least and never passes).  Every other
 *    cell keeps its label.  counts[k] = the cells labelled in round k.  A round that labels nothing is a fixed point.
 * 6. Merge (host): ada-mvs_amd/roofs.py merge_planes().  7. Residuals (_roof_residuals), int64 [2][R], row p - 1 for label p, over
 *    the cells with label p and a finite Z: row 0 the count of cells with e_p <= assign_tol, row 1 the largest
 *    llrint(min(e_p * 1024.0, 1048576.0)) (a NaN e_p: not counted, and the largest is 1048576); both 0 for a label without cells.
 *
 * Kernels (csrc/dsm_roofs.hip).  _roof_links: one pass, one lane per cell, the stride neighbours of the cell, of its east and of
 * its south neighbour read straight from global memory (coalesced row segments served by L2, as in _bld_flags).  _roof_label:
 * the scheme of _bld_label with the link bits in place of the mask: tiles of ADAMVS_BLD_TILE_W x ADAMVS_BLD_TILE_H in LDS (a
 * row run starts after the nearest lane to the left whose east edge is missing; vertical unions where the upper cell's south
 * edge exists), then rounds over the tile-border pairs whose edge exists: pairs kernel, hook kernel, compress kernel (the last
 * two are the building stage's), at most ADAMVS_BLD_MAX_ROUNDS rounds, more is ADAMVS_BLD_NOT_CONVERGED.  No workgroup waits
 * on another; visibility between rounds comes from the kernel boundaries; every loop is bounded.  _roof_moments and
 * _roof_residuals: integer atomics only, one set per run of equal labels in a wave (a segmented shuffle reduction).
 * _roof_grow runs the rounds round0 .. round0 + rounds - 1, one launch each: round k reads label[k & 1] and writes every cell of
 * label[(k + 1) & 1], counts[k] is zeroed first; round0 + rounds <= ADAMVS_ROOF_MAX_GROW.  The caller may read counts back
 * between calls and stop after a round that labelled nothing.  Everything is bit-identical from run to run: no floating-point
 * atomic, no floating-point sum.  Only _roof_label blocks.
 * All buffers device memory (planes: fp64 [P][3] = a, b, c of step 4; counts: uint32 [ADAMVS_ROOF_MAX_GROW]); workspace of at
 * least _roof_workspace_bytes(W, H) bytes, 256-byte aligned; stats: a HOST pointer.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or > ADAMVS_ROOF_MAX_SIDE or W H > ADAMVS_DSM_MAX_CELLS,
 * s outside 1 .. ADAMVS_BLD_MAX_STRIDE, a tolerance or z_ref not finite, a tolerance < 0, N, P or R < 0 or > W H, rounds < 0,
 * round0 < 0 or round0 + rounds > ADAMVS_ROOF_MAX_GROW, workspace_bytes below the query, any two buffers overlapping.
 * _roof_workspace_bytes returns < 0 for a grid outside the limits. */
#define ADAMVS_ROOF_MAX_SIDE 32768
#define ADAMVS_ROOF_MAX_GROW 256
#define ADAMVS_ROOF_Q_SCALE 256
#define ADAMVS_ROOF_Q_MAX 524287 /* 2^19 - 1 */
#define ADAMVS_ROOF_COLUMNS 18
enum {
  ADAMVS_ROOF_N = 0, ADAMVS_ROOF_SU = 1, ADAMVS_ROOF_SV = 2, ADAMVS_ROOF_SQ = 3, ADAMVS_ROOF_SUU = 4, ADAMVS_ROOF_SUV = 5,
  ADAMVS_ROOF_SVV = 6, ADAMVS_ROOF_SUQ = 7, ADAMVS_ROOF_SVQ = 8, ADAMVS_ROOF_SQQ_LO = 9, ADAMVS_ROOF_SQQ_HI = 10,
  ADAMVS_ROOF_ROW_MIN = 11, ADAMVS_ROOF_ROW_MAX = 12, ADAMVS_ROOF_COL_MIN = 13, ADAMVS_ROOF_COL_MAX = 14, ADAMVS_ROOF_Q_MIN = 15,
  ADAMVS_ROOF_Q_MAX_COL = 16, ADAMVS_ROOF_BUILDING = 17
};

long adamvs_roof_workspace_bytes(int W, int H);
int adamvs_roof_links(int W, int H, const float* dsm, const int* building, int s, double smooth_tol, double g_tol, double step_tol,
                      unsigned char* link, void* stream);
int adamvs_roof_label(int W, int H, const unsigned char* link, void* workspace, long workspace_bytes, int* parent,
                      adamvs_bld_stats* stats, void* stream);
int adamvs_roof_moments(int W, int H, const float* dsm, const int* label, const int* building, double z_ref, long N,
                        long long* table, void* stream);
int adamvs_roof_grow(int W, int H, const float* dsm, const int* building, double z_ref, long P, const double* planes,
                     double assign_tol, int round0, int rounds, int* label0, int* label1, unsigned* counts, void* stream);
int adamvs_roof_residuals(int W, int H, const float* dsm, const int* label, double z_ref, long R, const double* planes,
                          double assign_tol, long long* table, void* stream);

/* ---- LoD2 solids (after the roof planes): footprints, roof planes and terrain joined into one watertight solid per building --
 * ada-mvs_amd/lod2.py extract(); lod2_whu.py is the CLI.  Inputs: dtm [H][W] fp32 (terrain, NaN where there is no value),
 * building [H][W] int32 (0 = none, 1 .. B), roof [H][W] int32 (0 = none, 1 .. P, the plane labels of roofs_whu.py) and per plane
 * p its building bld(p) and its equation.  W, H <= ADAMVS_LOD2_MAX_SIDE and W H <= ADAMVS_DSM_MAX_CELLS.  A cell is (i, j), rows
 * running south; a lattice CORNER is (r, c), r in 0 .. H, c in 0 .. W: the north-west corner of cell (r, c).  Everything is
 * integer: heights in 1 / ADAMVS_LOD2_Z_SCALE m above z_ref = floor(min finite dtm), horizontal positions in
 * 1 / ADAMVS_LOD2_XY_SCALE of a cell.  No step depends on a visiting order; every output is bit-identical from run to run.
 *
 * 1. Planes as integers (host).  From plane p's z = z0 + sx (x - xc) + sy (y - yc) and the grid (x0, y_top, gsd), in fp64 in the
 *    order written: a = sx * gsd, b = -(sy * gsd) (metres per cell east and south),
 *    c = ((z0 + sx * ((x0 + 0.5 * gsd) - xc)) + sy * ((y_top - 0.5 * gsd) - yc)) - z_ref (metres at the centre of cell (0, 0)).
 *    A, B, C = rint(a 2^20), rint(b 2^20), rint(c 2^20) (ties to even) as int64; planes int64 [P][3].  The height of plane p at
 *    corner (r, c) is   zq = floor((A (2 c - 1) + B (2 r - 1) + 2 C + 2^10) / 2^11)   (round half up), evaluated in int64 by the one
 *    function lod2_corner_height() of csrc/lod2_plane.h on the device and on the host (_lod2_corner_heights_host).  The caller
 *    refuses a plane with |A| or |B| >= 2^40, |C| >= 2^50, or |zq| >= ADAMVS_LOD2_Z_MAX at one of the four grid corners (zq is
 *    monotonic along either axis, so it then holds at every corner); a record holds zq as an int32.
 * 2. Model labels (_lod2_fill), rounds over two label buffers.  The caller starts from m_0(c) = roof(c) if 1 <= roof(c) <= P and
 *    building(c) = bld(roof(c)) > 0, else 0.  In a round a cell with building(c) = b > 0 and label 0 (a label outside 1 .. P reads
 *    as 0) takes the smallest label 1 .. P among its four neighbours inside the grid with building = b, as of the previous
 *    round; a cell with building(c) <= 0 gets 0; every other cell keeps its label.  counts[k] = the cells labelled in round k.  A
 *    round that labels nothing is a fixed point.  At most ADAMVS_LOD2_MAX_FILL rounds.
 * 3. Building table (_lod2_table), int64 [ADAMVS_LOD2_COLUMNS][B], row k - 1 for building k, over the cells with building(c) = k:
 *    cells; filled = those with a model label 1 .. P; base = the smallest
 *    (long long)fmin(fmax(floor(((double)dtm - z_ref) * 1024.0), -2^30), 2^30) over those with a finite dtm; roof_min = the smallest
 *    zq of the cell's plane at the cell's four corners over those with a model label.  Sums start at 0, minima at 2^31 - 1.
 *    On the host a building gets no solid if filled = 0 ("no_plane"), else if it has no finite dtm ("no_terrain"), else if
 *    base >= roof_min ("base_not_below_roof"); the model labels of these buildings' cells are set to 0 by a look-up.
 * 4. Boundary runs (_lod2_count, _lod2_runs).  Horizontal line k (0 .. H) lies between the rows k - 1 and k and has the edges
 *    pos = 0 .. W - 1 from corner (k, pos) to (k, pos + 1); vertical line k (0 .. W) lies between the columns k - 1 and k and has
 *    the edges pos = 0 .. H - 1 from corner (pos, k) to (pos + 1, k).  A label outside the grid is 0 (outside).  Lines run east
 *    and south; L is the label on the left of that direction, R on the right: horizontal L = m(k - 1, pos), R = m(k, pos);
 *    vertical L = m(pos, k), R = m(pos, k - 1).  An edge is a BOUNDARY edge iff L != R.  A RUN is a maximal sequence of
 *    consecutive boundary edges of one line with the same (L, R).  One record of ADAMVS_LOD2_FIELDS int32 per run:
 *    orientation (0 horizontal, 1 vertical), line, start, end (the positions of its first and last corner: its edges are
 *    start .. end - 1), L, R, zL_s, zL_e, zR_s, zR_e: the heights of the two sides at the start and the end corner.  The height
 *    of side q > 0 is zq of plane q at that corner; the height of side 0 is plane_base[q' - 1] of the other side q' (the base of
 *    bld(q'): the caller's table).  records int32 [ADAMVS_LOD2_FIELDS][N] in ascending order of (orientation, line, start).
 * 5. Faces (host, exact integers): ada-mvs_amd/lod2.py faces().  Vertices are (1024 c, 1024 (H - r), z).  A run from S to E with
 *    d = zL - zR at either end: d_s = d_e = 0 no wall; d_s d_e >= 0 one vertical polygon S_R E_R E_L S_L (repeated vertices
 *    dropped), which faces the lower side; d_s d_e < 0 two triangles S_R X S_L and X E_R E_L with X at t = d_s / (d_s - d_e)
 *    along the run, position and height (zL_s + t (zL_e - zL_s)) each rounded half up, the same X in the roof rings of both
 *    sides.  On the vertical edges at S and E every other height of that corner (the side heights of all runs that end there)
 *    strictly inside is a vertex.  One roof polygon with holes per model plane, chained from its side of its runs (S to E where
 *    it is L, E to S where it is R; at a corner with two ways on, the left turn); one ground polygon per building at base from
 *    the runs against label 0, reversed.  Roofs face up, the ground down, walls away from the higher side.
 *
 * Kernels (csrc/dsm_lod2.hip).  _lod2_fill: the rounds round0 .. round0 + rounds - 1, one launch each, round k from label[k & 1]
 * into label[(k + 1) & 1], counts[k] zeroed first, one atomic add per workgroup; the caller may read counts back between calls
 * and stop at a fixed point.  _lod2_table: integer atomics only, one set per run of equal building labels in a wave.
 * _lod2_transpose: dst [W][H] = src [H][W] transposed through LDS tiles, so that the vertical lines are rows too.  _lod2_count:
 * a workgroup takes ADAMVS_LOD2_BLOCK consecutive edges of the row-major (line, pos) order of an orientation (the horizontal
 * lines over label, the vertical ones over label_t), reads its two rows of labels coalesced and keeps the pairs with one
 * neighbour on either side in LDS; an edge is a HEAD if it is a boundary edge and the edge before it on its line is not one of
 * the same pair, a TAIL likewise towards the edge after it.  The heads of a workgroup are counted, the counts of all workgroups
 * (horizontal first) scanned; *total = N.  _lod2_runs: the same flags again; head number h writes the start half of record h,
 * and the tail that closes it writes the end half: heads and tails alternate along the order, so a tail's number is the number
 * of heads before its workgroup, less one if the workgroup's first edge continues a run, plus its rank among the workgroup's
 * tails.  A tail compaction paired with the head compaction: no lane walks along a run.  The order comes from the scan alone.
 * All buffers device memory except those of _lod2_corner_heights_host (host memory: zq[i] = the height of plane plane[i]
 * (1 .. P) at corner (row[i], col[i])); counts: uint32 [ADAMVS_LOD2_MAX_FILL]; total: uint32 [1]; workspace of at least
 * _lod2_workspace_bytes(W, H) bytes, 256-byte aligned, the same between _lod2_count and _lod2_runs.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or > ADAMVS_LOD2_MAX_SIDE or W H > ADAMVS_DSM_MAX_CELLS,
 * z_ref not finite, B, P or N < 0, B or P > ADAMVS_DSM_MAX_CELLS (a table may be longer than the grid has cells), N above the number of lattice edges, rounds < 0, round0 < 0 or
 * round0 + rounds > ADAMVS_LOD2_MAX_FILL, workspace_bytes below the query, any two buffers overlapping; for the host entry a
 * plane number outside 1 .. P or a corner outside 0 .. 32768.  _lod2_workspace_bytes returns < 0 for a grid outside the limits. */
#define ADAMVS_LOD2_MAX_SIDE 32768
#define ADAMVS_LOD2_MAX_FILL 1024
#define ADAMVS_LOD2_Z_SCALE 1024
#define ADAMVS_LOD2_XY_SCALE 1024
#define ADAMVS_LOD2_PLANE_BITS 20      /* A, B, C are multiples of 2^-20 m */
#define ADAMVS_LOD2_Z_MAX 1073741824   /* 2^30: |zq| of every corner stays below it */
#define ADAMVS_LOD2_BLOCK 256          /* lattice edges per workgroup of _lod2_count and _lod2_runs */
#define ADAMVS_LOD2_COLUMNS 4
#define ADAMVS_LOD2_FIELDS 10
enum { ADAMVS_LOD2_CELLS = 0, ADAMVS_LOD2_FILLED = 1, ADAMVS_LOD2_BASE = 2, ADAMVS_LOD2_ROOF_MIN = 3 };
enum {
  ADAMVS_LOD2_F_ORIENTATION = 0, ADAMVS_LOD2_F_LINE = 1, ADAMVS_LOD2_F_START = 2, ADAMVS_LOD2_F_END = 3, ADAMVS_LOD2_F_L = 4,
  ADAMVS_LOD2_F_R = 5, ADAMVS_LOD2_F_ZL_S = 6, ADAMVS_LOD2_F_ZL_E = 7, ADAMVS_LOD2_F_ZR_S = 8, ADAMVS_LOD2_F_ZR_E = 9
};

long adamvs_lod2_workspace_bytes(int W, int H);
int adamvs_lod2_corner_heights_host(long P, const long long* planes, long n, const int* plane, const int* row, const int* col,
                                    long long* zq);
int adamvs_lod2_fill(int W, int H, const int* building, long P, int round0, int rounds, int* label0, int* label1, unsigned* counts,
                     void* stream);
int adamvs_lod2_table(int W, int H, const float* dtm, const int* building, const int* label, double z_ref, long B, long P,
                      const long long* planes, long long* table, void* stream);
int adamvs_lod2_transpose(int W, int H, const int* src, int* dst, void* stream);
int adamvs_lod2_count(int W, int H, const int* label, const int* label_t, long P, void* workspace, long workspace_bytes,
                      unsigned* total, void* stream);
int adamvs_lod2_runs(int W, int H, const int* label, const int* label_t, long P, const long long* planes, const int* plane_base,
                     long N, void* workspace, long workspace_bytes, int* records, void* stream);

/* ---- Trees (after the building extraction, independent of the roof planes): tree tops and their crowns from the nDSM --------
 * ada-mvs_amd/trees.py detect(); trees_whu.py is the CLI.  Inputs: ndsm [H][W] fp32 as dtm_whu.py writes it (NaN where there is
 * no value) and building [H][W] int32 (0 = none, the label raster of buildings_whu.py; a null pointer excludes nothing).  Outside
 * the buildings the nDSM is a canopy height model.  W H <= ADAMVS_DSM_MAX_CELLS.  A cell is c = (i, j), its index i W + j.  The
 * variable-window local-maximum filter (Popescu & Wynne 2004) and the marker-controlled crown growth with a height ratio and a
 * radius limit (Dalponte & Coomes 2016), restated without a visiting order.  Every comparison below is on integers unless it
 * says fp64.
 *
 * 1. Canopy.  C(c) iff ndsm(c) is finite, (double)ndsm(c) >= min_height (fp64, inclusive) and building(c) == 0.
 *    q(c) = llrint(min((double)ndsm(c), 2047.0) * 256.0) on C (1 / ADAMVS_TREE_Q_SCALE m, round to nearest, ties to even); 0 outside C.
 *    mask uint8 [H][W] is 1 on C, 0 elsewhere.
 * 2. Smoothed surface s, int32 [H][W]; -1 outside C, where it is not defined.  s_0 = q; each of the smooth_passes (0 .. 2) passes
 *    applies the 3 x 3 binomial weights w = (1 2 1) x (1 2 1) without a division:
 *      s_k+1(c) = sum over d in {-1, 0, 1}^2 of w(d) (C(c + d) ? s_k(c + d) : s_k(c)),
 *    a neighbour outside the grid or outside C contributing the centre's value.  s is q scaled by 16^passes: at most 2^27.
 *    s_max = the largest s on C, -1 if C is empty.
 * 3. Order.  c BEATS c' iff s(c) > s(c'), or s(c) == s(c') and index(c) < index(c').  A strict total order on C: plateaus need
 *    no special case.
 * 4. Window.  The caller passes an ascending table thr[1 .. r_cap] (int32, thr[1] = 0, 1 <= r_cap <= ADAMVS_TREE_MAX_RADIUS;
 *    the C argument points at thr[1]).  r(c) = the largest r with s(c) >= thr[r].  ada-mvs_amd/trees.py window_table() builds it
 *    in exact rational arithmetic: thr[r] is the smallest integer s with
 *    floor((radius_min + radius_slope s / (256 16^passes)) / gsd) >= r, clamped below at 1; r_cap is that radius at s_max.
 *    The window of c is the disc {c' in C : (i' - i)^2 + (j' - j)^2 <= r(c)^2}, clipped at the grid.
 * 5. Tops.  c in C is a TOP iff no cell of its window and none of its eight neighbours beats it (from r = 2 on the window
 *    contains the eight neighbours; the disc of r = 1 lacks the diagonal ones).
 * 6. Parents, int32 [H][W], -1 outside C.  b(c) = the best (in the order of 3) of the up to eight neighbours of c in C.  If b(c)
 *    exists and beats c: parent(c) = b(c).  Otherwise, if c is a top: parent(c) = c.  Otherwise parent(c) = the best cell of
 *    c's window, which beats c because c is no top.  Every parent other than a root beats its child, so the parents form a
 *    forest whose roots are exactly the tops; neither depends on a visiting order.
 * 7. Roots, int32 [H][W]: root(c) = the top reached from c, -1 outside C (a parent outside 0 .. W H - 1 counts as -1), by
 *    pointer jumping: round k writes, for every cell, next(c) = the cell ADAMVS_TREE_JUMP_HOPS parents up from c in the
 *    previous round's buffer (a root is its own parent, so the walk stays there).  The distance to the root falls to an
 *    eighth per round; at most ADAMVS_TREE_MAX_ROUNDS rounds, more is an error return (ADAMVS_TREE_NOT_CONVERGED), never a
 *    longer loop.  stats.rounds = the rounds that moved a pointer.
 * 8. Crowns.  The tops are numbered 1 .. T in ascending cell index (the caller scans the cells with root == own index into
 *    number int32 [H][W], read at the tops only).  With t = root(c): label(c) = number(t) iff
 *      (int64) s(c) 1000 >= ratio_pm s(t),  ratio_pm = round-half-even(crown_ratio 1000) in 0 .. 1000, and
 *      (i - i_t)^2 + (j - j_t)^2 <= rc2,    rc2 = floor((max_crown_radius / gsd)^2) >= 0, computed exactly by the caller;
 *    otherwise label(c) = 0, and the cells of C that fail a test are counted (unassigned, one int64).  A top always carries
 *    its own label.  A crown may consist of several 4-connected parts (the 8-neighbour ascent, the jump at a minor maximum and
 *    the radius test can each split it); trees.py reports the number per tree and hides nothing.
 * 9. Table, int64 [ADAMVS_TREE_COLUMNS][T], row k - 1 for label k, over the cells with 1 <= label <= T and a root inside the
 *    grid: cells; q_sum, q_max (of the unsmoothed q); row_min, row_max, col_min, col_max; r2_max (the largest squared cell
 *    distance to the top); top (the cell index of root(c)); s_top (s there).  A label without a cell: sums 0, minima
 *    2^31 - 1, maxima -1.  Integer sums, minima and maxima only.
 * 10. Selection and vectorising run on the host (ada-mvs_amd/trees.py select(), crown_polygons()).
 *
 * Kernels (csrc/dsm_trees.hip, whose head gives the reasons).  _tree_surface: the mask pass and one pass per smoothing round,
 * neighbours read straight from global memory; the last pass reduces s_max.  _tree_parents: one workgroup per tile of
 * ADAMVS_TREE_TILE^2 cells stages s with a one-cell halo in LDS, settles every cell that a neighbour beats, compacts the others
 * (the 8-neighbour local maxima) into an LDS list by wave ballot, and then sweeps one candidate's disc per wave, 64 cells of
 * its bounding box at a time, the disc rows read from L2, the best key reduced by shuffles.  _tree_roots: plain double-buffered
 * jumping, ADAMVS_TREE_JUMP_HOPS parents per round, 12 bytes per cell and round plus the later hops' gathers (the variant that first resolves every cell to its tile exit in LDS was not built); the
 * changed words of four rounds are read back together, and the loop stops at the first round that changed nothing.
 * _tree_table: the lanes of a wave that follow one another in a row with the same label are summed in registers and one lane
 * issues the atomics of the run.  No floating-point atomic, no floating-point sum: every output is bit-identical from run to
 * run.  No workgroup waits on another; visibility between rounds comes from the kernel boundaries.
 * _tree_parents and _tree_roots block and fill their own fields of stats (a HOST pointer, as is thr); the others do not block.
 * Everything else is device memory (s_max: one int32, unassigned: one int64); workspace of at least
 * _tree_workspace_bytes(W, H) bytes (about 8 bytes per cell), 256-byte aligned.
 * Argument errors (<0, before any launch): a null pointer other than building, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS,
 * min_height not finite or <= 0, smooth_passes outside 0 .. 2, r_cap outside 1 .. ADAMVS_TREE_MAX_RADIUS, a thr that does not
 * ascend from 0, ratio_pm outside 0 .. 1000, rc2 < 0, T < 0 or T > W H, workspace_bytes below the query, any two of the
 * buffers (workspace included) overlapping.  _tree_workspace_bytes returns < 0 for a grid outside the limits. */
#define ADAMVS_TREE_TILE 64        /* cells of a side of a tile of _tree_parents: a wave takes a row */
#define ADAMVS_TREE_MAX_RADIUS 64  /* largest window radius, cells */
#define ADAMVS_TREE_MAX_ROUNDS 32  /* cap on the rounds of pointer jumping: 2^28 cells need 11 */
#define ADAMVS_TREE_JUMP_HOPS 8    /* parents followed per cell and round of pointer jumping */
#define ADAMVS_TREE_NOT_CONVERGED (-2)
#define ADAMVS_TREE_Q_SCALE 256    /* ADAMVS_ROOF_Q_SCALE */
#define ADAMVS_TREE_COLUMNS 10
enum {
  ADAMVS_TREE_CELLS = 0, ADAMVS_TREE_Q_SUM = 1, ADAMVS_TREE_Q_MAX = 2, ADAMVS_TREE_ROW_MIN = 3, ADAMVS_TREE_ROW_MAX = 4,
  ADAMVS_TREE_COL_MIN = 5, ADAMVS_TREE_COL_MAX = 6, ADAMVS_TREE_R2_MAX = 7, ADAMVS_TREE_TOP = 8, ADAMVS_TREE_S_TOP = 9
};

typedef struct {
  int rounds;        /* _tree_roots: rounds of jumping that moved a pointer (< ADAMVS_TREE_MAX_ROUNDS) */
  int converged;     /* _tree_roots: 1 unless the cap was hit */
  long tops;         /* _tree_roots: cells with parent == own index */
  long candidates;   /* _tree_parents: 8-neighbour local maxima whose window was searched */
  long window_cells; /* _tree_parents: cells of those windows read (inside the disc and the grid) */
  float ms_parents;  /* _tree_parents: device time of the kernel in milliseconds; -1 if the events failed */
  float ms_jump;     /* _tree_roots: device time of the rounds, their read-backs included */
} adamvs_tree_stats;

long adamvs_tree_workspace_bytes(int W, int H);
int adamvs_tree_surface(int W, int H, const float* ndsm, const int* building, double min_height, int smooth_passes, void* workspace,
                        long workspace_bytes, unsigned char* mask, int* q, int* s, int* s_max, void* stream);
int adamvs_tree_parents(int W, int H, const int* s, int r_cap, const int* thr, void* workspace, long workspace_bytes, int* parent,
                        adamvs_tree_stats* stats, void* stream);
int adamvs_tree_roots(int W, int H, const int* parent, void* workspace, long workspace_bytes, int* root, adamvs_tree_stats* stats,
                      void* stream);
int adamvs_tree_crowns(int W, int H, const int* s, const int* root, const int* number, int ratio_pm, long rc2, int* label,
                       long long* unassigned, void* stream);
int adamvs_tree_table(int W, int H, const int* label, const int* q, const int* s, const int* root, long T, long long* table,
                      void* stream);

/* ---- Contours (after the ground filter, independent of the object stages): contour lines of a height raster as ordered
 * polylines ---------------------------------------------------------------------------------------------------------------------
 * ada-mvs_amd/contours.py trace(); contours_whu.py is the CLI.  Input: z [H][W] fp32 (the DTM as dtm_whu.py writes it, or any
 * other height raster of the grid; NaN where there is no value).  W H <= ADAMVS_DSM_MAX_CELLS.  Marching squares and "follow
 * the line from cell to cell", restated without a visiting order.  Samples sit at cell centres: cell (i, j) is at
 * (x0 + (j + 0.5) gsd, y_top - (i + 0.5) gsd).  A BLOCK (i, j), 0 <= i < H - 1, 0 <= j < W - 1, is the square between the four
 * samples A = (i, j), B = (i, j + 1), C = (i + 1, j + 1), D = (i + 1, j); its index is i W + j (the index of A: the cells of the
 * last row and column head no block); its edges are 0 = AB, 1 = BC, 2 = CD, 3 = DA.  A grid edge has the code 2 (i W + j) + d,
 * from sample (i, j) to its east (d = 0) or south (d = 1) neighbour.  Every comparison below is on integers.
 *
 * 1. Surface.  V(c) iff z(c) is finite and |(double) z(c) - z_ref| <= 8191.0.  On V: q(c) = llrint(((double) z(c) - z_ref) *
 *    256.0) (ties to even); s = q after smooth_passes (0 .. 2) passes of the 3 x 3 binomial weights (1 2 1) x (1 2 1) without
 *    a division, a neighbour outside the grid or outside V contributing the centre's value (the rule of Trees step 2), so s is
 *    the height in units of 1 / S, S = 256 16^passes, |s| < 2^30.  s = INT32_MIN outside V (heights may be negative).
 *    info int32 [3] = s_min, s_max over V (INT32_MAX, INT32_MIN if V is empty), the finite cells that failed the range test
 *    (the caller treats any as an error).
 * 2. Levels.  lev[0 .. K - 1], int32, strictly ascending, 0 <= K <= ADAMVS_CONTOUR_MAX_LEVELS, a HOST pointer.
 *    contours.level_table() builds it in exact rationals: round-half-even((base + n interval - z_ref) S) for every integer n
 *    whose level lies inside [z_ref + s_min / S, z_ref + s_max / S].  A sample is UP at level k iff s >= lev[k].
 * 3. Segments.  A block with all four samples in V is crossed by exactly the levels with min(corners) < lev[k] <= max(corners),
 *    one contiguous range of the table.  At such a level walk the corners A, B, C, D, A: an edge from a down corner to an up
 *    corner is an ENTRY, from an up corner to a down corner an EXIT; there are one or two of each.  One entry, one exit: one
 *    segment.  Two entries (the saddle; its levels are a contiguous sub-range): the centre is up iff
 *    2 (sA + sB + sC + sD) >= 4 (2 lev[k] - 1) (int64); centre up: each entry e pairs with the exit (e - 1) mod 4 (the two down
 *    corners are cut off); centre down: with the exit (e + 1) mod 4.  A segment runs from its entry crossing to its exit
 *    crossing: the higher ground is on its left in world coordinates, a ring round a summit runs counter-clockwise, a ring
 *    round a pit clockwise.  A block with a sample outside V has no segment: lines end there and at the border of the grid.
 *    count int32 [H][W]: the segments per block (0 in the last row and column).
 * 4. Numbering.  Segments are numbered 0 .. N - 1 by (block index, level k, entry edge), ascending.  N + (number of lines)
 *    < 2^31, else the error return ADAMVS_CONTOUR_TOO_MANY.
 * 5. Links.  A crossing is the pair (grid edge code, k).  seg_entry, seg_exit (edge codes), seg_level (k), int32 [N] each.
 *    succ(n) = the segment whose entry crossing is n's exit crossing, pred its inverse, -1 where there is none.  Each crossing
 *    is the exit of at most one segment and the entry of at most one, shared by the two blocks on its edge, which see the edge
 *    in opposite senses: the segments form disjoint open chains and rings.
 * 6. Lines.  An open chain starts at its segment without a pred, a ring at its smallest-numbered segment.  start(n) int32 = the
 *    start of n's line, rank(n) int32 = the succ steps from start(n) to n, closed(n) uint8 = whether the line is a ring.  Lines
 *    are numbered 0 .. M - 1 by ascending start.  Line m has len(m) + 1 vertices: the entry crossings of its segments in rank
 *    order, then the exit crossing of the last one (for a ring the first vertex again).
 * 7. Vertices.  vertex int64 [N + M][3] = (edge code, num, den): with a = s at the edge's sample (i, j) and b = s at its east or
 *    south neighbour, num / den = (2 lev[k] - 1 - 2 a) / (2 b - 2 a), normalised to den > 0, not reduced; 0 < num < den.  The
 *    half unit keeps every crossing strictly inside its edge: no two segments share a vertex by accident, and a plateau
 *    exactly at a level produces nothing.  line_first int64 [M + 1] (vertex offsets, line_first[M] = N + M), line_start int32
 *    [M], line_level int32 [M] (k), line_closed uint8 [M].
 * 8. The host (contours.py) turns t = num / den into x = x0 + (j + 0.5 + (d == 0 ? t : 0)) gsd, y = y_top - (i + 0.5 +
 *    (d == 1 ? t : 0)) gsd in fp64, sums the lengths, drops the short lines and writes the rest ordered by (level, line).
 *
 * The split into calls (csrc/dsm_contours.hip, whose head gives the reasons).  _contour_surface: the quantise pass and one pass
 * per smoothing round; the out-of-range count and the range are reduced per workgroup before one atomic each.  _contour_count: one
 * workgroup per tile of ADAMVS_CONTOUR_TILE^2 blocks stages its 65 x 65 samples and the level table in LDS; per block two
 * binary searches give the level range and two more the saddle sub-range, the count is the sum of the two lengths; then the scan
 * over the blocks (workgroup scans, k_fusion_scan over their totals, an add pass; the total also in 64 bits).  It blocks and
 * returns N in stats.segments; the offsets stay in the workspace, which _contour_segments must be given unchanged.
 * _contour_segments: one lane per SEGMENT (this is how (block, level) pairs are spread over the lanes: a cliff is many lanes,
 * not one lane's loop); the lane finds its block by a binary search in the offsets, its level and entry from the two ranges,
 * and the numbers of succ and pred in closed form from the neighbouring block's four samples (re-read from L2; no tile in LDS
 * here): the neighbour's offset + the levels of its range below k + its saddle levels below k + the entry order inside a
 * saddle.  No sort, no hash, no atomic.  _contour_rank: list ranking by pointer doubling over pred, double-buffered, one kernel
 * per round, a pair (ancestor, value) per segment.  Phase 1 carries the smallest number seen; a head marks what reaches it as
 * arrived.  It stops after a round without an arrival that lowered no minimum of a segment not yet arrived.  (While an open
 * chain has such segments every round brings arrivals.  In a ring the window of every segment has the same length w >= the
 * spacing gcd(w, L) of the ancestors' orbit; if no minimum fell, the minimum is constant along every orbit, and the windows of
 * an orbit cover the ring: it is the ring's minimum.)  The rings are cut at their minimum; phase 2 carries the distance.  Each
 * phase moves for at most ceil(log2 N) rounds and is given ADAMVS_CONTOUR_MAX_ROUNDS / 2; more is the error return
 * ADAMVS_CONTOUR_NOT_CONVERGED, never a longer loop.  The changed words of four rounds are read back together; the result does
 * not depend on where the loop stops.  It blocks and returns M in stats.lines.  _contour_lines: flags of the starts, their scan
 * into line numbers, the tails scatter the vertex counts and the line table, the scan into line_first, every segment stores its
 * entry vertex at line_first[line] + rank and the tail also its exit vertex.  It blocks.  Integer atomics only and one owner
 * per stored word: every output is bit-identical from run to run.  No workgroup waits on another.
 * Everything is device memory except lev and stats; workspaces of at least _contour_workspace_bytes(W, H) (surface, count,
 * segments: about 12 bytes per cell) and _contour_rank_workspace_bytes(N) (rank, lines: about 20 bytes per segment), 256-byte
 * aligned.  With N = 0 (no level, no block: W == 1 or H == 1) every call succeeds and the arrays of length N or M may be null.
 * Argument errors (<0, before any launch): a null pointer, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, z_ref not finite,
 * smooth_passes outside 0 .. 2, K outside 0 .. ADAMVS_CONTOUR_MAX_LEVELS, a table that does not strictly ascend, N outside
 * 0 .. 2^31 - 1, M outside 0 .. N or zero with N > 0 or N + M >= 2^31, workspace_bytes below the query, any two of the buffers
 * (workspace included) overlapping; after the read-back of one word, an N or M that is not the one the offsets or the starts
 * give.  The two queries return < 0 outside the limits. */
#define ADAMVS_CONTOUR_TILE 64           /* blocks of a side of a tile of _contour_count: a wave takes a row */
#define ADAMVS_CONTOUR_MAX_LEVELS 4096   /* entries of the level table: 16 KB of LDS */
#define ADAMVS_CONTOUR_MAX_ROUNDS 64     /* cap on the rounds of list ranking, both phases together */
#define ADAMVS_CONTOUR_Q_SCALE 256       /* ADAMVS_TREE_Q_SCALE */
#define ADAMVS_CONTOUR_MAX_ABS_M 8191    /* |z - z_ref| of a cell of V, metres */
#define ADAMVS_CONTOUR_NOT_CONVERGED (-2)
#define ADAMVS_CONTOUR_TOO_MANY (-3)

typedef struct {
  int rounds;        /* _contour_rank: rounds of both phases that changed a pair */
  int rounds_min;    /* _contour_rank: those of phase 1 (heads and ring minima) */
  int rounds_dist;   /* _contour_rank: those of phase 2 (distances) */
  int launched;      /* _contour_rank: rounds launched (whole chunks of four per phase) */
  int converged;     /* _contour_rank: 1 unless a phase hit its cap */
  int reserved;
  long segments;     /* _contour_count: N */
  long lines;        /* _contour_rank: M */
  float ms_count;    /* _contour_count: device time of the count and the scan in milliseconds; -1 if the events failed */
  float ms_rank;     /* _contour_rank: device time of both phases, their read-backs included */
} adamvs_contour_stats;

long adamvs_contour_workspace_bytes(int W, int H);
long adamvs_contour_rank_workspace_bytes(long N);
int adamvs_contour_surface(int W, int H, const float* z, double z_ref, int smooth_passes, void* workspace, long workspace_bytes, int* s,
                           int* info, void* stream);
int adamvs_contour_count(int W, int H, const int* s, int K, const int* lev, void* workspace, long workspace_bytes, int* count,
                         adamvs_contour_stats* stats, void* stream);
int adamvs_contour_segments(int W, int H, const int* s, int K, const int* lev, long N, void* workspace, long workspace_bytes,
                            int* seg_entry, int* seg_exit, int* seg_level, int* succ, int* pred, void* stream);
int adamvs_contour_rank(long N, const int* pred, void* workspace, long workspace_bytes, int* start, int* rank, unsigned char* closed,
                        adamvs_contour_stats* stats, void* stream);
int adamvs_contour_lines(int W, int H, const int* s, int K, const int* lev, long N, long M, const int* seg_entry, const int* seg_exit,
                         const int* seg_level, const int* succ, const int* start, const int* rank, const unsigned char* closed,
                         void* workspace, long workspace_bytes, long long* line_first, int* line_start, int* line_level,
                         unsigned char* line_closed, long long* vertex, void* stream);

/* ---- Drainage (after the ground filter, next to the contours): the depression-free surface, D8 flow directions, flow
 * accumulation, catchments and the stream links of a height raster ------------------------------------------------------------
 * ada-mvs_amd/drainage.py route(); drainage_whu.py is the CLI.  Input: the surface s of _contour_surface (step 1 of Contours:
 * the heights above z_ref in 1 / (256 16^passes) m, INT32_MIN outside V, refused beyond 8191 m).  W H <= ADAMVS_DSM_MAX_CELLS
 * (< 2^30).  A cell is c = (i, j), its index i W + j, rows running south.  The eight neighbours in the order of the tie rule, with
 * their ESRI codes: E 1, SE 2, S 4, SW 8, W 16, NW 32, N 64, NE 128.  Priority-flood, the topological walk of the accumulation and
 * "follow the stream", restated without a visiting order.  Every step is on integers.
 *
 * 1. Routing surface.  r(c) = s(c) 2^(8 - 4 passes) on V: ADAMVS_DRAIN_UNITS = 65536 units per metre whatever the smoothing,
 *    |r| < 2^29; INT32_MIN outside V.
 * 2. Edge cells.  A cell of V is an EDGE cell iff it lies in the first or last row or column or one of its eight neighbours is
 *    outside V.  Edge cells are the outlets.  Every other cell of V has eight neighbours in V.
 * 3. Fill.  F int32 [H][W]: F = r at the edge cells, INT32_MIN outside V, and at every other cell of V
 *    F(c) = max(r(c), min over the eight neighbours n of F(n) + 1): one unit per step, so no flat survives and every such cell
 *    has a neighbour with a smaller F.  The solution is unique (induct over the cells in ascending F) and equals priority-flood
 *    with an epsilon of one unit.  |F| < 2^30.
 * 4. Directions.  dir uint8 [H][W]: 255 outside V, 0 at an edge cell; elsewhere the code of the neighbour with the steepest
 *    positive drop d = F(c) - F(n), an orthogonal drop a against a diagonal drop b compared as 2 a^2 against b^2 in int64, ties
 *    to the first neighbour in the order above.  The RECEIVER of c is that neighbour.  F falls strictly along receivers: a forest
 *    rooted at the edge cells.
 * 5. Accumulation.  acc int32 [H][W]: acc(c) = the sum of value over the cells whose path along the receivers passes through c, c
 *    included; value = 1 on V for a null pointer (the cell count), and with value = "a stream cell without a stream donor" the
 *    Shreve magnitude.  0 outside V.  root int32 [H][W]: the outlet that c's path ends at, -1 outside V.
 * 6. Streams.  The stream cells are the cells of V with acc >= min_cells; the receiver of a stream cell is one.  nd uint8 [H][W]:
 *    the stream cells among the eight neighbours whose receiver is c, 255 where c is no stream cell.  HEADS are the stream cells
 *    with nd != 1: sources and junctions.  A head with a receiver heads a LINK: itself, the stream cells with nd = 1 below it (its
 *    OWN cells, one chain along the receivers) and, as the last vertex, the receiver of its last own cell if that cell has one: a
 *    head again, shared with the other links that end there and the first vertex of its own link if it has a receiver.  A head
 *    that is an outlet heads no link.  Links are numbered 0 .. L - 1 by ascending head index.  link int32 [H][W]: the link that
 *    owns the cell, pos int32 [H][W]: its receiver steps below the head; -1 both where no link owns the cell.
 * 7. Link table.  link_first int32 [L + 1] (vertex offsets, link_first[L] = P), link_head, link_end (the last vertex), link_to
 *    (the link that link_end heads, -1 if none: an outlet) int32 [L]; vertex int32 [P]: the cells of link l at link_first[l] + pos
 *    and link_end after them, running downstream.  P < 2^31.
 * 8. The host (drainage.py) takes the cell centres as coordinates in fp64, the length and drop of every link, its
 *    upstream_cells (acc of its last own cell), Strahler orders in one pass over the links by ascending acc(head), numbers the
 *    outlets with acc >= min_cells 1 .. K by cell index for the basin raster, drops short links and writes the files.
 *
 * The split into calls (csrc/dsm_drainage.hip, whose head gives the reasons).  _drain_fill: r, the edge test and the start of F
 * (r at the edge cells, INT32_MAX elsewhere on V), then ROUNDS: in a round one workgroup per tile of ADAMVS_DRAIN_TILE^2 cells
 * loads its tile with a one-cell halo into LDS (34 x 34 words, 4.6 KB per workgroup), lowers its cells in place to a standstill
 * and writes back those that fell.  The sweeps race; the operator is monotone and no value is ever below the fixed point, so
 * every schedule ends at the same integers.  The schedule's bound: let t(c) = 0 at an edge cell and otherwise
 * t(c) = max(1, min over the neighbours n with F(n) < F(c) of t(n) + [n lies in another tile]).  Cell c holds F(c) after round
 * t(c) at the latest (a cell is final in the round in which a lower neighbour of its tile is, and one round after a lower
 * neighbour of another tile), so at most max t rounds change a word and round max t + 1 changes none.  It runs until a round
 * changes nothing or max_rounds have been launched and returns stats.rounds (the rounds that changed a word, <= max t),
 * stats.launched (whole chunks of four while the cap allows; one read-back of the changed words, a stream synchronise, per chunk)
 * and stats.converged; without convergence F still holds INT32_MAX or values above the fixed point and must not be used.
 * _drain_direction: one lane per cell.  _drain_accumulate: pointer doubling, a pair (2^k-th ancestor or ~root, sum over the
 * descendants nearer than 2^k) per cell, double-buffered; a round adds every pair's sum to its ancestor's with an integer atomic;
 * ceil(log2(longest path + 1)) rounds and one that moves nothing, at most 32, else (dir holds a cycle: not one of
 * _drain_direction's) the error return ADAMVS_DRAIN_NOT_A_FOREST.  It blocks.  _drain_streams: nd and the donors in closed form,
 * the scan of the link heads, list ranking upstream by the distance rounds of the contours, link and pos, the tails' vertex
 * counts and their scan.  It blocks and returns L in stats.links and P in stats.vertices; the offsets stay in the workspace,
 * which _drain_links must be given unchanged.  _drain_links: the table and the vertices, every word stored by the one cell that
 * owns it.  Integer atomics only: every output is bit-identical from run to run.  No workgroup waits on another.
 * Everything is device memory except stats; a workspace of at least _drain_workspace_bytes(W, H) (about 20 bytes per cell),
 * 256-byte aligned.  With L = 0 _drain_links succeeds and the arrays of length L or P may be null.  Argument errors (<0, before
 * any launch): a null pointer other than value, W or H <= 0 or W H > ADAMVS_DSM_MAX_CELLS, smooth_passes outside 0 .. 2,
 * max_rounds < 1, min_cells < 1, L outside 0 .. W H, P outside 2 L .. 2^31 - 1 (0 with L = 0), workspace_bytes below the query,
 * any two of the buffers (workspace included) overlapping; after the read-back of one word, a P that is not the one the offsets
 * give.  The query returns < 0 outside the limits. */
#define ADAMVS_DRAIN_TILE 32             /* cells of a side of a tile of the fill */
#define ADAMVS_DRAIN_UNITS 65536         /* units of r and F per metre */
#define ADAMVS_DRAIN_NOT_A_FOREST (-2)

typedef struct {
  int rounds;        /* rounds that changed a word (fill), moved a pair (accumulate, streams) */
  int launched;      /* rounds launched */
  int converged;     /* 1 once a round changed nothing; 0: the cap was hit */
  int reserved;
  long links;        /* _drain_streams: L */
  long vertices;     /* _drain_streams: P */
  float ms;          /* device time of the call in milliseconds, its read-backs included; -1 if the events failed */
  float reserved2;
} adamvs_drain_stats;

long adamvs_drain_workspace_bytes(int W, int H);
int adamvs_drain_fill(int W, int H, const int* s, int smooth_passes, int max_rounds, void* workspace, long workspace_bytes, int* r, int* F,
                      adamvs_drain_stats* stats, void* stream);
int adamvs_drain_direction(int W, int H, const int* F, unsigned char* dir, void* stream);
int adamvs_drain_accumulate(int W, int H, const unsigned char* dir, const int* value, void* workspace, long workspace_bytes, int* acc,
                            int* root, adamvs_drain_stats* stats, void* stream);
int adamvs_drain_streams(int W, int H, const unsigned char* dir, const int* acc, int min_cells, void* workspace, long workspace_bytes,
                         unsigned char* nd, int* link, int* pos, adamvs_drain_stats* stats, void* stream);
int adamvs_drain_links(int W, int H, const unsigned char* dir, const unsigned char* nd, const int* link, const int* pos, long L, long P,
                       void* workspace, long workspace_bytes, int* link_first, int* link_head, int* link_end, int* link_to, int* vertex,
                       void* stream);

/* ---- Solar (after the DSM and the roof planes): the horizon of every cell in K directions, the sky-view factor, the minutes of
 * sun and the direct-beam energy per cell and per roof plane ------------------------------------------------------------------
 * ada-mvs_amd/solar.py expose(); solar_whu.py is the CLI.  Input: the surface s of _contour_surface with 0 smoothing passes
 * (step 1 of Contours: the heights above z_ref in 1 / 256 m, INT32_MIN outside V, refused beyond 8191 m).
 * W H <= ADAMVS_DSM_MAX_CELLS, W and H <= ADAMVS_SOLAR_MAX_SIDE.  A cell is c = (i, j), its index i W + j, rows running south.
 * r.horizon's ray march and r.sun's sums, restated without a visiting order.  Every comparison of the horizon is on integers.
 *
 * 1. Surface.  s as above: |s| <= 8191 * 256 < 2^21.
 * 2. Directions.  K is 8, 16 or 32.  The direction set is every (di, dj) with gcd(|di|, |dj|) = 1 and max(|di|, |dj|) <= 1, 2, 3
 *    respectively, sorted by the azimuth az = atan2(dj, -di) mod 2 pi (clockwise from north), ascending: k = 0 is north, (-1, 0).
 *    The tables are the literals ADAMVS_SOLAR_DIRS_8, _16, _32 below.  len2_k = di^2 + dj^2.  The sector weight w_k is half the
 *    angular gap to each cyclic neighbour divided by 2 pi; the weights sum to 1; the host computes them in fp64 and passes them
 *    (weight[K], a HOST pointer, every one finite and > 0).  The sector of an azimuth is the k at the smallest angular distance,
 *    a tie going to the smaller k.
 * 3. Horizon.  hz_n, hz_h int32 [K][H][W].  For a cell c of V and direction k look at the cells c + n (di, dj), n = 1, 2, ..,
 *    while they stay inside the raster; keep those in V with h_n = s(c + n d) - s(c) > 0; among them maximise h_n / n, comparing
 *    h_a n_b against h_b n_a in int64, a tie going to the smallest n.  hz_n = n*, hz_h = h_{n*}; both 0 if no cell qualifies
 *    and 0 outside V.  Cells outside V are transparent: they neither occlude nor get a result.  The ray is bounded by the raster
 *    only.
 * 4. Sky-view factor.  svf fp64 [H][W], q = (256 gsd)^2 an fp64 scalar of the host.  acc = 0.0; for k ascending: t = 1.0 if
 *    hz_h = 0, else L2 = ((double) n * (double) n) * ((double) len2_k * q) and t = L2 / (L2 + (double) h * (double) h);
 *    acc = acc + w_k * t.  Without fp contraction every operation is one correctly rounded fp64 +, * or /: a loop in the same
 *    order on the host gives the same bits.  0.0 outside V.  This is 1 - mean(sin^2 horizon), the isotropic sky seen by a
 *    horizontal surface.
 * 5. Exposure.  A sample table of 0 <= T <= ADAMVS_SOLAR_MAX_SAMPLES rows, HOST pointers: sector[T] (k_t, ascending), thr[T]
 *    (fp64, finite, >= 0: tan(elevation) sqrt(len2_k) gsd 256, surface units per step), minutes_w[T] and energy_w[T] (int32,
 *    >= 0, each summing to at most 2^31 - 1), sun[T][3] (int32, round(32768 v) of the unit vector towards the sun, x east, y
 *    north, z up, every |component| <= 32768).  Optional: label int32 [H][W] with values 0 .. P and normal int32 [P + 1][3] =
 *    round(32768 n), every |component| <= 32768 (both device pointers, both or neither); label 0 and a null label pointer
 *    mean the horizontal normal (0, 0, 32768), whatever row 0 holds.  For c in V: lit_t(c) = !(hz_h > 0 && (double) hz_h >
 *    thr_t * (double) hz_n) in sector k_t (one multiply, one compare; equality counts as lit); minutes(c) = sum_t lit_t m_t;
 *    direct(c) = sum_t lit_t (((int64) e_t * min(2^30, max(0, nx sx + ny sy + nz sz))) >> 30), the dot product in int64 (the
 *    cap is passed only by the rounding of two parallel unit vectors; with it neither sum can overflow).  Both int32
 *    [H][W], 0 outside V.
 * 6. Plane table.  table int64 [3][P + 1]: the cells, the sum of minutes and the sum of direct per label over V; a null label
 *    pointer counts every cell of V under label 0.
 *
 * The split into calls (csrc/dsm_solar.hip, whose head gives the reasons).  _solar_horizon: for the look direction d the lattice
 * lines are walked along w = -d from the cells whose predecessor c - w lies outside the raster; with a = min(|di|, H) and
 * b = min(|dj|, W) there are a W + (H - a) b of them, numbered in closed form: first the a full rows on the side the lines enter
 * from (row by row, column ascending), then the first (wj > 0) or last b columns of the remaining rows.  One lane per line, the
 * lines of all K directions in one grid.  Along a line with the step counter m, cells outside V skipped, the lane keeps the upper
 * convex hull of the cells passed as a stack of (m, height), nearest on top (Dozier, Bruno and Downey 1981): at a cell of height v,
 * while the stack holds two entries and the second (m2, v2) is strictly better than the top (m1, v1), (v2 - v)(m - m1) >
 * (v1 - v)(m - m2) in int64, pop; then the top is the answer, n = m - m1 and h = v1 - v, if v1 > v and there is no occluder
 * otherwise; push (m, v).  The strict > keeps collinear points, so the nearest of equals is on top.  One refinement that changes no
 * result: if the last comparison ended in equality, the cell is collinear with the top two entries and takes the top's place
 * instead of being pushed (the old top lies between its neighbours on the hull; a later cell on their line or below it is
 * answered by the new top, one above it pops both), so a plane's stack stays at two entries.  The top
 * ADAMVS_SOLAR_STACK_WINDOW entries live in LDS; deeper ones spill to the workspace, one entry per cell of the line, and come back
 * one at a time when the window runs below two.  stats: lines, the deepest stack, the entries spilled, the device time.  It
 * blocks.  _solar_svf, _solar_expose (the table goes to the head of the workspace and is read with wave-uniform addresses; a
 * label outside 0 .. P is counted and is the error return ADAMVS_SOLAR_BAD_LABEL after one read-back; it blocks) and
 * _solar_plane_sums (the wave's label runs are summed into their first lane, which issues the integer atomics): one lane per
 * cell.  Integer atomics only and one owner per stored word: every output is bit-identical from run to run.  No workgroup waits on
 * another.  Everything is device memory except stats, weight and the sample table; a workspace of at least
 * _solar_workspace_bytes(W, H, K) for the horizon (about 8 K bytes per cell) and ADAMVS_SOLAR_HEAD_BYTES for the exposure,
 * 256-byte aligned.  Argument errors (<0, before any launch): a null pointer other than label and normal (and the table's with
 * T = 0), W or H <= 0 or above ADAMVS_SOLAR_MAX_SIDE or W H > ADAMVS_DSM_MAX_CELLS, K not 8, 16 or 32, T outside
 * 0 .. ADAMVS_SOLAR_MAX_SAMPLES, a table out of the ranges or the order of step 5, P outside 0 .. ADAMVS_DSM_MAX_CELLS, label without normal or
 * normal without label, q or a weight not finite or not > 0, workspace_bytes below the need, any two of the device buffers
 * (workspace included) overlapping.  The query returns < 0 outside the limits. */
#define ADAMVS_SOLAR_STACK_WINDOW 16     /* stack entries per line kept in LDS */
#define ADAMVS_SOLAR_MAX_SAMPLES 8192    /* rows of the sample table */
#define ADAMVS_SOLAR_MAX_SIDE 32768      /* ADAMVS_ROOF_MAX_SIDE */
#define ADAMVS_SOLAR_HEAD_BYTES 262656   /* 512 + 32 ADAMVS_SOLAR_MAX_SAMPLES: the control block and the sample table */
#define ADAMVS_SOLAR_BAD_LABEL (-2)
#define ADAMVS_SOLAR_DIRS_8 {{-1, 0}, {-1, 1}, {0, 1}, {1, 1}, {1, 0}, {1, -1}, {0, -1}, {-1, -1}}
#define ADAMVS_SOLAR_DIRS_16 {{-1, 0}, {-2, 1}, {-1, 1}, {-1, 2}, {0, 1}, {1, 2}, {1, 1}, {2, 1}, {1, 0}, {2, -1}, {1, -1}, {1, -2}, {0, -1}, {-1, -2}, {-1, -1}, {-2, -1}}
#define ADAMVS_SOLAR_DIRS_32 {{-1, 0}, {-3, 1}, {-2, 1}, {-3, 2}, {-1, 1}, {-2, 3}, {-1, 2}, {-1, 3}, {0, 1}, {1, 3}, {1, 2}, {2, 3}, {1, 1}, {3, 2}, {2, 1}, {3, 1}, {1, 0}, {3, -1}, {2, -1}, {3, -2}, {1, -1}, {2, -3}, {1, -2}, {1, -3}, {0, -1}, {-1, -3}, {-1, -2}, {-2, -3}, {-1, -1}, {-3, -2}, {-2, -1}, {-3, -1}}

typedef struct {
  long lines;        /* the lattice lines of all K directions */
  long spills;       /* stack entries written to the workspace */
  int deepest;       /* the deepest stack of a line */
  int reserved;
  float ms;          /* device time of the call in milliseconds; -1 if the events failed */
  float reserved2;
} adamvs_solar_stats;

long adamvs_solar_workspace_bytes(int W, int H, int K);
int adamvs_solar_horizon(int W, int H, int K, const int* s, void* workspace, long workspace_bytes, int* hz_n, int* hz_h,
                         adamvs_solar_stats* stats, void* stream);
int adamvs_solar_svf(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, const double* weight, double q, double* svf,
                     void* stream);
int adamvs_solar_expose(int W, int H, int K, const int* s, const int* hz_n, const int* hz_h, int T, const int* sector, const double* thr,
                        const int* minutes_w, const int* energy_w, const int* sun, const int* label, long P, const int* normal,
                        void* workspace, long workspace_bytes, int* minutes, int* direct, void* stream);
int adamvs_solar_plane_sums(int W, int H, const int* s, const int* label, long P, const int* minutes, const int* direct, long long* table,
                            void* stream);

/* ---- TSDF mesh (after fuse_whu.py): the depth maps of all views integrated into a truncated signed-distance field on a voxel
 * grid, brick by brick, and its zero level set extracted as a coloured triangle mesh ---------------------------------------
 * ada-mvs_amd/mesh.py drives it per brick; mesh_whu.py is the CLI.  World axes: x east, y north, z up.
 *
 * Volume.  Origin O (fp64, the min corner), voxel size s (fp64).  Sample g = (i, j, k) (integers >= 0) sits at O + g s.  The
 * volume is cut into bricks of B^3 cubes, B in {32, 64, 128}: brick b = (bx, by, bz) owns the cubes b B .. b B + B - 1 along
 * each axis and holds the samples b B .. b B + B (one layer shared with each upper neighbour), so every cube belongs to
 * exactly one brick.  Inside a brick, sample l = g - b B (0 <= l <= B per axis) is entry n = (l.z (B+1) + l.y)(B+1) + l.x of
 * the per-sample arrays ([(B+1)^3], "sample row-major"), and cube l (0 <= l < B) is entry (l.z B + l.y) B + l.x of the
 * per-cube arrays ([B^3], "cube row-major").  The brick: a HOST pointer to an adamvs_mesh_brick, copied into the arguments.
 *
 * Views.  One DEVICE array of adamvs_mesh_view, built once per scene from a host array that adamvs_mesh_check_views
 * accepted: K (fp32, row-major, last row 0 0 1), R_cw (fp32, row-major: world -> camera x right / y down / z forward) and
 * c = C - O (formed in fp64 by the caller, rounded to fp32), the depth map [H][W] fp32 (device) and the image [H][W][4]
 * uint8 RGBA (device).  Per brick the caller passes a DEVICE list of view indices, sorted ascending, no repeats, and
 * CONSERVATIVE: every view that projects a sample of the closed brick box (grown by mu) into its image is in it.  An index
 * outside [0, nviews) is skipped.
 * Precision: all camera-frame arithmetic is fp32 relative to O.  Cameras (|c| per axis) and bricks ((b + 1) B s per axis)
 * farther than ADAMVS_MESH_MAX_EXTENT = 16384 m from O are refused (fp32 spacing <= 2^-10 m there).  With L = |g s| + |c|
 * (Euclidean, <= 2 sqrt(3) 16384 m), each view's sdf is within 16 2^-24 L of the fp64 value of the same fp32 inputs, hence
 * |tsdf - tsdf_fp64| <= 16 2^-24 L / mu + 2^-24 (weight + 2)  (<= 0.055 m / mu + 2^-24 (weight + 2) at the limit),
 * wherever the pixel choices and the tests below decide alike (a pixel coordinate within that error of a half integer,
 * z, sdf + mu or |sdf| - mu within it of 0, may go either way).
 *
 * Integration (adamvs_tsdf_integrate): every sample g of the brick independently, the views of the list in list order, no
 * atomics.  sf = (float)s, muf = (float)mu; per view:
 *   x = (float)g sf - c (fp32),  p = R_cw x,  z = p.z;  skip the view unless z > 0;
 *   u = (K00 p.x + K01 p.y + K02 z) / z,  v = (K10 p.x + K11 p.y + K12 z) / z  (pixel centres at integer coordinates);
 *   the nearest pixel (floor(u + 0.5), floor(v + 0.5)): skip unless it lies inside the image and its depth d is finite and
 *   > 0 (depth 0 marks a pixel fusion rejected: unknown, not free space);
 *   sdf = d - z (fp32); skip if sdf < -muf;
 *   T += min(1, sdf / muf) (fp32, in list order), weight += 1;
 *   if |sdf| <= muf: the pixel's R, G, B are added to integer sums and 1 to a colour count n.
 * Outputs [(B+1)^3]: tsdf = T / (float)weight (0 where weight = 0), weight uint16 saturating at 65535, rgba uint32
 * (little-endian r g b a): per channel (sum + n / 2) / n in integers and alpha 255, 0 where n = 0.  Every step is integer or
 * in a fixed order, so a sample's value does not depend on the brick that computed it as long as the view lists are
 * conservative: the shared layers of neighbouring bricks are bit-identical.
 *
 * Extraction: marching tetrahedra on the Kuhn split.  A cube is PROCESSED iff its 8 corners have weight >= min_weight.  It
 * splits into 6 tetrahedra along its main diagonal, tet t for the axis permutation (a, b, c) =
 *   t = 0 (x y z), 1 (x z y), 2 (y x z), 3 (y z x), 4 (z x y), 5 (z y x),
 * with vertices v0 = 000, v1 = e_a, v2 = e_a + e_b, v3 = 111.  Every lattice edge a tet uses runs from a sample g in one of 7
 * positive directions, numbered  0 +x, 1 +y, 2 +z, 3 +xy, 4 +xz, 5 +yz, 6 +xyz;  a vertex is "edge e of sample g".
 * A corner is INSIDE iff tsdf < 0; the tet case is sum over k of inside(v_k) << k.  A vertex exists on an edge (g, g + e) iff
 * its two samples differ in that sign and a processed cube of the brick uses the edge.  With a = g, b = g + e:
 *   lambda = t_a / (t_a - t_b)  (fp32),  position = O + ((double)g + (double)lambda e) s  per axis, fp64, no contraction;
 *   colour = per channel rint(c_a + lambda (c_b - c_a)) in fp32 (no contraction), clamped to 0 .. 255 (a corner without
 *   colour counts as 0).
 * Triangles per tet: cases 0 and 15 give none.  A lone vertex i (one inside or one outside) gives the triangle on its edges
 * to the other three, in ascending order of those.  A 2-2 split, inside {i < j}, outside {k < l}, gives the quad
 * q0 = (i,k), q1 = (i,l), q2 = (j,l), q3 = (j,k), cut along q0 - q2 into (q0 q1 q2) and (q0 q2 q3).  Each triangle is then
 * oriented so that its right-hand normal, at lambda = 1/2 on every edge, points along (centroid of the outside corners -
 * centroid of the inside corners), i.e. toward increasing tsdf (out of the solid); if not, its last two vertices swap.
 * Output order: vertices in sample row-major order, then edge direction; triangles in cube row-major order, then tet order,
 * then the order above.  Indices are brick-local (uint32) plus a caller-given vertex_base.  A vertex on a face, edge or
 * corner layer shared with a neighbouring brick is written by each brick that uses it, at bit-identical coordinates and
 * colour: welding by exact position (mesh.py weld) merges them.
 *
 * Calls, per brick, in stream order (no inter-workgroup waits, no atomics: bit-identical from run to run).  Workgroups cover
 * ADAMVS_MESH_TILE consecutive entries: nblocks_cubes = B^3 / 256, nblocks_samples = ceil((B+1)^3 / 256).
 *   _tsdf_integrate       tsdf [(B+1)^3] fp32, weight [(B+1)^3] uint16, rgba [(B+1)^3] uint32;
 *   _mesh_classify        cube_code [B^3] uint32: bit 0 processed, bits 1 + 4 t .. 4 + 4 t the case of tet t (0 for a cube
 *                         not processed), bits 25 .. 28 its triangle count; block_tris [nblocks_cubes] uint32;
 *   _mesh_count_vertices  edge_mask [(B+1)^3] uint8 (bit e: the vertex on edge e of the sample exists); block_verts
 *                         [nblocks_samples] uint32;
 *   adamvs_fusion_scan of block_verts -> vert_offsets [nblocks_samples + 1] and of block_tris -> tri_offsets [nblocks_cubes + 1];
 *   _mesh_emit            xyz [nv][3] fp64, rgb [nv][3] uint8, first_vertex [(B+1)^3] uint32 (the brick-local index of the
 *                         sample's first vertex; its vertex on edge e is first_vertex + popcount(edge_mask & ((1 << e) - 1))),
 *                         then faces [nt][3] uint32.  Nothing is written at or past vert_capacity / tri_capacity.
 * Argument errors (<0, before any launch): a null pointer (the view list may be null when nlist = 0), B not in the set, s or
 * mu not finite or <= 0, a brick index < 0, O not finite, (b + 1) B s > ADAMVS_MESH_MAX_EXTENT, min_weight < 1 or > 65535,
 * nviews < 1 or > ADAMVS_MESH_MAX_VIEWS, nlist < 0 or > nviews, a capacity < 0, and in _mesh_check_views (host array) a view
 * with a null pointer, H or W < 1, a non-finite K / R_cw / c, K's last row not 0 0 1, or |c| > ADAMVS_MESH_MAX_EXTENT. */
#define ADAMVS_MESH_TILE 256
#define ADAMVS_MESH_MAX_VIEWS 65535
#define ADAMVS_MESH_MAX_EXTENT 16384.0

typedef struct {
  float K[9];
  float R[9];
  float c[3];
  int H, W;
  const float* depth;
  const unsigned char* rgba;
} adamvs_mesh_view;

typedef struct {
  double origin[3];
  double voxel, mu;
  int B, bx, by, bz;
  int min_weight;
} adamvs_mesh_brick;

int adamvs_mesh_check_views(const adamvs_mesh_view* views, int nviews);
int adamvs_tsdf_integrate(const adamvs_mesh_brick* brick, const adamvs_mesh_view* views, int nviews, const int* view_list, int nlist,
                          float* tsdf, unsigned short* weight, unsigned* rgba, void* stream);
int adamvs_mesh_classify(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned short* weight, unsigned* cube_code,
                         unsigned* block_tris, void* stream);
int adamvs_mesh_count_vertices(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned* cube_code, unsigned char* edge_mask,
                               unsigned* block_verts, void* stream);
int adamvs_mesh_emit(const adamvs_mesh_brick* brick, const float* tsdf, const unsigned* rgba, const unsigned* cube_code,
                     const unsigned char* edge_mask, const unsigned* vert_offsets, const unsigned* tri_offsets, unsigned vertex_base,
                     double* xyz, unsigned char* rgb, unsigned* first_vertex, long vert_capacity, unsigned* faces, long tri_capacity,
                     void* stream);

/* ---- Mesh simplification (after mesh_whu.py): vertex clustering on a lattice, one Garland-Heckbert quadric per cell ---------
 * (Lindstrom's out-of-core simplification.)  ada-mvs_amd/simplify.py drives it; simplify_whu.py is the CLI.  It welds the mesh
 * by exact position first (mesh.py weld), always, so the result does not depend on the brick size or on --weld.
 *
 * Inputs: vertices xyz [nv][3] fp64 world, rgb [nv][3] uint8, faces [nf][3] uint32, the cell size c > 0 in metres, the lattice
 * origin O (fp64, O <= min xyz per axis) and rank_eps (default 1e-3).  All arithmetic below is fp64 without contraction.
 *
 * 1. Cell of a vertex.  Per axis i = floor((x - O) / c); key = iz << 42 | iy << 21 | ix (ADAMVS_SIMPLIFY_KEY_BITS = 21 bits per
 *    axis).  A non-finite coordinate is error code 1, an index < 0 or >= 2^21 error code 2 (never a clamp); the key of such a
 *    vertex is -1.  The distinct keys in ascending order are the CELLS 0 .. nc - 1; the centre of a cell is O + (i + 0.5) c.
 * 2. Quadric of a cell: over every face with at least one corner in the cell, once per face and cell even where two or three
 *    corners share it, and whether or not the face survives step 5.  With the face's corners relative to the cell centre,
 *    p0, p1, p2:  u = p1 - p0, w = p2 - p0, n = u x w = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0)  (not normalised: a face
 *    weighs its area squared),  d = -(n0 p0.x + n1 p0.y + n2 p0.z);  A += n n^T, b += d n, and sum d^2 for the reported error.
 *    The sums do not feel the sign of n, so the order of a face's corners is free: the driver takes them ascending by welded
 *    vertex number (a function of the positions alone) and the faces ascending by those triples, the CANONICAL face list.  The
 *    rounding of every sum is then a function of the mesh as a set, not of the order its faces were written in.
 * 3. Members: every input vertex of the cell, including one that no face references.  m = the mean of their positions relative
 *    to the centre; colour = per channel (sum + count / 2) / count in integers (half rounds up, as the tsdf's colours do).
 * 4. Representative.  lambda_k, v_k = the eigen-decomposition of the symmetric A; eigenvalue k is KEPT iff
 *    lambda_k > rank_eps lambda_max.  p = m + sum over the kept k of v_k (v_k . g) / lambda_k,  g = -(b + A m):  the minimiser of
 *    the quadric nearest to m, the same whatever basis the solver returns.  If nothing is kept, or some |p_k| > c / 2, or p is
 *    not finite, then p = m (FALLBACK): a representative always lies in its own cell.  Position = centre + p; rank = the
 *    number kept (0 .. 3); error = p.A p + 2 b.p + sum d^2.
 * 5. Faces.  A face SURVIVES iff its three corners lie in three distinct cells.  Of the surviving faces with the same set of
 *    three cells the first in input order is KEPT (thin double sheets fold onto each other); kept faces stay in input order
 *    with their orientation.
 * 6. Vertices out: the cells USED by a kept face, in ascending key order, and the kept faces with their corners renumbered.
 *    Cells that no kept face uses disappear.
 *
 * Calls, in stream order.  The caller numbers the cells (unique of the keys, ascending, with the inverse -> vcell [nv] int32),
 * runs _simplify_corners on the faces as given (fcell and survive, for steps 5 and 6) and on the canonical face list (entry_cell,
 * for step 2; _simplify_accumulate then takes that list as its faces), sorts entry_cell STABLY (-> entry [3 nf]: the indices 3 f + k in sorted order; fstart [nc + 1]: where each cell's run
 * starts, fstart[nc] = the first sentinel) and sorts the vertices stably by cell (-> vorder [nv], vstart [nc + 1]).  No atomics
 * and no inter-workgroup waits: the order of every sum is a function of these sorted inputs only, so the output is
 * bit-identical from run to run.  Workgroups cover ADAMVS_SIMPLIFY_TILE consecutive entries.
 *   _simplify_keys        keys [nv] int64, bad [nv] uint8 (the error code, 0 = fine);  origin: HOST pointer to 3 doubles;
 *   _simplify_corners     fcell [nf][3] int32 (the cells of the corners), entry_cell [nf][3] int32 (the same, with the sentinel nc
 *                         where the corner repeats an earlier corner's cell: it sorts to the end), survive [nf] uint8.  A face
 *                         with an index >= nv gets nc thrice and does not survive;
 *   _simplify_accumulate  one wave per cell: lane l takes entries l, l + 64, .. of the run in order and the 64 partial sums meet
 *                         in a fixed butterfly (xor 32, 16, .. 1).  quadric [nc][10] fp64 = A00 A01 A02 A11 A12 A22, b, sum d^2;
 *                         member [nc][3] fp64 (the sum of step 3, not yet divided), colour [nc][3] uint64 (the channel sums);
 *   _simplify_solve       one lane per cell: cyclic Jacobi, 8 sweeps of the rotations (0,1) (0,2) (1,2), then steps 3 and 4:
 *                         pos [nc][3] fp64, col [nc][3] uint8, rank [nc] uint8, fallback [nc] uint8, error [nc] fp64;
 *   _simplify_solve_host  step 4 for n cells on the HOST (host pointers, the same inline function the kernel runs; mean = m):
 *                         p [n][3] relative to the centre.  For checks of the solve on a machine without a device;
 *   _simplify_triples     surv [ns] int64: the surviving faces in ascending order -> tri [3][ns] int32, the three cells of each in
 *                         ascending order, one row per rank.  The caller sorts the faces stably and lexicographically by them
 *                         (-> order [ns] int64, indices into surv);
 *   _simplify_first       keep [nf] uint8 (zeroed by the caller): 1 for the first face of each run of equal triples;
 *   _simplify_mark        used [nc] uint8 (zeroed by the caller): plain stores of 1 at the cells of the kept faces;
 *   _simplify_count       block_count [ceil(n / 256)] uint32 of any flag array [n] uint8; adamvs_fusion_scan makes the offsets;
 *   _simplify_emit        xyz [nu][3] fp64, rgb [nu][3] uint8, new_index [nc] uint32 (written at used cells), then faces
 *                         [nk][3] uint32.  Nothing is written at or past vert_capacity / face_capacity.
 * Argument errors (<0, before any launch): a null pointer, nv, nf, nc or ns < 1 or > 2^31 - 1, nc > nv, c not finite or <= 0,
 * O not finite, rank_eps not in [0, 1), a capacity < 0. */
#define ADAMVS_SIMPLIFY_TILE 256
#define ADAMVS_SIMPLIFY_KEY_BITS 21

int adamvs_simplify_keys(const double* origin, double cell, const double* xyz, long nv, long long* keys, unsigned char* bad, void* stream);
int adamvs_simplify_corners(const unsigned* faces, long nf, const int* vcell, long nv, int nc, int* fcell, int* entry_cell,
                            unsigned char* survive, void* stream);
int adamvs_simplify_accumulate(const double* origin, double cell, const long long* keys, int nc, const double* xyz,
                               const unsigned char* rgb, long nv, const unsigned* faces, long nf, const long long* entry,
                               const long long* fstart, const long long* vorder, const long long* vstart, double* quadric,
                               double* member, unsigned long long* colour, void* stream);
int adamvs_simplify_solve(const double* origin, double cell, double rank_eps, const long long* keys, int nc, const double* quadric,
                          const double* member, const unsigned long long* colour, const long long* vstart, double* pos,
                          unsigned char* col, unsigned char* rank, unsigned char* fallback, double* error, void* stream);
int adamvs_simplify_solve_host(const double* quadric, const double* mean, long n, double cell, double rank_eps, double* p, int* rank,
                               int* fallback, double* error);
int adamvs_simplify_triples(const int* fcell, long nf, const long long* surv, long ns, int* tri, void* stream);
int adamvs_simplify_first(const int* tri, const long long* surv, const long long* order, long ns, long nf, unsigned char* keep,
                          void* stream);
int adamvs_simplify_mark(const int* fcell, const unsigned char* keep, long nf, int nc, unsigned char* used, void* stream);
int adamvs_simplify_count(const unsigned char* flags, long n, unsigned* block_count, void* stream);
int adamvs_simplify_emit(const double* pos, const unsigned char* col, const unsigned char* used, int nc, const unsigned* cell_offsets,
                         const int* fcell, const unsigned char* keep, long nf, const unsigned* face_offsets, double* xyz,
                         unsigned char* rgb, unsigned* new_index, long vert_capacity, unsigned* faces, long face_capacity, void* stream);

/* ---- Mesh smoothing (after mesh_whu.py, before simplify_whu.py): bilateral normal filtering ---------------------------------
 * (Zheng, Fu, Au, Tai, "Bilateral normal filtering for mesh denoising", the local iterative scheme.)  ada-mvs_amd/smooth.py
 * drives it; smooth_whu.py is the CLI.  It welds the mesh by exact position first (mesh.py weld), always.  Flat ground and
 * roofs flatten, creases stay; the topology is untouched.
 *
 * Inputs: vertices xyz [nv][3] fp64 world, rgb [nv][3] uint8, faces [nf][3] uint32, the origin O (fp64: the volume origin of
 * <mesh>.json, else the per-axis vertex minimum), sigma_s > 0 (metres), sigma_r > 0, normal_iters and vertex_iters in 0 .. 1000,
 * the cap > 0 (metres) and fix_boundary.  All arithmetic below is fp64 without contraction, on p = xyz - O; sqrt and the
 * divisions round correctly, exp is the device library's.  |a|^2 of a 3-vector is (a0 a0 + a1 a1) + a2 a2 everywhere.  Faces,
 * their order and the colours leave unchanged; only positions move.
 *
 * 1. Face records, from the input positions.  With the corners a, b, c:  u = b - a, w = c - a,
 *    m = u x w = (u1 w2 - u2 w1, u2 w0 - u0 w2, u0 w1 - u1 w0),  area A = |m| / 2,  normal n = m / |m|, or the zero vector when
 *    |m| = 0 (a DEGENERATE face),  centroid c = ((a + b) + c) / 3.
 * 2. Incidence.  F(v): the faces with a corner at vertex v, ascending by face number, each once.  N(f): f itself, then the
 *    faces of F(corner 0), then those of F(corner 1), then those of F(corner 2), each in order, leaving out every face that
 *    already appeared (f included; a corner that repeats an earlier corner of f adds nothing).  That order is the summation
 *    order of step 3.
 * 3. Normal filter, normal_iters times, double-buffered (every read is of the previous pass):
 *      s_f = sum over g in N(f) of  A_g exp(-(|c_f - c_g|^2 / (2 sigma_s^2) + |n_f - n_g|^2 / (2 sigma_r^2))) n_g
 *    (the product of the spatial and the range weight, as one exponential), added term by term from zero;
 *    n_f <- s_f / |s_f| if |s_f| > 1e-12, else n_f stays.  Areas and centroids stay those of step 1 throughout.
 * 4. Fixed vertices.  The edges of a face are its corner pairs (0, 1), (1, 2), (2, 0), unordered.  With fix_boundary a vertex
 *    is FIXED iff it is an end of an edge that occurs exactly once among the 3 nf edges.  An edge that occurs three or more
 *    times gets no special treatment.
 * 5. Vertex update, vertex_iters times, Jacobi (every read is of pass t, writes go to pass t + 1).  c_f^t = the centroids of
 *    the current positions.  For a vertex that is not fixed and has faces:
 *      s = sum over f in F(v), in order, of  n_f t_f,   t_f = (n_f.x e.x + n_f.y e.y) + n_f.z e.z,   e = c_f^t - x_v
 *      x' = x_v + s / |F(v)|,   d = x' - x0_v,   x_v <- x0_v + d k,   k = cap / |d| if |d| > cap (the vertex is CLAMPED), else 1.
 *    Fixed vertices and vertices without faces keep x0.
 * Output: O + p for every vertex step 5 updated; the input bits for fixed vertices, vertices without faces and every vertex when
 * vertex_iters = 0.
 *
 * Calls, in stream order.  The caller forms p, sorts the 3 nf (vertex, face) entries STABLY by vertex, entry 3 f + k carrying
 * corner k of face f, or the sentinel nv where that corner repeats an earlier corner of f (-> vface [3 nf] int32: the faces
 * in sorted order; vstart [nv + 1] int64: where each vertex's run starts, vstart[nv] = the first sentinel), and sorts the edge
 * keys.  No atomics and no inter-workgroup waits: every lane writes its own element only, the order of every sum is a function
 * of the sorted input, so the output is bit-identical from run to run.  Workgroups cover ADAMVS_SMOOTH_TILE consecutive
 * elements, one lane each.
 *   _smooth_faces       rec [nf][8] fp64, 64-byte aligned: centroid, area, normal, 0 (a face with an index >= nv: all zero);
 *   _smooth_edge_keys   keys [3 nf] int64: min << 32 | max of the corner pairs (0, 1), (1, 2), (2, 0);
 *   _smooth_boundary    keys [n] int64 SORTED; fixed [nv] uint8 (zeroed by the caller): plain stores of 1 at both ends of every
 *                       key that differs from both its neighbours;
 *   _smooth_filter      one pass of step 3: nin [nf][3] -> nout [nf][3] (nin != nout).  Whether a face already appeared is
 *                       decided by comparing its three vertex numbers with the earlier corners of f;
 *   _smooth_centroids   cen [nf][3] fp64 of the positions p [nv][3];
 *   _smooth_update      one pass of step 5: p0 (the input), p -> pout [nv][3] (distinct buffers), clamped [nv] uint8 (written
 *                       for every vertex).
 * Argument errors (<0, before any launch): a null pointer, nv < 1 or > 2^31 - 1, nf < 1 or > (2^31 - 1) / 3, a sigma or the cap
 * not finite or <= 0, rec not aligned to 64 bytes, aliased buffers. */
#define ADAMVS_SMOOTH_TILE 256

int adamvs_smooth_faces(const double* p, long nv, const unsigned* faces, long nf, double* rec, void* stream);
int adamvs_smooth_edge_keys(const unsigned* faces, long nf, long long* keys, void* stream);
int adamvs_smooth_boundary(const long long* keys, long n, long nv, unsigned char* fixed, void* stream);
int adamvs_smooth_filter(const double* rec, const double* nin, double* nout, const unsigned* faces, long nf, long nv, const int* vface,
                         const long long* vstart, double sigma_s, double sigma_r, void* stream);
int adamvs_smooth_centroids(const double* p, long nv, const unsigned* faces, long nf, double* cen, void* stream);
int adamvs_smooth_update(const double* p0, const double* p, double* pout, long nv, const double* nrm, const double* cen, long nf,
                         const int* vface, const long long* vstart, const unsigned char* fixed, double cap, unsigned char* clamped,
                         void* stream);

/* ---- Mesh cleaning (after mesh_whu.py, before smooth_whu.py): small components dropped, small holes closed --------------------
 * ada-mvs_amd/clean.py drives it; clean_whu.py is the CLI.  The zero level set of a TSDF built from predicted depth carries
 * FLOATERS (small blobs where a few consistent but wrong depths were fused) and PINHOLES (small loops of open edges where a
 * few voxels missed the weight threshold).  This step removes the first and closes the second; it moves no vertex.
 *
 * Inputs: vertices xyz [nv][3] fp64 world, rgb [nv][3] uint8, faces [nf][3] uint32, the origin O (fp64: the volume origin of
 * <mesh>.json, else the per-axis vertex minimum), min_faces >= 0, an optional min_area > 0 (square metres) and
 * max_hole_edges M in 0 .. ADAMVS_CLEAN_MAX_HOLE_EDGES.  fp64 without contraction; the divisions and sqrt round correctly.
 *
 * 1. Weld by exact position (mesh.py weld), always; positions p = xyz - O.  A vertex that is not finite is an error.
 * 2. Degenerate faces (two equal corner indices after the weld) are dropped; the rest keep their order.  nf counts the rest.
 * 3. Components.  Two faces are connected when they share a welded vertex; the LABEL of a component is the smallest welded
 *    vertex index in it.  Rounds over a label per vertex, parent[v] = v at first.  One round: with the previous round's labels
 *    r = parent[corner] of a face and m the smallest of the three, every r != m is hooked, parent'[r] = min(parent'[r], m)
 *    (parent' starts as a copy of parent; r is a root, and an integer minimum does not depend on the order, so a round's
 *    result is a function of its input); then every vertex is given the root of its tree (parent'[v] followed until it stops
 *    changing).  The rounds end with the first that hooks nothing; the labels are then the unique fixed point.  A face's
 *    label is that of its corner 0.  Per component: its face count and its AREA.  A face's area is A = |u x w| / 2 of
 *    _smooth_faces (on p).  With the faces sorted STABLY by label (so ascending face number within a component) and that
 *    sorted sequence cut into chunks of ADAMVS_CLEAN_CHUNK consecutive positions, a component's PIECES are its runs inside the
 *    chunks it meets; a piece is summed from zero in ascending position, and the area of the component is its first piece plus
 *    the others, added one by one in ascending position.  (A component of fewer faces than one chunk that lies inside one
 *    chunk is therefore the plain sum in ascending face number.)  A component is KEPT iff faces >= min_faces and, where
 *    min_area is given, area >= min_area.
 * 4. The faces of kept components are the SURVIVING faces, s = 0 .. ns - 1 in input order.  Half-edge h = 3 s + k runs from
 *    corner k (its TAIL) to corner (k + 1) % 3 (its HEAD) of surviving face s.
 * 5. Boundary.  h is a BOUNDARY half-edge iff its key min << 32 | max occurs exactly once among the 3 ns keys (three or more
 *    times: not boundary).  A vertex is SIMPLE iff exactly one boundary half-edge leaves it and exactly one enters it.
 *    succ(h), for a boundary half-edge whose head is simple, is the boundary half-edge leaving head(h); else it is undefined.
 * 6. Loops.  A LOOP is a cycle of succ all of whose vertices are simple; its label is its smallest h, its length L its number
 *    of half-edges.  A loop is CLOSED iff 3 <= L <= M.  A chain that meets a vertex that is not simple (two holes pinched at a
 *    vertex, a hole next to an edge of three faces) belongs to no loop and stays open.  Computed by pointer doubling,
 *    double-buffered, from lab = h, nxt = succ(h) (or h itself where undefined), broken = (succ undefined):
 *      lab'[h] = min(lab[h], lab[nxt[h]]),  broken'[h] = broken[h] | broken[nxt[h]],  nxt'[h] = nxt[nxt[h]].
 *    After R rounds lab[h] is the minimum over the 2^R half-edges from h on.  With fewer rounds than the longest cycle needs
 *    the labels on it are window minima, and a group of equal labels can be short by accident; so whatever R, a label group
 *    is a loop only if none of its members is broken and EVERY member satisfies lab[h] == lab[succ(h)] with the original
 *    succ: the group is then closed under an injective map, so it is a union of cycles, and as each of them contains the
 *    group's label it is one cycle.  clean.py runs R = ceil(log2(boundary half-edges)) + 1 rounds, which labels every cycle
 *    whole, so that the loops longer than M can be counted.
 * 7. Fill, for every closed loop in ascending label: one new vertex at O + s / L, s the sum of p[tail(h)] over the loop's
 *    half-edges in ascending h from zero (each axis on its own); its colour per channel floor(c / L + 0.5), c the integer sum
 *    of the tails' channel; and for every half-edge a -> b of the loop one new face (b, a, centre), so that the shared edge
 *    runs the other way in the new face and the orientation of the mesh carries over.
 * 8. Output.  Vertices: the welded vertices that a surviving face uses, in welded order, with the bits of their input position
 *    and their colour, then the fill vertices by loop label.  Faces: the surviving faces in input order, then the fill faces
 *    in ascending h.  Where fill vertices were added clean.py welds this output once more, which only moves them to their
 *    places in the lexicographic order (and merges one that lands exactly on an existing vertex into it, keeping that vertex's
 *    colour): the weld of the next step then changes nothing, and cleaning a cleaned mesh returns it bit for bit.
 *
 * Calls, in stream order; the sorts, scans and compactions between them are the caller's.  The only atomics are integer
 * atomicMin and atomicAdd on values that do not depend on the order; there is no floating-point atomic, so the output is
 * bit-identical from run to run.  Workgroups cover ADAMVS_CLEAN_TILE consecutive elements, one lane each.
 *   _clean_components  one round of step 3: parent_in [nv] int32 -> parent_out [nv] (distinct), changed [1] = whether a hook
 *                      happened.  Before the first round parent_in[v] = v;
 *   _clean_area        area [nf] fp64; order [nf] int64: the faces sorted stably by label; seg_of [nf] int64: the rank of the
 *                      component at each sorted position; seg_start [ncomp + 1] int64; lead [ceil(nf / CHUNK)] and
 *                      first [ncomp] fp64 scratch -> out [ncomp] fp64;
 *   _clean_boundary    keys_sorted, entry [3 ns] int64 (entry: the half-edge of each sorted key) -> bnd [3 ns] uint8, all written;
 *   _clean_successor   -> out_count, in_count [nv] int32, out_edge [nv] int32 (the smallest boundary half-edge leaving the
 *                      vertex, 2^31 - 1 if none), succ [3 ns] int32 (-1: undefined or off the boundary), and the initial lab,
 *                      nxt [3 ns] int32 and broken [3 ns] uint8 of step 6 (off the boundary: lab = nxt = h, broken = 1);
 *   _clean_double      one round of step 6.  Entries off the boundary are skipped: the caller initialises BOTH buffers of
 *                      lab, nxt and broken with _clean_successor's output;
 *   _clean_validate    count [3 ns] int32 (the size of each label group, at its label), bad [3 ns] uint8 -> loop [3 ns] int32
 *                      (the label of h's loop, -1 where h is in none), closed [3 ns] uint8;
 *   _clean_accumulate  members [nm] int32: the closed half-edges sorted stably by loop label (ascending h within a loop),
 *                      start [nl + 1] int64, origin: 3 fp64 on the HOST -> centre [nl][3] fp64 (world), colour [nl][3] uint8;
 *   _clean_emit        new_index [nv] int32 (-1: unused), fill_edge [nfill] int32 (the closed half-edges ascending),
 *                      loop_of [nfill] int32 (the rank of each one's loop) -> xyz_out, rgb_out [nvs + nl][3], faces_out
 *                      [ns + nfill][3] uint32.
 * Argument errors (<0, before any launch): a null pointer, nv < 1 or > 2^31 - 1, ns (nf) < 1 or > (2^31 - 1) / 3, ncomp, nl, nm,
 * nfill or nvs out of range, M outside 0 .. ADAMVS_CLEAN_MAX_HOLE_EDGES, an origin that is not finite, aliased buffers. */
#define ADAMVS_CLEAN_TILE 256
#define ADAMVS_CLEAN_CHUNK 1024
#define ADAMVS_CLEAN_MAX_HOLE_EDGES 4096
#define ADAMVS_CLEAN_MAX_ROUNDS 64

int adamvs_clean_components(const unsigned* faces, long nf, long nv, const int* parent_in, int* parent_out, unsigned* changed, void* stream);
int adamvs_clean_area(const double* area, long nf, const long long* order, const long long* seg_of, const long long* seg_start, long ncomp,
                      double* lead, double* first, double* out, void* stream);
int adamvs_clean_boundary(const long long* keys_sorted, const long long* entry, long ns, unsigned char* bnd, void* stream);
int adamvs_clean_successor(const unsigned* faces, long ns, long nv, const unsigned char* bnd, int* out_count, int* in_count, int* out_edge,
                           int* succ, int* lab, int* nxt, unsigned char* broken, void* stream);
int adamvs_clean_double(const unsigned char* bnd, long ns, const int* lab_in, const int* nxt_in, const unsigned char* broken_in, int* lab_out,
                        int* nxt_out, unsigned char* broken_out, void* stream);
int adamvs_clean_validate(const unsigned char* bnd, const int* succ, const int* lab, const unsigned char* broken, long ns, int max_hole_edges,
                          int* count, unsigned char* bad, int* loop, unsigned char* closed, void* stream);
int adamvs_clean_accumulate(const double* p, const unsigned char* rgb, long nv, const unsigned* faces, long ns, const int* members, long nm,
                            const long long* start, long nl, const double* origin, double* centre, unsigned char* colour, void* stream);
int adamvs_clean_emit(const double* xyz, const unsigned char* rgb, long nv, const int* new_index, const unsigned* faces, long ns,
                      const int* fill_edge, const int* loop_of, long nfill, const double* centre, const unsigned char* colour, long nl, long nvs,
                      double* xyz_out, unsigned char* rgb_out, unsigned* faces_out, void* stream);

/* ---- Cloud distance (scoring a cloud or a mesh against a truth): bounded nearest neighbour and a surface sampler ---------------
 * ada-mvs_amd/accuracy.py drives it; accuracy_whu.py is the CLI.  Accuracy is the distance from every point of a reconstruction
 * to its nearest point of the truth, completeness the same the other way round (the DTU and Tanks-and-Temples measures); both
 * are one search: for every QUERY the nearest TARGET within the truncation distance D.
 *
 * Inputs: targets T [nt][3] and queries Q [nq][3], fp64 world; D > 0 in metres; the lattice origin O (fp64).
 *
 * 1. Lattice.  Cell side c = D.  The driver's default origin is, per axis, (min of the targets) - c / 3 - c: the third keeps
 *    a plane at a round height off a cell boundary, the whole cell keeps every target's lower neighbour inside the lattice.
 *    Cells, keys (x in the low bits) and cell centres are those of step 1 of "Mesh simplification", computed by
 *    _simplify_keys for both clouds.  A target that is not finite or lies outside the 2^21 cells of an axis is an error of
 *    the driver.  A query that is not finite or outside the lattice is no error: it has no candidates.
 * 2. Candidates of a query in cell (ix, iy, iz): the targets of the 27 cells (ix - 1 .. ix + 1, iy - 1 .. iy + 1,
 *    iz - 1 .. iz + 1) that exist in the lattice.  Every target within D of the query is among them, since c = D.
 * 3. Distance.  With the centre C (fp64) of the QUERY's cell:  qf = fp32(q - C),  pf = fp32(p - C), both subtractions in fp64,
 *    each component rounded once;  then in fp32, every operation rounded:  e = qf - pf,  d2 = (e.x e.x + e.y e.y) + e.z e.z.
 *    |q - C| <= c / 2 and |p - C| <= 3 c / 2 per component, whatever the world offset.
 * 4. Choice.  Over the candidates the least (d2, original index) in lexicographic order: among equal d2 the target with the
 *    lowest number in the CALLER's order wins, so the result is a function of the targets as a set.  The candidate is KEPT iff
 *    d2 <= fp32(D D) (the product in fp64, rounded once).  Output per query, at its original position:  d2 fp32 and index int32
 *    of the kept candidate, else +inf and -1.  The driver reports dist = sqrt(d2) in fp32.
 *
 * Bound, with u = 2^-24 (half an ulp of fp32, relative).  Rounding q - C (at most c / 2) costs u c / 2, rounding p - C (at most
 * 3 c / 2) costs 3 u c / 2, rounding the difference e (at most c wherever d <= D matters) costs u c: at most 3 u c = 1.8e-7 c
 * per component (2.4e-7 c with ulps counted whole in places), at most sqrt(3) times that, 3.1e-7 c, on d when all three
 * components err the same way.  The fp64 subtractions share one C and round relative 2^-53: nothing at this scale.  A square
 * and two sums put at most 3 u on d2, the root halves that and adds its own u: 2.5 u d <= 1.5e-7 c for d <= D.  Hence
 *      | d - d_fp64 | <= 1e-6 c
 * with a factor two to spare; the tests hold the kernel to it.  A target within 1e-6 c of D, or two candidates within 2e-6 c
 * of each other, may fall either way; nothing else may.
 *
 * Calls, in stream order.  The caller sorts the target keys STABLY (-> the sorted targets [nt][3] fp64, gathered, and tindex
 * [nt] int32, their numbers in the caller's order), takes the distinct keys ascending (ukeys [nc] int64) with the start of each
 * cell's run (tstart [nc + 1] int64, tstart[nc] = nt), sorts the query keys stably (qorder [nqs] int64: the queries with a
 * key >= 0 in sorted order, as numbers in the caller's order) and cuts every run of equal query keys into WORK ITEMS of at most
 * ADAMVS_CLOUD_TILE queries (item_key, item_first [ni] int64: the cell and the position in qorder; item_count [ni] int32).
 *   _cloud_nearest        one workgroup of 256 lanes per work item.  Nine lanes find the nine rows (dy, dz) of step 2: with x in
 *                         the low key bits the cells ix - 1 .. ix + 1 of a row are one run of the sorted targets, found by two
 *                         binary searches in ukeys; a row outside the lattice and an empty row give an empty run.  The nine
 *                         runs, row (dy, dz) = (-1, -1), (0, -1), (1, -1), (-1, 0), .. in that order, are walked as one sequence
 *                         in tiles of 256 candidates: each lane forms pf of one candidate and stores (pf, index) as one 16-byte
 *                         LDS entry.  With P the smallest power of two >= the item's queries the 256 lanes form S = 256 / P
 *                         SLICES: lane l serves query l mod P in slice l / P, and after the barrier sweeps candidates
 *                         slice, slice + S, .. of the tile, the lanes of a slice reading one shared address (a broadcast; the
 *                         slices of a wave read consecutive entries, which lie in different banks).  The S partial results
 *                         of a query meet in a tree under the rule of step 4, a minimum, so the result does not depend on
 *                         how the candidates were split.  d2 and index must be pre-filled with +inf and -1 by the caller: queries
 *                         outside every work item are not written.  pairs [ni] uint64: the (query, candidate) pairs each
 *                         workgroup evaluated (candidates of the item times its queries).  No atomics, no waits between
 *                         workgroups: bit-identical from run to run and under any permutation of T or of Q;
 *   _cloud_nearest_host   steps 1 to 4 on the HOST for small nt, nq (host pointers, the same inline functions for the row
 *                         search, the pair update and the truncation as the kernel; the keys are recomputed here);
 *                         pairs: one uint64 or null.  For checks of the rule on a machine without a device.
 *
 * Surface sampler: a mesh (xyz [nv][3] fp64, faces [nf][3] uint32) is scored through points on its faces.  With the spacing
 * s > 0 and the corners v0, v1, v2 of a face, all in fp64 without contraction:
 *      n = max(1, ceil(L / s)),   L = sqrt(max over the edges (v0 v1), (v1 v2), (v2 v0) of (dx dx + dy dy) + dz dz);
 *      sample (i, j), i + j <= n:   (v0 + (i / n) (v1 - v0)) + (j / n) (v2 - v0)   per component, in exactly this order.
 * Faces ascending; within a face i ascending, then j: (n + 1)(n + 2) / 2 samples, the corners included, so samples shared by
 * neighbouring faces stay duplicated.  n > ADAMVS_CLOUD_MAX_SUBDIV = 1024 (or L not finite) is an error of the driver, which
 * names the face.  Covering: the samples split the face into n^2 congruent triangles with edges <= L / n <= s, and every point
 * of a triangle with edges <= s lies within s / sqrt(3) of a corner (the circumradius of the equilateral case is the worst
 * that can hold a point away from all three corners).  Hence every point of a face lies within s / sqrt(3) of a sample, and
 * for any point x:  d_samples(x)^2 <= d_surface(x)^2 + s^2 / 3.
 *   _cloud_sample_count   subdiv [nf] int32: n per face; 1025 for n > 1024 or L not finite; 0 for a face with an index >= nv;
 *   _cloud_sample_emit    offsets [nf + 1] int64: the exclusive sum of (n + 1)(n + 2) / 2 over the faces (the caller's); points
 *                         [total][3] fp64.  One wave per face.  Nothing is written at or past capacity.  Bit-identical to the
 *                         restatement of the formula above.
 * Argument errors (<0, before any launch): a null pointer, a count < 1 or > 2^31 - 1, nc > nt, D or s not finite or <= 0, O not
 * finite, a capacity < 0. */
#define ADAMVS_CLOUD_TILE 256
#define ADAMVS_CLOUD_MAX_SUBDIV 1024

int adamvs_cloud_nearest(const double* origin, double D, const long long* ukeys, const long long* tstart, int nc, const double* targets,
                         const int* tindex, long nt, const double* queries, long nq, const long long* qorder, long nqs,
                         const long long* item_key, const long long* item_first, const int* item_count, long ni, float* d2, int* index,
                         unsigned long long* pairs, void* stream);
int adamvs_cloud_nearest_host(const double* origin, double D, const double* targets, long nt, const double* queries, long nq, float* d2,
                              int* index, unsigned long long* pairs);
int adamvs_cloud_sample_count(const double* xyz, long nv, const unsigned* faces, long nf, double spacing, int* subdiv, void* stream);
int adamvs_cloud_sample_emit(const double* xyz, long nv, const unsigned* faces, long nf, const int* subdiv, const long long* offsets,
                             double* points, long capacity, void* stream);

/* ---- Cloud neighbourhoods (filtering the fused cloud): the k nearest neighbours of every point, and a normal from them --------
 * ada-mvs_amd/cloud_filter.py drives it; filter_whu.py is the CLI (after fuse_whu.py, before everything that reads the cloud).
 * Nothing else judges a fused point against the fused points around it: the statistical and the radius outlier rules and the
 * normals all rest on one search: for every point the k nearest OTHER points within the radius R.
 *
 * Inputs: the cloud P [n][3], fp64 world; R > 0 in metres; 1 <= k <= ADAMVS_KNN_MAX_K = 32; the lattice origin O (fp64).
 *
 * Steps 1 to 3 are those of "Cloud distance" with D = R, the cloud being both the targets and the queries: the lattice of cell
 * side c = R (keys by _simplify_keys; a point that is not finite or outside the lattice is an error of the driver), the
 * candidates of a point from the 27 cells around its own, and d2 in fp32 relative to the centre C of the QUERY's cell
 * (qf = fp32(q - C), pf = fp32(p - C), e = qf - pf, d2 = (e.x e.x + e.y e.y) + e.z e.z, every operation rounded).  d2 of the pair
 * (i, j) is taken about the centre of i's cell and d2 of (j, i) about the centre of j's: the two may differ in the last bits.
 * 4. Choice.  A candidate j of the point i is a NEIGHBOUR iff j != i (another NUMBER: an exact duplicate of p_i at another
 *    number is a neighbour at d2 = 0) and d2 <= fp32(R R) (the product in fp64, rounded once: the keep rule of "Cloud
 *    distance").  Of its neighbours the point keeps the k that are least in the lexicographic order (d2, number in the caller's
 *    order): among equal d2 the lower number comes first, and of two equidistant candidates for the last place the lower number
 *    stays.  Output per point:  d2 [k] fp32 ascending in that order, padded with +inf;  index [k] int32, padded with -1;
 *    count int32 = min(k, neighbours).  The result is a function of the cloud as a set.
 *
 * Bound.  The arithmetic is that of "Cloud distance", so with d = sqrt(d2):  | d - d_fp64 | <= 1e-6 c  for every kept neighbour.
 * A candidate within 1e-6 c of R may be counted or not, and two candidates within 2e-6 c of each other may swap places (or, at
 * the last place, one may stand for the other); nothing else may differ from an fp64 search.
 *
 * Calls, in stream order.  The caller sorts the keys STABLY (-> sorted [n][3] fp64, the points gathered, and pindex [n] int32,
 * their numbers in the caller's order), takes the distinct keys ascending (ukeys [nc] int64) with the start of each cell's run
 * (tstart [nc + 1] int64, tstart[nc] = n) and cuts every run into WORK ITEMS of at most ADAMVS_CLOUD_TILE points (item_key,
 * item_first [ni] int64: the cell and the position in the sorted order; item_count [ni] int32), exactly as for _cloud_nearest.
 *   _knn_search        one workgroup per work item; any contiguous range of the work items may be given to one call (the driver
 *                      runs a large cloud in such chunks, so that the [n][k] arrays never exist whole).  The point at sorted
 *                      position s is written at ROW s - row_base of d2 [rows][k], index [rows][k], count [rows]; rows outside
 *                      [0, rows) are not written, and rows no work item covers are left as they were.  Nine lanes find the nine
 *                      rows of cells and the candidates pass through an LDS tile as in _cloud_nearest; with P the smallest power
 *                      of two >= the queries of the pass the lanes form S slices, lane l serving query l mod P on candidates
 *                      slice, slice + S, ..  Every (query, candidate) pair is evaluated once.  Each lane keeps a list of at most
 *                      k entries in LDS columns (slot-major, so the lanes of a wave use different banks) and the list's worst
 *                      (d2, number) in registers: an entry is appended while the list has room, later it replaces the worst,
 *                      which one scan of the k slots finds again; once the list is full a candidate costs one compare unless it
 *                      enters.  The S lists of a query meet in a tree under the same order (the lower half takes the upper
 *                      half's entries), so the split does not show; the final list leaves through ranks: every entry is
 *                      written at the position given by the number of entries before it.  One kernel per class of k:
 *                      k <= 8 and k <= 16 with 256 lanes, k <= 32 with 128 lanes (32 KiB of lists each at most; an item
 *                      of more than 128 queries then walks its candidates twice, for different queries).  pairs [ni] uint64:
 *                      candidates of the item times its queries.  No atomics, no waits between workgroups: bit-identical
 *                      from run to run, independent of the chunking, equivariant under any permutation of P;
 *   _knn_search_host   steps 1 to 4 on the HOST for small n (host pointers; the same inline functions for the rows, the pair
 *                      and the order; the keys are recomputed here); rows are the points in the caller's order; pairs: one
 *                      uint64 or null.
 *
 * Normals.  For the point p with the neighbours x_0 .. x_(m-1), m = count, in the order of its list; fp64, every operation
 * rounded, no contraction.  The members are the differences d_j = x_j - p and the point itself as d_m = 0:  M = m + 1,
 *      mean = (sum of d_j, j ascending) / M;     e_j = d_j - mean  (e_m = 0 - mean);
 *      C_ab = (sum over j = 0 .. m of e_j.a e_j.b, j ascending) / M,   the six entries of the symmetric 3x3.
 * Cyclic Jacobi on C from V = I, 8 sweeps of the rotations (0,1), (0,2), (1,2): the rotation of "Mesh simplification".  Of
 * the diagonal, lambda0 is the least entry (the lowest position among equals), lambda2 the largest (the highest position among
 * equals), lambda1 the third.  The point is VALID iff m >= 3 and lambda1 > ADAMVS_KNN_RANK_EPS lambda2, rank_eps = 1e-12: points
 * on a line leave lambda1 at rounding level, some 1e-32 lambda2, and any real spread across the line is far above 1e-12.
 *      normal = v / sqrt((v.x v.x + v.y v.y) + v.z v.z),  v the column of V of lambda0;  flipped if the first non-zero of
 *      (n.z, n.y, n.x) is negative (UPWARD; the fused cloud does not record its views, so nothing orients towards a camera);
 *      curvature = fp32(l / ((l + lambda1) + lambda2)),  l = max(lambda0, 0):  the surface variation of Pauly et al. (PCL's).
 * A point that is not valid has normal (0, 0, 0), curvature 0 and flag ADAMVS_KNN_TOO_FEW = 1 (m < 3) or ADAMVS_KNN_COLLINEAR =
 * 2; a valid one has flag ADAMVS_KNN_VALID = 0.
 *   _knn_normals       one lane per row.  points [n][3] fp64 in the caller's order; index [rows][k], count [rows] of _knn_search;
 *                      row_point [rows] int32: the number of each row's point (null: row r is point r).  normal [rows][3]
 *                      fp64, curvature [rows] fp32, flag [rows] uint8.  A neighbour number outside [0, n) is skipped;
 *   _knn_normals_host  the same on the HOST through the same inline function.
 * Argument errors (<0, before any launch): a null pointer (row_point and the host's pairs may be null), k outside 1 .. 32, R not
 * finite or <= 0, O not finite, a count < 1 or > 2^31 - 1, nc > n, a row range outside the cloud. */
#define ADAMVS_KNN_MAX_K 32
#define ADAMVS_KNN_RANK_EPS 1e-12
#define ADAMVS_KNN_VALID 0
#define ADAMVS_KNN_TOO_FEW 1
#define ADAMVS_KNN_COLLINEAR 2

int adamvs_knn_search(const double* origin, double R, int k, const long long* ukeys, const long long* tstart, int nc, const double* sorted,
                      const int* pindex, long n, const long long* item_key, const long long* item_first, const int* item_count, long ni,
                      long long row_base, long rows, float* d2, int* index, int* count, unsigned long long* pairs, void* stream);
int adamvs_knn_search_host(const double* origin, double R, int k, const double* points, long n, float* d2, int* index, int* count,
                           unsigned long long* pairs);
int adamvs_knn_normals(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                       double* normal, float* curvature, unsigned char* flag, void* stream);
int adamvs_knn_normals_host(const double* points, long n, const int* index, const int* count, int k, long rows, const int* row_point,
                            double* normal, float* curvature, unsigned char* flag);

/* ---- Cloud registration (before accuracy_whu.py): a reconstruction aligned to the truth by point-to-plane ICP ----------------
 * ada-mvs_amd/register.py drives it; register_whu.py is the CLI.  A reconstruction and an independently georeferenced truth
 * never share a frame exactly, and a residual shift or tilt lands in every figure of "Cloud distance"; DTU and Tanks and
 * Temples register by ICP before they score.  The SOURCE (the reconstruction) is moved onto the TARGET (the truth).
 *
 * All arithmetic below is fp64 without contraction: every operation written is one rounding.
 *
 * Transform.  (R [3][3] row-major, t [3]) about a pivot c [3]:  y = R (x - c) + c + t.  The driver takes c as the centre of the
 * targets' bounding box, (min + max) / 2 per axis (exact, and independent of the targets' order), so that the products R d
 * are formed on numbers of the size of the scene, not of its georeferenced offset.
 *   _rigid_apply        one lane per point.  d = x - c;  y_k = ((R_k0 d_0 + R_k1 d_1) + R_k2 d_2) + u_k,  with u = c + t formed by
 *                       the caller in fp64.  A point that is not finite stays not finite (every component of y).  With R = I and
 *                       t = 0 a point whose components lie within [c_k / 2, 2 c_k] (a georeferenced scene about its own centre)
 *                       comes back with its own bits: the difference is then exact;
 *   _rigid_apply_host   the same on the HOST through the same inline function.
 *
 * Correspondences.  The moved source Y [nq][3] is searched against the targets by _cloud_nearest with D = the truncation
 * distance: index [nq] int32, the nearest target's number in the caller's order or -1.  The targets P [nt][3] carry normals
 * N [nt][3] fp64 and flags [nt] uint8 of "Cloud neighbourhoods" (ADAMVS_KNN_VALID = 0), all in the caller's order.  The sign
 * of a normal does not matter below.
 *
 * Sums.  With the pivot c, a length scale L > 0 (the driver's: max(half the diagonal of the targets' box, D)) and a Huber
 * width delta (delta <= 0: off), query i is a PAIR iff 0 <= j = index[i] < nt, flag[j] == 0 and y = Y_i is finite.  For a pair,
 * with p = P_j and n = N_j:
 *      e = y - p;    r = (e_0 n_0 + e_1 n_1) + e_2 n_2;    q = (y - c) / L  (three divisions);
 *      a = (q x n, n), six numbers:  a_0 = q_1 n_2 - q_2 n_1,  a_1 = q_2 n_0 - q_0 n_2,  a_2 = q_0 n_1 - q_1 n_0  (each the
 *      difference of two products),  a_3 .. a_5 = n;
 *      w = 1 if delta <= 0 or |r| <= delta, else delta / |r|.
 * To first order a rotation by the vector omega about c and a shift dt change r by a . x with x = (L omega, dt): L makes the six
 * unknowns of one size.  The ADAMVS_ICP_TERMS = 32 TERMS of a pair, in this order:
 *      0 .. 20   (w a_u) a_v for u <= v, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5);
 *      21 .. 26  (w a_u) r;
 *      27 .. 31  (w r) r,   r r,   (e_0 e_0 + e_1 e_1) + e_2 e_2,   1.0,   w.
 * A query that is no pair contributes 32 zeros.  The sums of 0 .. 20 are the upper triangle of A = sum w a a^T, those of
 * 21 .. 26 are g = sum w a r; the driver solves A x = -g on the host through the eigenpairs of A, keeping those with
 * lambda_i > min_eig_ratio lambda_max (a flat scene constrains three of the six freedoms; the others stay where they were).
 * Sum 30 is the number of pairs, 28 and 29 over it the mean squares of the point-to-plane and point-to-point residuals.
 *   _icp_accumulate     workgroup b (256 lanes) owns queries 256 b .. 256 b + 255 (lanes past nq hold zeros).  Each term is summed
 *                       within each wave by the fixed butterfly over lane distances 32, 16, .. 1 (s_l <- s_l + s_(l xor m),
 *                       every lane ends with the same bits), then the four wave sums as (W0 + W1) + (W2 + W3).
 *                       partial [nb][32] fp64, nb = ceil(nq / 256);
 *   _icp_reduce         one workgroup of 256.  Lane l adds partial[b] for b = l, l + 256, .. ascending, starting from 0.0; then
 *                       the same wave and (W0 + W1) + (W2 + W3) order.  sums [32] fp64.  nb = 0 gives zeros;
 *   _icp_accumulate_host, _icp_reduce_host   the same on the HOST (host pointers) through the same inline functions and the same
 *                       order of additions, so that the whole loop can be checked on a machine without a device.
 * No atomics and no inter-workgroup waits.  The sums depend on the queries' order and on nothing else: not on the launch
 * shape, and (the index naming a target by its number in the caller's order) not on how the search ordered the targets; they
 * are bit-identical from run to run.
 * Argument errors (<0, before any launch): a null pointer, a count < 0 or > 2^31 - 1, R, c or u not finite, L not finite or
 * <= 0, delta NaN. */
#define ADAMVS_ICP_TERMS 32

int adamvs_rigid_apply(const double* R, const double* c, const double* u, const double* x, long n, double* y, void* stream);
int adamvs_rigid_apply_host(const double* R, const double* c, const double* u, const double* x, long n, double* y);
int adamvs_icp_accumulate(const double* y, const int* index, long nq, const double* targets, const double* normals,
                          const unsigned char* flag, long nt, const double* c, double L, double delta, double* partial, void* stream);
int adamvs_icp_accumulate_host(const double* y, const int* index, long nq, const double* targets, const double* normals,
                               const unsigned char* flag, long nt, const double* c, double L, double delta, double* partial);
int adamvs_icp_reduce(const double* partial, long nb, double* sums, void* stream);
int adamvs_icp_reduce_host(const double* partial, long nb, double* sums);

/* ---- Image orthophoto (after dsm_whu.py): the source images mosaicked over a DSM into a true orthophoto -------------------
 * ada-mvs_amd/ortho.py drives it; ortho_whu.py is the CLI.  World axes: x east, y north, z up; rows run south.
 *
 * Grid.  The DSM grid (x0, y_top, gsd fp64; W x H cells, row 0 north) and K = upsample, an integer 1 .. 8.  The orthophoto
 * has W_o = W K by H_o = H K cells of size g = gsd / K (fp64), at most ADAMVS_ORTHO_MAX_CELLS = 2^28; cell (i, j) (column i,
 * row j) is entry j W_o + i and has its centre at x = x0 + (i + 1/2) g, y = y_top - (j + 1/2) g.
 *
 * Surface (adamvs_ortho_surface).  The DSM dsm [H][W] fp32 (NaN: no surface) is a triangulated height field: its vertices are
 * the cell centres (a, b), world (x0 + (a + 1/2) gsd, y_top - (b + 1/2) gsd, dsm[b][a]) in fp64, and each quad
 * (a, b) - (a+1, b+1) is split along that diagonal into (a,b) (a+1,b) (a+1,b+1) and (a,b) (a,b+1) (a+1,b+1).  For cell (i, j),
 * in fp64:  s = (i + 1/2) / K - 1/2,  t = (j + 1/2) / K - 1/2,  clamped to [0, W-1] x [0, H-1];  a = floor(s), fs = s - a,
 * b = floor(t), ft = t - b;  if fs >= ft the vertices (a,b) (a+1,b) (a+1,b+1) have weights (1-fs, fs-ft, ft), otherwise
 * (a,b) (a,b+1) (a+1,b+1) have (1-ft, ft-fs, fs).  height = sum of w z over the vertices with w > 0, in that order (fp64);
 * NaN unless every such vertex is finite.  Vertices of weight 0 are not read, so K = 1 gives the DSM cell for cell.
 *
 * Views.  A HOST pointer to an adamvs_ortho_view, copied into the arguments: C (camera centre, world, fp64), R = R_cw (fp32,
 * row-major, world -> camera x right / y down / z forward), K (fp32, row-major, last row 0 0 1), the image [H][W][4] uint8
 * RGBA (device; alpha ignored).  Projection of a world point X (fp64):  d = (float)(X - C) per axis (the difference in fp64,
 * so 10^6 m coordinates lose nothing), p = R d, z = p.z, u = (K00 p.x + K01 p.y + K02 z) / z, v = (K10 p.x + K11 p.y + K12 z) / z,
 * fp32, left to right, no contraction.  Pixel centres are integer (u, v).
 *
 * Z-buffer (adamvs_ortho_zbuf), per view: zbuf [H][W] uint32, the bits of a positive float, cleared to +inf (0x7F800000) by the
 * call.  Every triangle of the split whose three vertices are finite, project with z > ADAMVS_ORTHO_NEAR = 0.1 m and finite
 * (u, v), is rasterised:  area = (u1-u0)(v2-v0) - (v1-v0)(u2-u0); skipped if 0 or not finite; if < 0, vertices 1 and 2 swap and
 * area = -area.  For a pixel centre (x, y) inside the image:  e0 = (u2-u1)(y-v1) - (v2-v1)(x-u1),
 * e1 = (u0-u2)(y-v2) - (v0-v2)(x-u2),  e2 = (u1-u0)(y-v0) - (v1-v0)(x-u0);  covered iff e0, e1, e2 >= 0 (inclusive);
 * depth = area / (e0 / z0 + e1 / z1 + e2 / z2) (1/z linear in screen space; the reciprocals 1/z_k taken first, fp32), and
 * zbuf = atomicMin(zbuf, bits(depth)) (order-independent: bit-identical from run to run).  Triangles whose box of pixel
 * centres holds more than ADAMVS_ORTHO_SMALL_PX are rasterised one wave per triangle from a list (big_list, at least
 * 2 (W-1)(H-1) entries; big_count one uint32), so long triangles do not stall a wave of short ones; the result is the same.
 *
 * Visibility of the sample P = (x, y, height) of cell (i, j) in a view: height is not NaN; z > 0; border <= u <= W-1-border and
 * border <= v <= H-1-border (fp32); and z <= zbuf[floor(v + 1/2)][floor(u + 1/2)] + occlusion_tol (fp32).
 * Score s = -d.z / sqrt(d.x d.x + d.y d.y + d.z d.z) (fp32: the cosine of the ray's off-nadir angle).  Colour c = a bilinear
 * sample at (u, v): x_a = floor(u), f_x = u - x_a, x_b = min(x_a + 1, W - 1) (likewise y),
 * c = (1 - f_y)((1 - f_x) c(x_a,y_a) + f_x c(x_b,y_a)) + f_y((1 - f_x) c(x_a,y_b) + f_x c(x_b,y_b)) per channel, fp32.
 *
 * Compose (adamvs_ortho_compose), one call per view in ascending image id, one lane per cell (the cell's state is owned by
 * that lane: no atomics).  State: acc [N][4] fp32, wmax [N] fp32, view [N] int32, nvis [N] int32; the caller initialises
 * acc = 0, view = -1, nvis = 0 and wmax = -inf (best) or 0 (feather).  A visible view adds 1 to nvis and:
 *   ADAMVS_ORTHO_BEST:    if s > wmax:  wmax = s, view = view_id, acc = (1, c)  (an equal score keeps the earlier view);
 *   ADAMVS_ORTHO_FEATHER: e = min(u, W-1-u, v, H-1-v),  w = (s s)(s s) min(1, (e - border) / feather_px);
 *                         acc += (w, w c) in fp32;  if w > wmax:  wmax = w, view = view_id.
 * Finalize (adamvs_ortho_finalize): where view >= 0 and acc.0 > 0, rgba = (floor(acc.k / acc.0 + 1/2) clamped to 0 .. 255,
 * k = 1..3, alpha 255) and view_out = view; elsewhere rgba = 0 and view_out = -1.  nvis_out = min(nvis, 65535) uint16.
 * rgba [N][4] uint8, view_out [N] int32, nvis_out [N] uint16.
 *
 * Argument errors (<0, before any launch): a null pointer, W or H < 1, K not in 1 .. 8, W_o H_o > ADAMVS_ORTHO_MAX_CELLS,
 * x0 / y_top / gsd not finite or gsd <= 0, a view of H or W < 1 or with a non-finite C, R or K or K's last row not 0 0 1,
 * big_capacity < 2 (W-1)(H-1), an unknown mode, border < 0 or not finite, feather_px <= 0 or not finite, occlusion_tol < 0 or
 * not finite. */
#define ADAMVS_ORTHO_TILE 256
#define ADAMVS_ORTHO_MAX_CELLS (1L << 28)
#define ADAMVS_ORTHO_MAX_UPSAMPLE 8
#define ADAMVS_ORTHO_NEAR 0.1f
#define ADAMVS_ORTHO_SMALL_PX 16
#define ADAMVS_ORTHO_BEST 0
#define ADAMVS_ORTHO_FEATHER 1

typedef struct {
  double x0, y_top, gsd;
  int W, H, K;
} adamvs_ortho_grid;

typedef struct {
  double C[3];
  float R[9];
  float K[9];
  int H, W;
  const unsigned char* rgba;
} adamvs_ortho_view;

int adamvs_ortho_surface(const adamvs_ortho_grid* grid, const float* dsm, double* height, void* stream);
int adamvs_ortho_zbuf(const adamvs_ortho_grid* grid, const float* dsm, const adamvs_ortho_view* view, unsigned* zbuf, unsigned* big_count,
                      unsigned* big_list, long big_capacity, void* stream);
int adamvs_ortho_compose(const adamvs_ortho_grid* grid, const adamvs_ortho_view* view, int view_id, const double* height,
                         const unsigned* zbuf, int mode, float border, float feather_px, float occlusion_tol, float* acc, float* wmax,
                         int* view_state, int* nvis, void* stream);
int adamvs_ortho_finalize(const adamvs_ortho_grid* grid, const float* acc, const int* view_state, const int* nvis, unsigned char* rgba,
                          int* view_out, unsigned short* nvis_out, void* stream);

/* ---- Image orthophoto: radiometric balance (ortho_whu.py --balance gain) ---------------------------------------------------
 * ada-mvs_amd/ortho.py drives it.  One gain per view and channel, from the pairwise statistics of the views over the cells
 * they both see (the block adjustment of Brown & Lowe 2007; OpenCV's GainCompensator); the V x V solve is the host's.  Every
 * device result of this section is an integer.
 *
 * Observation lattice.  For a stride S (integer >= 1) the lattice is the DSM cells (a S, b S), a < W_s = ceil(W / S),
 * b < H_s = ceil(H / S); N_s = W_s H_s <= ADAMVS_ORTHO_BAL_MAX_SAMPLES = 2^20; lattice cell (a, b) is entry b W_s + a.  Its
 * sample is the K = 1 sample of DSM cell (a S, b S): x = x0 + (a S + 1/2) gsd, y = y_top - (b S + 1/2) gsd, height
 * dsm[b S][a S] as fp64 (not finite: no surface).  No height array is needed, and the balance does not depend on the upsample.
 *
 * adamvs_ortho_observe, per view: one lane per lattice cell; grid.K is ignored.  obs [N_s][4] uint16 (8-byte aligned) is written
 * completely by the call.  Where the sample is visible in the view, by exactly the visibility rule of "Image orthophoto" (zbuf
 * is the view's buffer from adamvs_ortho_zbuf), with c its bilinear sample:  obs = (q_r, q_g, q_b, 1),
 * q_k = floor(64 c_k + 1/2) in fp32 (64 c_k is exact; at most 16320).  Elsewhere obs = (0, 0, 0, 0).
 *
 * adamvs_ortho_pair_stats: obs [V][N_s][4] uint16 (the views' planes, 8-byte aligned), pairs [P][2] int32 (device) with
 * 0 <= a < b < V (NOT checked on the device: the caller checks them), stats [P][7] int64, zeroed by the call with a kernel.
 * For pair p = (a, b), over every lattice cell where both flags are 1 and |q_a,k - q_b,k| <= max_diff_q for k = 0, 1, 2:
 * n += 1, Sa_k += q_a,k, Sb_k += q_b,k; the layout is (n, Sa_0, Sa_1, Sa_2, Sb_0, Sb_1, Sb_2).  All sums are integers (at most
 * 2^20 x 16320 < 2^34) and are added with integer atomics, so the result does not depend on the order of the reduction: it is
 * bit-identical from run to run and equal to any exact restatement.  One workgroup per (chunk of ADAMVS_ORTHO_BAL_CHUNK lattice
 * cells, pair), P ceil(N_s / chunk) < 2^31 of them; it adds its seven sums with one 64-bit atomic each.  P = 0 returns 0
 * without a launch (and before the pointers are looked at).
 *
 * adamvs_ortho_adjust_image: rgba_in, rgba_out [H][W][4] uint8 (device; they may not alias), gain [3] a HOST pointer.  One lane
 * per pixel:  out_k = min(255, floor(gain_k * (float)in_k + 0.5f)) for k = 0 .. 2 (one fp32 product, one fp32 sum, no
 * contraction); alpha is copied.
 *
 * adamvs_ortho_seam_stats: over the W_o x H_o mosaic adamvs_ortho_finalize wrote (view_out [N] int32, rgba [N][4] uint8), every
 * horizontally and every vertically adjacent pair of cells with both view_out >= 0 and different views:  stats[0] += 1,
 * stats[1 + k] += d_k d_k with d_k the integer difference of channel k.  stats [4] int64, zeroed by the call; integer atomics,
 * one set per workgroup.  The rms colour step across seams is sqrt((s1 + s2 + s3) / (3 s0)).
 *
 * Argument errors (<0, before any launch), beyond those of the calls above: S < 1 or N_s > ADAMVS_ORTHO_BAL_MAX_SAMPLES;
 * V < 1, N_s < 1 or N_s over the cap, P < 0 or 2^31 workgroups or more; max_diff_q outside 0 .. ADAMVS_ORTHO_BAL_MAX_Q; a gain
 * that is not finite or <= 0; H or W < 1 (H W at most ADAMVS_ORTHO_MAX_CELLS); a null pointer; rgba_out == rgba_in. */
#define ADAMVS_ORTHO_BAL_MAX_SAMPLES (1L << 20)
#define ADAMVS_ORTHO_BAL_CHUNK 8192
#define ADAMVS_ORTHO_BAL_MAX_Q 16320

int adamvs_ortho_observe(const adamvs_ortho_grid* grid, const float* dsm, const adamvs_ortho_view* view, const unsigned* zbuf, int S,
                         float border, float occlusion_tol, unsigned short* obs, void* stream);
int adamvs_ortho_pair_stats(const unsigned short* obs, int V, long N_s, const int* pairs, int P, int max_diff_q, long long* stats,
                            void* stream);
int adamvs_ortho_adjust_image(const unsigned char* rgba_in, int H, int W, const float* gain, unsigned char* rgba_out, void* stream);
int adamvs_ortho_seam_stats(const adamvs_ortho_grid* grid, const int* view_out, const unsigned char* rgba, long long* stats,
                            void* stream);

/* ---- Mesh texturing (after mesh_whu.py): a triangle mesh textured from the source images ----------------------------------
 * ada-mvs_amd/texture.py drives it; texture_whu.py is the CLI.  Views are adamvs_ortho_view structs (a HOST pointer, copied into the
 * arguments; projection exactly as "Image orthophoto" states it).  Mesh: xyz [nv][3] fp64 (device), faces [nf][3] uint32,
 * counter-clockwise about the outward normal; a face with an index >= nv is ignored by every call (no view, no chart).
 * 1 <= nv, 0 <= nf <= 2^31 - 1.  Workgroups cover ADAMVS_TEXTURE_TILE consecutive faces (vertices, edge entries, texels).
 *
 * Labelling, one call of each per view in ascending image id:
 *   _project  uvz [nv][4] fp32: (u, v, z, 0) of every vertex.
 *   _zbuf     zbuf [H][W] uint32, cleared to +inf by the call, then every face whose three vertices have z > ADAMVS_ORTHO_NEAR
 *             and finite (u, v, z) is rasterised by the orthophoto's rule (set-up, inclusive edge functions, 1/z interpolated in
 *             screen space, atomicMin on the bits); faces whose box holds more than ADAMVS_ORTHO_SMALL_PX pixel centres go
 *             through big_list (at least nf entries) one wave per face.  The result does not depend on that split.
 *   _score    face f with vertices (u_k, v_k, z_k) is VISIBLE iff every z_k > ADAMVS_ORTHO_NEAR and
 *             border <= u_k <= W-1-border, border <= v_k <= H-1-border (fp32); area = (u1-u0)(v2-v0) - (v1-v0)(u2-u0) < 0
 *             (front-facing: counter-clockwise about the outward normal is clockwise in an image whose v runs down; no swap);
 *             z_k <= zbuf[floor(v_k + 1/2)][floor(u_k + 1/2)] + tol for k = 0, 1, 2 and for the centroid
 *             uc = (u0 + u1 + u2) / 3, vc = (v0 + v1 + v2) / 3, zc = 3 / (1/z0 + 1/z1 + 1/z2) (fp32, left to right).
 *             Then nvis += 1 and, with score = -area / 2: if score > best, best = score, label = view, uv = (u0 v0 u1 v1 u2 v2)
 *             (a tie keeps the earlier view).  State: best [nf] fp32 (caller: -inf), label [nf] int32 (-1), nvis [nf] int32
 *             (0), uv [nf][6] fp32.  One lane per face owns its state: no atomics.
 * Charts: a chart is a maximal set of faces with the same label >= 0 connected through shared edges.
 *   _edge_keys   keys [3 nf] int64: entry e = 3 f + k is the edge (faces[f][k], faces[f][(k+1) % 3]) as min << 32 | max.
 *                The caller sorts the entries by key, then label, then e (a stable sort by label, then a stable one by key)
 *                into keys_sorted and entry (int64 entry ids).
 *   _components  parent [nf] int32 (caller: parent[f] = f); one round: sorted neighbours i, i+1 with equal keys and equal labels
 *                >= 0 and roots ra = parent[a] != rb = parent[b] do atomicMin(parent[max(ra, rb)], min(ra, rb)) and set
 *                *changed (cleared by the call); then every face walks to its root and stores it.  The caller repeats rounds
 *                until *changed stays 0: then parent[f] is the smallest face of f's chart.  parent[x] <= x holds throughout.
 *   _rank        chart ids in ascending root order and palette indices of the untextured faces (label -1) in face order:
 *                root_chart [nf] (the chart id of a root, -1 elsewhere), pal [nf] (-1 for textured faces); block_roots,
 *                block_untex [nblocks], root_off, untex_off [nblocks + 1] uint32 workspace; root_off[nblocks] is the chart
 *                count and untex_off[nblocks] the untextured count (adamvs_fusion_scan).
 *   _boxes       chart [nf] int32 (-1 untextured); box [nc][4] int32 (caller: INT_MAX, INT_MAX, INT_MIN, INT_MIN) becomes
 *                (min floor u, min floor v, max floor u, max floor v) over the chart's corners (atomic min / max).
 * Atlas: pages [npages][P][P] of uint32 texels, byte k = channel k (alpha byte 0); the caller zeroes them.  Charts are placed by
 * the caller: charts [nc][8] int32 = (x0, y0, w, h, ox, oy, page, view) with x0 = max(minu - pad, 0),
 * x1 = min(maxu + 1 + pad, W - 1), w = x1 - x0 + 1 (likewise y).
 *   _fill    per view: items [n][8] rows of charts (that view's), prefix [n + 1] int64 = exclusive sum of w h; texel t of the
 *            concatenation is image texel (x, y) of item k (prefix[k] <= t < prefix[k+1]) copied to atlas texel
 *            (ox + x - x0, oy + y - y0) of page `page`, alpha byte 0.  No resampling.
 *   _coords  tc [nf][6] fp32, texnum [nf] int32: a textured face of chart c has s_k = (ox + (u_k - x0) + 1/2) / P,
 *            t_k = 1 - (oy + (v_k - y0) + 1/2) / P (fp32, left to right) and texnum = page; the k-th untextured face has
 *            all three corners at the centre of texel (pal_ox + k mod P, pal_oy + k div P) of page pal_page, which it writes:
 *            per channel (c0 + c1 + c2 + 1) div 3 of its vertex colours vrgb [nv][3] uint8 (the rounded mean).
 * Argument errors (<0, before any launch): a null pointer where data is read or written, nv < 1, nf < 0 or > 2^31 - 1, a view
 * of H or W < 1 or with a non-finite C, R or K or K's last row not 0 0 1, border or tol < 0 or not finite, big_capacity < nf,
 * P not a power of two in ADAMVS_TEXTURE_MIN_PAGE .. ADAMVS_TEXTURE_MAX_PAGE, npages < 1, n < 0.
 *
 * Seam levelling (csrc/texture_level.hip; opt-in, after _boxes, the packing, _fill and _coords, on their labels, charts and atlas).
 * Every chart boundary between two views shows the views' difference in exposure; one additive correction g per node and
 * channel, found by one global least-squares solve and interpolated over the charts, levels it (Waechter et al. 2014, the
 * global adjustment; this definition is the project's own).
 * Nodes.  One node per distinct pair (vertex index v, chart c) over the corners of textured faces (chart >= 0), numbered in
 * ascending (v, c).  Untextured faces contribute nothing.  Vertices are identified by index: an unwelded mesh is levelled
 * brick by brick.  n <= ADAMVS_TEXTURE_LEVEL_MAX_NODES = 2^30.  corner_node [nf][3] int32: the node of every corner of a
 * textured face (anything on untextured faces: they own no texel).  pos [n][2] fp32: the node's (u, v) in its chart's view, the
 * uv the faces of c stored at v (every such face stored the same bits); node_view [n] int32: that view's index.
 * Edges, undirected, each once: SMOOTHNESS (weight 1 / lambda) between (v, c) and (w, c) for every distinct mesh edge {v, w},
 * v != w, of a face of chart c; DATA (weight 1) between (v, a) and (v, b) for every vertex v and charts a < b at v.  A smoothness
 * edge {v, w} of chart c is a SEAM edge if {v, w} is also an edge of a textured face of another chart.
 * Graph: a CSR over the nodes with both directions of every edge, rowptr [n + 1] int32, col [nnz] uint32 sorted by neighbour
 * within a row: bits 0 .. 29 the neighbour, bit 30 set on a seam edge, bit 31 set on a data edge.  Built by the caller.
 *   _level_observe  f [n][3] fp32 (R G B), the colour chart c's view shows at v.  sample(x, y) is the bilinear sample "Image
 *                   orthophoto" states, in view node_view[i] (view_tab [nviews][3] int64 on the device: the image's device
 *                   address, W, H).  With p = pos[i]: acc = 0, wsum = 0; for every seam edge of row i in ascending neighbour j,
 *                   d = pos[j] - p, and for (t, w) = (0, 1), (1/4, 3/4), (1/2, 1/2) in that order: acc = acc + w sample(p + t d),
 *                   wsum = wsum + w; f = acc / wsum (fp32, left to right, no contraction).  A node without a seam edge takes
 *                   f = sample(p).
 *   _level_rhs      b [n][3] fp64: b_i = sum over the data neighbours j of row i, ascending, of ((double)f_j - (double)f_i).
 * System.  Per channel, minimise  sum_data (f_i + g_i - f_j - g_j)^2 + (1 / lambda) sum_smooth (g_i - g_j)^2.  The normal
 * equations are the weighted graph Laplacian L g = b, L = D - W.  L is singular (constants per connected component); the
 * solution wanted is the MINIMUM-NORM one: a chart without seams keeps g = 0 exactly, a large chart moves less than a small
 * neighbour.
 * The solve takes any CSR of the graph: the driver renumbers the nodes for it (by chart, then along a Z-order curve of pos in
 * quarter pixels, ties in node order), so that a row's neighbours lie near it in memory, permutes b into that order and g back.
 * The numbering fixes the order of every sum, so it is part of what makes g reproducible bit for bit.
 *   _level_cg_init  g = 0, r = p = b, state: r.r = b.b per channel, iterations = 0, stop = every channel has r.r <= tol^2 b.b
 *                   (so b = 0 stops before the first iteration).
 *   _level_cg       `iters` iterations of plain conjugate gradients (NO preconditioner: from g = 0 the iterates stay in
 *                   range(L), so the limit is the minimum-norm solution; a Jacobi preconditioner changes that gauge), fp64
 *                   vectors [n][3] and scalars, the three channels interleaved, sharing L, each with its own alpha and beta:
 *                   Ap = L p;  alpha = r.r / p.Ap (0 if p.Ap <= 0);  g += alpha p;  r -= alpha Ap;  beta = r'.r' / r.r (0 if
 *                   r.r <= 0 or alpha = 0: a refused step restarts from r; with beta = 1 there p would double every iteration
 *                   until it overflows and 0 * inf reaches g);  iterations += 1;  stop as above;  p = r + beta p.  Once stop is
 *                   set every remaining kernel of the call (and of later calls) returns without writing: g and the count are
 *                   those of the stopping iteration, so the caller may queue 16 iterations per read of the flag.  Dot products: ADAMVS_TEXTURE_LEVEL_BLOCKS = 2048
 *                   workgroups at most, each a fixed run of rows, reduced by one workgroup in a fixed order; no floating-point
 *                   atomics, so g is bit-identical from run to run.  partials [3 ADAMVS_TEXTURE_LEVEL_BLOCKS] fp64 workspace.
 *                   g, r, p, Ap hold [n + 1][3] fp64, 16-byte aligned: one spare row, so that the update passes may read and
 *                   write the vectors 16 bytes per lane whatever the parity of 3 n; the spare row holds no data.
 *                   state [16] fp64: 0..2 r.r, 3..5 b.b, 6..8 alpha, 9..11 beta, 12 stop (0 / 1), 13 iterations, 14 tol^2.
 * Apply.  The texels of all chart boxes concatenated in chart order, row-major in each box: prefix [nc + 1] int64 = exclusive
 * sum of w h, texels = prefix[nc]; owner [texels] int32.
 *   _level_owner    owner = INT_MAX (unowned), then for every textured face f of chart c: its image triangle uv[f] set up as the
 *                   z-buffer's triangles are (orientation swap, box of pixel centres, here clamped to the chart's box) and
 *                   owner = atomicMin(owner, f) on every texel whose centre, the pixel centre (x0 + dx, y0 + dy), passes the
 *                   inclusive edge functions: the owner is the smallest face of c that holds the centre.  Faces whose box holds
 *                   more than ADAMVS_ORTHO_SMALL_PX centres go through big_list (at least nf entries) one wave per face.
 *   _level_dilate   one round, owner_in -> owner_out (two buffers): an owned texel keeps its owner; an unowned one takes the
 *                   owner of the first owned texel of its 3 x 3 neighbourhood inside the chart's box, in row-major order, of
 *                   owner_in.  The caller runs ADAMVS_TEXTURE_LEVEL_BAND = 2 rounds (bilinear taps of a face's texture
 *                   coordinates lie within one texel of its triangle).
 *   _level_apply    an owned texel with centre (x, y) and owner f = (u_k, v_k), corner nodes n_k, g_k = (float)g[n_k]:
 *                   area = (u1-u0)(v2-v0) - (v1-v0)(u2-u0),  e1 = (u0-u2)(y-v2) - (v0-v2)(x-u2),  e2 = (u1-u0)(y-v0) - (v1-v0)(x-u0),
 *                   b1 = e1 / area, b2 = e2 / area,  gi = g0 + b1 (g1 - g0) + b2 (g2 - g0) clamped to [min g_k, max g_k] (which
 *                   changes nothing inside the triangle and bounds the band outside it), fp32, left to right; per channel the
 *                   texel becomes floor(texel + gi + 1/2) clamped to 0 .. 255.  Unowned texels, the palette block and the alpha
 *                   byte are untouched.
 * Argument errors (<0, before any launch): a null pointer where data is read or written, n < 0 or > 2^30, nnz < 0, nviews < 1,
 * lambda <= 0 or not finite, tol < 0 or not finite, iters < 0, nc < 0, texels < 0, nf < 0, big_capacity < nf, owner_in ==
 * owner_out, a vector of _level_cg not 16-byte aligned, P and npages as above. */
#define ADAMVS_TEXTURE_TILE 256
#define ADAMVS_TEXTURE_MIN_PAGE 1024
#define ADAMVS_TEXTURE_MAX_PAGE 16384
#define ADAMVS_TEXTURE_MAX_FACES 2147483647L
#define ADAMVS_TEXTURE_LEVEL_MAX_NODES (1L << 30)
#define ADAMVS_TEXTURE_LEVEL_BLOCKS 2048
#define ADAMVS_TEXTURE_LEVEL_BAND 2

int adamvs_texture_project(const adamvs_ortho_view* view, const double* xyz, long nv, float* uvz, void* stream);
int adamvs_texture_zbuf(const adamvs_ortho_view* view, const float* uvz, long nv, const unsigned* faces, long nf, unsigned* zbuf,
                        unsigned* big_count, unsigned* big_list, long big_capacity, void* stream);
int adamvs_texture_score(const adamvs_ortho_view* view, int view_index, const float* uvz, long nv, const unsigned* faces, long nf,
                         const unsigned* zbuf, float border, float tol, float* best, int* label, int* nvis, float* uv, void* stream);
int adamvs_texture_edge_keys(const unsigned* faces, long nf, long long* keys, void* stream);
int adamvs_texture_components(const long long* keys_sorted, const long long* entry, long nf, const int* label, int* parent,
                              unsigned* changed, void* stream);
int adamvs_texture_rank(const int* label, const int* parent, long nf, unsigned* block_roots, unsigned* block_untex, unsigned* root_off,
                        unsigned* untex_off, int* root_chart, int* pal, void* stream);
int adamvs_texture_boxes(const int* label, const int* parent, const int* root_chart, const float* uv, long nf, int* chart, int* box,
                         void* stream);
int adamvs_texture_fill(const adamvs_ortho_view* view, const int* items, const long long* prefix, int n, long texels, int P, long npages,
                        unsigned char* atlas, void* stream);
int adamvs_texture_coords(const int* label, const int* chart, const int* pal, const float* uv, long nf, const int* charts, int pal_ox,
                          int pal_oy, int pal_page, int P, long npages, const unsigned* faces, long nv, const unsigned char* vrgb,
                          unsigned char* atlas, float* tc, int* texnum, void* stream);
int adamvs_texture_level_observe(const long long* view_tab, int nviews, const int* rowptr, const unsigned* col, long nnz,
                                 const int* node_view, const float* pos, long n, float* f, void* stream);
int adamvs_texture_level_rhs(const int* rowptr, const unsigned* col, long nnz, const float* f, long n, double* b, void* stream);
int adamvs_texture_level_cg_init(const double* b, long n, double tol, double* g, double* r, double* p, double* partials, double* state,
                                 void* stream);
int adamvs_texture_level_cg(const int* rowptr, const unsigned* col, long nnz, long n, double lambda, int iters, double* g, double* r,
                            double* p, double* ap, double* partials, double* state, void* stream);
int adamvs_texture_level_owner(const float* uv, const int* chart, long nf, const int* charts, const long long* prefix, int nc,
                               long texels, int* owner, unsigned* big_count, unsigned* big_list, long big_capacity, void* stream);
int adamvs_texture_level_dilate(const int* charts, const long long* prefix, int nc, long texels, const int* owner_in, int* owner_out,
                                void* stream);
int adamvs_texture_level_apply(const float* uv, const int* corner_node, long nf, const double* g, long n, const int* charts,
                               const long long* prefix, int nc, long texels, const int* owner, int P, long npages,
                               unsigned char* atlas, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ADAMVS_HIP_H */
