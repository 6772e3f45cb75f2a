// Internal launcher interface between the UNet executor (engine.cpp) and the kernel files.
#pragma once
#include "common.h"

namespace etainv {

// ---- igemm.hip
struct IGemmParams {
  const void* a1 = nullptr;   // activations, NHWC [B][H][W][c1]
  const void* a2 = nullptr;   // optional second source (channel concat), NHWC [B][H][W][c2]
  const void* w = nullptr;    // weights [N][taps][c1+c2]
  const float* bias = nullptr;      // [N] (physical column order)
  const float* rowvec = nullptr;    // [batch][rowvec_stride] fp32, added per batch row (time-embedding projection)
  int rowvec_stride = 0;
  int out_f32 = 0;                  // store fp32 instead of T (time-embedding projections)
  int out_nchw = 0;                 // conv_out: N == 4, store the first out_nchw channels as io-dtype NCHW [batch][out_nchw][Ho*Wo]
  int pad0 = 0;                     // 3x3 taps start at the output origin (VAE downsampler: F.pad(x,(0,1,0,1)) + stride-2 conv, no top/left pad)
  int out_io_dtype = 0;
  const void* residual = nullptr;   // [M][N]
  void* out = nullptr;              // [M][N]  (or [M][N/2] with geglu)
  const void* zeros = nullptr;      // filled in by launch_igemm
  // timing experiments only (ETAINV_IGEMM_DEBUG bit mask): 1 no DMA in the loop, 2 no epilogue, 4 no MFMA, 8 stores hit cache-resident
  // rows, 16 no young-store vmcnt allowance, 32 8-byte stores (no lane swap), 64 epilogue without its stores, 128 scalar A&S erf in GEGLU
  int debug = 0;
  // Head-major output of a fused QKV projection (round 4): out = three planes [part q|k|v][batch row][head][token][hm_dim] instead of [M][3 * heads * hm_dim],
  // so that a 64-key tile of one head is one contiguous block for the attention kernel (igemm_hm_ok says whether a launch can do it: LayerNorm
  // consumer on the 256 x 160 ring, hm_dim 40 / 80, whole tiles inside one batch row).  0 = row-major
  int hm_heads = 0, hm_dim = 0, hm_tokens = 0, hm_magic = 0;   // (hm_magic: filled in by launch_igemm)
  unsigned long* stamps = nullptr;         // diagnostic build (-DETAINV_IGEMM_STAMPS) only
  int M = 0, N = 0;
  int c1 = 0, c2 = 0;
  int H = 1, W = 1;           // source spatial dims (before the fused upsample)
  int Ho = 1, Wo = 1;         // output spatial dims
  int stride = 1, ups = 0, taps = 1;
  int ups_pm = 0;                   // ups == 2: virtual rows ordered phase-major [phase][image][source pixel] (filled in by launch_igemm: source images that are not
                                    // whole 256-row tiles -- 8 x 8, 24 x 24 -- where [image][phase][pixel] would put two phases' kernels into one tile)
  int geglu = 0;
  int xcd_gn = 1;             // XCD grid along N for the tile order (1, 2, 4 or 8; chosen by launch_igemm_t from a traffic model, see there)
  int ksplit = 1;             // split-K parts (filled in by launch_igemm for small M*N with deep K)
  float* ws = nullptr;        // [ksplit][M][N] fp32 partials
  int rows_per_batch = 1;     // Ho*Wo for convs; M/batch for linears
  // per-image operands (a GroupNorm folded into the 1x1 conv that follows it): rows of image b use w + b * w_batch_stride (elements) and
  // bias + b * bias_batch_stride; 0 = one weight matrix.  Needs rows_per_batch % (M tile) == 0.
  int64_t w_batch_stride = 0;
  int bias_batch_stride = 0;
  // ---- LayerNorm folded into the GEMM pair around it (the transformer blocks' norm1/2/3: no LayerNorm pass over HBM).
  // Producer side (the GEMM that writes the LayerNorm's input x): per row and per column chunk of the STORED (rounded) output, the pair
  // (mean, M2 = sum of squared deviations from that mean) -> stat_out[m][stat_P][2]; stat_P is chosen by launch_igemm (columns of one wave
  // tile per chunk) and reported through its stat_P argument; 0 = this launch could not emit them (the caller runs launch_row_stats).
  float* stat_out = nullptr;
  int stat_P = 0;
  // stat_kind 1: GroupNorm producer instead -- stat_out[row block][2][N]: per channel, the sum and the sum of squares of the stored output over the
  // rows of each wave tile (stat_P = rows per block, reported by launch_igemm); launch_groupnorm_pre consumes them
  int stat_kind = 0;
  // Consumer side (K = LayerNorm width, weights pre-multiplied by gamma: launch_ln_fold): out = rstd[m] * (acc - mean[m] * ln_s[n]) + bias[n],
  // bias = the folded c vector; ln_stat = (mean, rstd) per row, [M][2] (launch_ln_finalize of the producer's partials, or launch_row_stats).
  const float* ln_stat = nullptr;
  const float* ln_s = nullptr;      // [N] physical column order, like bias
};
// The two shapes every launch starts from -- the engine's and the etainv_op_* entry points' alike; what is special to a launch (residual, geglu, second
// source, time row, output form, statistics, head-major planes, per-image operands) is assigned by name on the result.
// Linear / 1x1 conv: out [M][N] = a [M][K] w[N][K]^T + bias
inline IGemmParams igemm_linear(const void* a, const void* w, const float* bias, void* out, int M, int N, int K) {
  IGemmParams p;
  p.a1 = a;
  p.w = w;
  p.bias = bias;
  p.out = out;
  p.M = M;
  p.N = N;
  p.c1 = K;
  p.H = p.Ho = 1;
  p.W = p.Wo = M;
  p.taps = 1;
  p.rows_per_batch = M;
  return p;
}
// conv3x3 over NHWC [batch][H][W][cin], pad 1: stride 1 / 2, or behind a fused nearest-2x upsample (ups)
inline IGemmParams igemm_conv3x3(const void* a, const void* w, const float* bias, void* out, int batch, int H, int W, int cin, int cout, int stride, int ups) {
  IGemmParams p;
  p.a1 = a;
  p.w = w;
  p.bias = bias;
  p.out = out;
  p.c1 = cin;
  p.H = H;
  p.W = W;
  p.Ho = ups ? H * 2 : (stride == 2 ? H / 2 : H);
  p.Wo = ups ? W * 2 : (stride == 2 ? W / 2 : W);
  p.stride = stride;
  p.ups = ups;
  p.taps = 9;
  p.M = batch * p.Ho * p.Wo;
  p.N = cout;
  p.rows_per_batch = p.Ho * p.Wo;
  return p;
}
// stat_P (optional): receives the number of partials per row written to p.stat_out (0: none written)
int launch_igemm(const IGemmParams& p, int dtype, hipStream_t s, int* stat_P = nullptr);
bool igemm_hm_ok(const IGemmParams& p, int dtype);     // may this launch (with hm_* set) write the head-major layout?
bool igemm_ups4_ok(const IGemmParams& p, int dtype);   // may this launch run the phase form (ups == 2, taps == 4) of a fused-upsample conv?
// What the calling thread's last launch_igemm chose (host-side record, no device state; etainv_op_last_igemm_plan hands it to the parity tests):
// route = index into the route names (kIGemmRouteF32: the fp32 twin; -1: no launch yet, or the launcher refused), the output tile, the K split, and
// form = 1 for ppconv's dual-M kernel / the epilogue kind 0..3 of a dual-N launch / 0 otherwise
struct IGemmPlan {
  int route = -1, bm = 0, bn = 0, ksplit = 1, form = 0;
};
constexpr int kIGemmRouteF32 = 8;
IGemmPlan& igemm_last_plan();
const char* igemm_route_name(int route);   // nullptr outside 0 .. kIGemmRouteF32

// ---- ppgemm.hip: the dual-N ping-pong GEMM; launch_igemm routes to it when pp_dualn_applicable.
// dual-N form: a 256 x 320 output tile as two 160-column halves sharing one staged activation K tile (-31 % LDS-DMA bytes per FLOP; the 1x1 GEMMs are bound
// by the DMA fill rate): bias (+ residual) (+ LayerNorm row statistics), LayerNorm consumer (row-major / head-major QKV planes), and -- as a 256 x 256 tile
// of two 128-column halves -- the LayerNorm-consumer GEGLU projection
bool pp_dualn_applicable(const IGemmParams& p, int dtype);
bool pp_dualn_hm_ok(const IGemmParams& p, int dtype);   // ... as a LayerNorm consumer that writes the head-major QKV planes (hm_* set)?
int launch_pp_dualn(const IGemmParams& p, int dtype, hipStream_t s, int* stat_P = nullptr);

// ---- ppconv.hip: conv3x3 stride 1 in PATCH form (16 x 16 pixel tiles, halo'd activation patch per channel chunk) with the wave groups in anti-phase and a
// lean issue side; bias + time row + residual + GroupNorm-statistics epilogues; launch_igemm routes to it when pp_conv_applicable
bool pp_conv_applicable(const IGemmParams& p, int dtype);
int launch_pp_conv(const IGemmParams& p, int dtype, hipStream_t s, int* stat_P = nullptr);

// ---- f32path.hip: the fp32-operand execution (dtype == ETAINV_F32 routes here from the launchers of igemm / norm / attention)
int launch_igemm_f32(const IGemmParams& p, hipStream_t s);
int launch_groupnorm_f32(const void* x1, const void* x2, int c1, int c2, const float* gamma, const float* beta, void* out, int b, int hw, int groups,
                         float eps, int silu, float* scratch, hipStream_t s);
int launch_layernorm_f32(const void* x, const float* gamma, const float* beta, void* out, int rows, int c, float eps, hipStream_t s);
int launch_self_attention_f32(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img, hipStream_t s, int first_row = 0);
struct CrossParams;
int launch_cross_attention_f32(const void* q, const void* kv, void* out, int b, int d, const CrossParams& p, hipStream_t s);

// ---- norm.hip
// GroupNorm(32 groups) over NHWC with optional second (concatenated) source and fused SiLU.
// scratch: >= b * GN_CHUNKS_MAX * groups * 2 floats
constexpr int GN_MAX_CHUNKS = 64;
int launch_groupnorm(const void* x1, const void* x2, int c1, int c2, const float* gamma, const float* beta, void* out,
                     int b, int hw, int groups, float eps, int silu, float* scratch, int dtype, hipStream_t s);
// GroupNorm whose statistics arrive as per-channel partials from the epilogues of the GEMMs that wrote x1 / x2 (IGemmParams::stat_kind 1; part =
// [b * hw / wm][2][c] floats): a finalize launch (sums in double, fixed order) -> final_stats = [b][groups][2] (mean, rstd) followed by the apply
// pass's per-channel scale / shift planes [b][2][c1 + c2] (the buffer holds b * (2 * groups + 2 * C) floats), then the apply pass of launch_groupnorm
int launch_groupnorm_pre(const void* x1, const void* x2, int c1, int c2, const float* part1, int wm1, const float* part2, int wm2, const float* gamma,
                         const float* beta, void* out, int b, int hw, int groups, float eps, int silu, float* final_stats, int dtype, hipStream_t s);
// the finalize half of launch_groupnorm_pre alone: final_stats[b][groups] = (mean, rstd)
int launch_gn_finalize(int c1, int c2, const float* part1, int wm1, const float* part2, int wm2, int b, int hw, int groups, float eps, float* final_stats,
                       hipStream_t s, const float* gamma = nullptr, const float* beta = nullptr, float* scsh = nullptr);
// GroupNorm (no activation) folded into the 1x1 conv / Linear W [n][k] that follows it: per image b, W_b[n][k] = W[n][k] * rstd[b][g(k)] * gamma[k]
// (rounded to the compute dtype) and c_b[n] = sum_k (beta[k] - mean[b][g(k)] * rstd * gamma[k]) * W[n][k] + bias[n]
int launch_gn_fold(const float* w, const float* gamma, const float* beta, const float* bias, const float* final_stats, int groups, int b, int n, int k,
                   void* wb_out, float* cb_out, int dtype, hipStream_t s);
int launch_layernorm(const void* x, const float* gamma, const float* beta, void* out, int rows, int c, float eps, int dtype,
                     hipStream_t s);
// x_out = round(x + ls_gamma * y) (optional store) and h_out = LayerNorm(x_out as stored), one wave per row; fp16, bf16 and fp32
int launch_layerscale_add_layernorm(const void* y, const float* ls_gamma, const void* x, const float* ln_gamma, const float* ln_beta, float eps, void* x_out,
                                    void* h_out, int rows, int c, int dtype, hipStream_t s);
// stat[row] = (mean, rstd) of x[row][0..c): IGemmParams::ln_stat computed by a pass over x (when the producing GEMM could not emit partials)
int launch_row_stats(const void* x, float* stat, int rows, int c, float eps, int dtype, hipStream_t s);
// partials[row][P] (mean, M2) pairs over cw columns each (IGemmParams::stat_out) -> stat[row] = (mean, rstd); Chan's update in index order
int launch_ln_finalize(const float* partials, int P, int cw, float eps, float* stat, int rows, hipStream_t s);

// ---- attention.hip
// self-attention modes: 0 plain; 1 ptp self-replace (cond target rows use Q,K of their source row);
// 2 masactrl (target rows use K,V of their source row).  Modes 1/2 need the 4*n_img backward row layout.
// 16-bit launches of head_dim 40 / 80: their kernels take pre-scaled queries (the engine folds softmax scale * log2(e) into the to_q weights) and head-major
// QKV planes (IGemmParams::hm_*).  head_dim 160 and fp32 take neither.  (Rounds 1-6 kept a generic 16x16x32 kernel behind A/B switches; it lost every A/B and is gone.)
inline bool self_attn_prescaled_hm_ok(int d, int dtype) { return dtype != ETAINV_F32 && (d == 40 || d == 80); }
// q_prescaled: the queries already carry softmax scale * log2(e); head_major: qkv holds three head-major planes (both: self_attn_prescaled_hm_ok launches only)
// first_row: the call carries rows [first_row, 4 n_img) of the [u_s, u_t, c_s, c_t] x n_img layout (0, or n_img when the uncond source rows are left out:
// backward steps with eta == 0, etainv/pipeline.py)
int launch_self_attention_mode(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img, int dtype,
                               hipStream_t s, int q_prescaled = 0, int first_row = 0, int head_major = 0);
struct CrossParams {
  int N = 0, heads = 8, n_ctx = 77;
  float scale_log2 = 0.f;
  int layout = 0;      // 0: no roles (plain); 1: forward store layout [u x B, c x B] or [c x B]; 2: backward 4B layout
  int n_img = 1;
  int rows = 0;        // batch rows in this call
  int first_row = 0;   // layout 2: the call carries rows [first_row, 4 n_img) of [u_s, u_t, c_s, c_t] x n_img (0 or n_img)
  int edit = 0;        // ptp cross edit on cond target rows
  int map_layer = -1;  // >= 0: accumulate cond-half probabilities into maps_acc layer `map_layer`
  int n_img_cap = 1;
  const int32_t* mapper = nullptr;
  const float* alphas = nullptr;
  const float* replace_mat = nullptr;
  const float* equalizer = nullptr;
  const float* cross_alpha = nullptr;
  float* maps_acc = nullptr;
  int xcd_gx = 0;      // > 0: 1-D grid with the heads of one (row, query range) on one XCD; the value = query-block lanes per (row, head) (attention.hip)
};
// What an etainv_attn_ctrl means for a cross-attention launch: row layout, image count, first row and the prompt-to-prompt edit tables.  The one
// definition for the UNet's transformer blocks and for etainv_op_cross_attention (the map store -- map_layer, maps_acc, n_img_cap -- is the caller's).
inline void cross_params_from_ctrl(CrossParams& cp, const etainv_attn_ctrl* ctrl) {
  if (!ctrl || (ctrl->mode != ETAINV_ATTN_PTP && ctrl->mode != ETAINV_ATTN_STORE)) return;
  const bool ptp = ctrl->mode == ETAINV_ATTN_PTP;
  cp.n_img = ctrl->n_img;
  cp.layout = ptp ? (ctrl->src_exit_block ? 3 : 2) : 1;   // 3: rows [u_t, c_t, c_s] (cond source rows leave early)
  cp.first_row = ptp ? ctrl->first_row : 0;
  if (ptp && (ctrl->mapper || ctrl->replace_mat)) {   // (without cross_alpha: the launcher's refusal, not a silently skipped edit)
    cp.edit = 1;
    cp.mapper = ctrl->mapper;
    cp.alphas = ctrl->alphas;
    cp.replace_mat = ctrl->replace_mat;
    cp.equalizer = ctrl->equalizer;
    cp.cross_alpha = ctrl->cross_alpha;
  }
}
// Refuses (before any launch, 16-bit and fp32 alike) a row count that does not fit the layout -- layout 1: b in {n_img, 2 n_img}; layout 2: first_row in
// {0, n_img} and b + first_row == 4 n_img; layout 3: b in {2 n_img, 3 n_img} --, an edit without cross_alpha, a store without maps_acc or with n_img > n_img_cap.
int launch_cross_attention_p(const void* q, const void* kv, void* out, int b, int d, const CrossParams& p, int dtype, hipStream_t s);

// ---- misc.hip
// im2col of the 3x3 / 4-channel input conv: NCHW io-dtype latent [n_lat][4][L][L] (row r reads r % n_lat) -> T [rows][L*L][64] (k = tap*4 + ci, 36..63 zero)
int launch_im2col_in(const void* latent, int io_dtype, int n_lat, int rows, int L, void* out, int dtype, hipStream_t s);
// sinusoidal timestep embedding (flip_sin_to_cos, freq_shift 0): t_host [rows] (HOST array, passed by value in the kernel arguments) -> [rows][dim] T
int launch_time_embedding(const int64_t* t_host, int rows, int dim, void* out, int dtype, hipStream_t s);
// y = silu(x) elementwise on T
int launch_silu(const void* x, void* out, int64_t n, int dtype, hipStream_t s);
// cast fp32 -> T with optional row permutation (weights): the `mode` of launch_pack_weight / launch_ln_fold
enum PackMode { PK_PLAIN = 0, PK_CONV = 1, PK_GEGLU = 2, PK_CONV_IN_GEMM = 5 };   // (3 and 4 were the direct conv_in / conv_out kernels' layouts: retired)
int launch_pack_ups4(const float* src, void* dst, int cout, int cin, int dtype, hipStream_t s);   // conv3x3 weights -> four 2x2 phase kernels (IGemmParams::ups == 2)
int launch_pack_weight(const float* src, void* dst, int64_t rows, int64_t cols, int mode, int taps, int dtype, hipStream_t s, float scale = 1.0f,
                       const float* colscale = nullptr);
// LayerNorm(gamma, beta) folded into the Linear (w_src [rows][cols] fp32, pack mode 0 / 2) that consumes it: packed operand W' = gamma . W, the
// row sums s of the rounded W' and c = beta W^T + bias (bias_packed may be null) -- see IGemmParams::ln_stat
int launch_ln_fold(const float* w_src, const float* gamma, const float* beta, const float* bias_packed, int64_t rows, int64_t cols, int mode, float scale,
                   void* w_dst, float* s_dst, float* c_dst, int dtype, hipStream_t s);
int launch_cast_f32(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t s);
// activation [rows][row_elems], rows % n_src == 0: every row r >= n_src becomes a copy of row r % n_src (plug-and-play feature injection); a row must be
// a whole number of 16-byte vectors
int launch_rows_broadcast(void* x, int rows, int n_src, int64_t row_elems, int dtype, hipStream_t s);

// ---- proximal.hip
// etainv_prox_guidance (include/etainv.h) behind its stream cast: every refusal is made here, before anything touches the device
int launch_prox_guidance(const float* eps_u, const float* eps_c, float g, int mode, int use_rank, int rank_lo, float rank_w, float thr_fixed,
                         float* eps_out, const float* x, float a_from, float a_to, float* x_out, float* thr_out, int n_groups, int rows_per_group,
                         int l, hipStream_t s);

// ---- metrics.hip
// etainv_image_metrics (include/etainv.h) behind its stream cast: every refusal is made here, before anything touches the device
int launch_image_metrics(const float* pred, const float* target, int b, int h, int w, float lo, float hi, int mask, float* out, void* workspace,
                         int64_t workspace_bytes, hipStream_t s);

// ---- clip.hip, dino.hip: the 16x16x32 MFMA of either 16-bit operand type behind one name (A[row = lane & 15][k = 8 (lane >> 4) + j],
// B[k][col = lane & 15], C[row = 4 (lane >> 4) + r][col = lane & 15])
template <typename T> struct ClipFrag;
template <> struct ClipFrag<f16> {
  typedef f16x8 v8;
  typedef f16x4 v4;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
};
template <> struct ClipFrag<bf16> {
  typedef bf16x8 v8;
  typedef bf16x4 v4;
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
};

// ---- maps.hip
int launch_word_maps(const float* maps_acc, int n_layers, int n_img_cap, int rows_per_img, int row_sel, int heads, int res, int L,
                     int n_img, const int32_t* tokens, int n_tok, int steps_done, float* out, int accumulate, float scale,
                     hipStream_t s, unsigned layer_mask = ~0u);
int launch_local_blend(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, float* x, int n_img,
                       const float* blend_alpha, float thres, hipStream_t s);

}  // namespace etainv
