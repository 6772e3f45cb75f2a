// Per-op entry points of libetainv_hip.so (etainv_op_*): single launches for the parity tests, in the forms the engine launches them.  The GEMM and
// conv forms start from the same two builders as the engine's (kernels.h: igemm_linear, igemm_conv3x3) and name what is special to each.
#include <cmath>

#include "common.h"
#include "kernels.h"

using namespace etainv;

extern "C" int etainv_op_gemm(const void* a, const void* w, const void* bias, const void* residual, void* out, int m, int n, int k,
                              int geglu, int dtype, void* stream) {
  IGemmParams p = igemm_linear(a, w, (const float*)bias, out, m, n, k);
  p.residual = residual;
  p.geglu = geglu;
  return launch_igemm(p, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_gemm_ln(const void* a, const void* w_folded, const float* c_vec, const float* s_vec, const float* stat,
                                 const void* residual, void* out, float* stat_out, int* stat_p_out, int m, int n, int k, int geglu,
                                 int dtype, void* stream) {
  IGemmParams p = igemm_linear(a, w_folded, c_vec, out, m, n, k);
  p.residual = residual;
  p.geglu = geglu;
  if (stat) {
    p.ln_stat = stat;
    p.ln_s = s_vec;
  }
  p.stat_out = stat_out;
  return launch_igemm(p, dtype, (hipStream_t)stream, stat_p_out);
}

// the fused QKV projection as transformer() launches it: head-major planes [q|k|v][row][head][token][head_dim] when igemm_hm_ok allows (*wrote_head_major = 1),
// the row-major LayerNorm-consumer GEMM of etainv_op_gemm_ln otherwise (0)
extern "C" int etainv_op_gemm_ln_hm(const void* a, const void* w_folded, const float* c_vec, const float* s_vec, const float* stat, void* out, int m, int n,
                                    int k, int heads, int head_dim, int tokens, int* wrote_head_major, int dtype, void* stream) {
  ETAINV_CHECK(stat && s_vec && c_vec && wrote_head_major, "the LayerNorm-consumer GEMM needs stat, s_vec, c_vec and wrote_head_major");
  IGemmParams p = igemm_linear(a, w_folded, c_vec, out, m, n, k);
  p.ln_stat = stat;
  p.ln_s = s_vec;
  *wrote_head_major = 0;
  if (self_attn_prescaled_hm_ok(head_dim, dtype)) {
    IGemmParams q = p;
    q.hm_heads = heads;
    q.hm_dim = head_dim;
    q.hm_tokens = tokens;
    if (igemm_hm_ok(q, dtype)) {
      *wrote_head_major = 1;
      return launch_igemm(q, dtype, (hipStream_t)stream);
    }
  }
  return launch_igemm(p, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_gemm_gnstat(const void* a, const void* w, const float* bias, const void* residual, void* out, float* part, int* wm_out, int m,
                                     int n, int k, int rows_per_image, int dtype, void* stream) {
  IGemmParams p = igemm_linear(a, w, bias, out, m, n, k);
  p.residual = residual;
  p.rows_per_batch = rows_per_image;
  p.stat_out = part;
  p.stat_kind = 1;
  return launch_igemm(p, dtype, (hipStream_t)stream, wm_out);
}

extern "C" int etainv_op_conv3x3_gnstat(const void* x_nhwc, const void* w_okkc, const float* bias, const float* rowvec, const void* residual, void* out,
                                        float* part, int* wm_out, int b, int h, int wd, int cin, int cout, int dtype, void* stream) {
  IGemmParams p = igemm_conv3x3(x_nhwc, w_okkc, bias, out, b, h, wd, cin, cout, /*stride=*/1, /*ups=*/0);
  p.rowvec = rowvec;
  p.rowvec_stride = cout;
  p.residual = residual;
  p.stat_out = part;
  p.stat_kind = 1;
  return launch_igemm(p, dtype, (hipStream_t)stream, wm_out);
}

extern "C" int etainv_op_groupnorm_pre(const void* x1, const void* x2, int c1, int c2, const float* part1, int wm1, const float* part2, int wm2,
                                       const float* gamma, const float* beta, void* out, int b, int hw, int groups, float eps, int silu,
                                       float* final_stats, int dtype, void* stream) {
  return launch_groupnorm_pre(x1, x2, c1, c2, part1, wm1, part2, wm2, gamma, beta, out, b, hw, groups, eps, silu, final_stats, dtype,
                              (hipStream_t)stream);
}

extern "C" int etainv_op_ln_fold(const float* w, const float* gamma, const float* beta, const float* bias, int n, int k, int geglu, float scale,
                                 void* w_out, float* s_out, float* c_out, int dtype, void* stream) {
  const int mode = geglu ? PK_GEGLU : PK_PLAIN;
  // the bias goes through the same row permutation as the weight (into c_out, which the fold then reads and overwrites element by element)
  if (bias && launch_pack_weight(bias, c_out, n, 1, mode, 1, ETAINV_F32, (hipStream_t)stream)) return 1;
  return launch_ln_fold(w, gamma, beta, bias ? c_out : nullptr, n, k, mode, scale, w_out, s_out, c_out, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_row_stats(const void* x, float* stat, int rows, int c, float eps, int dtype, void* stream) {
  return launch_row_stats(x, stat, rows, c, eps, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_ln_finalize(const float* partials, int p, int cw, float eps, float* stat, int rows, void* stream) {
  return launch_ln_finalize(partials, p, cw, eps, stat, rows, (hipStream_t)stream);
}

extern "C" int etainv_op_conv3x3_ex(const void* x_nhwc, const void* w_okkc, const void* bias, const void* residual, void* out, int b, int h,
                                    int wd, int cin, int cout, int stride, int upsample, int pad0, int out_nchw, int out_io_dtype,
                                    int dtype, void* stream) {
  IGemmParams p = igemm_conv3x3(x_nhwc, w_okkc, (const float*)bias, out, b, h, wd, cin, cout, stride, upsample);
  p.residual = residual;
  p.pad0 = pad0;
  p.out_nchw = out_nchw;
  p.out_io_dtype = out_io_dtype;
  return launch_igemm(p, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_pack_ups4(const float* w_oc33, void* dst, int cout, int cin, int dtype, void* stream) {
  return launch_pack_ups4(w_oc33, dst, cout, cin, dtype, (hipStream_t)stream);
}

// conv3x3 (+ second source, fused upsample, stride 2) with the time row read the way the UNet reads it: rowvec points at this layer's columns inside the
// [b][rowvec_stride] fp32 matrix of all time projections
extern "C" int etainv_op_conv3x3_rv(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const void* w_okkc, const void* bias,
                                    const float* rowvec, int rowvec_stride, const void* residual, void* out, int b, int h, int wd, int cout,
                                    int stride, int upsample, int taps, int dtype, void* stream) {
  ETAINV_CHECK(!rowvec || rowvec_stride >= cout, "rowvec_stride must cover the cout columns of a row");
  IGemmParams p = igemm_conv3x3(x_nhwc, w_okkc, (const float*)bias, out, b, h, wd, c1, cout, stride, upsample);
  p.a2 = x2_nhwc;
  p.c2 = c2;
  p.rowvec = rowvec;
  p.rowvec_stride = rowvec_stride;
  p.residual = residual;
  p.taps = taps;
  return launch_igemm(p, dtype, (hipStream_t)stream);
}
// the time row as its own dense [b][cout] matrix
extern "C" int etainv_op_conv3x3(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const void* w_okkc, const void* bias,
                                 const float* rowvec, const void* residual, void* out, int b, int h, int wd, int cout, int stride,
                                 int upsample, int taps, int dtype, void* stream) {
  return etainv_op_conv3x3_rv(x_nhwc, x2_nhwc, c1, c2, w_okkc, bias, rowvec, cout, residual, out, b, h, wd, cout, stride, upsample, taps, dtype, stream);
}

extern "C" int etainv_op_groupnorm(const void* x_nhwc, const void* x2_nhwc, int c1, int c2, const float* gamma, const float* beta,
                                   void* out, int b, int hw, int groups, float eps, int silu, float* scratch, int dtype, void* stream) {
  return launch_groupnorm(x_nhwc, x2_nhwc, c1, c2, gamma, beta, out, b, hw, groups, eps, silu, scratch, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_layernorm(const void* x, const float* gamma, const float* beta, void* out, int rows, int c, float eps, int dtype,
                                   void* stream) {
  return launch_layernorm(x, gamma, beta, out, rows, c, eps, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_self_attention(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img, int dtype,
                                        void* stream) {
  return launch_self_attention_mode(qkv, out, b, n, heads, d, mode, n_img, dtype, (hipStream_t)stream);
}

// every argument of the launcher (the engine's form: q_prescaled = 1 at head_dim 40 / 80, head-major planes, the three-row layouts through first_row)
extern "C" int etainv_op_self_attention_ex(const void* qkv, void* out, int b, int n, int heads, int d, int mode, int n_img, int q_prescaled, int first_row,
                                           int head_major, int dtype, void* stream) {
  return launch_self_attention_mode(qkv, out, b, n, heads, d, mode, n_img, dtype, (hipStream_t)stream, q_prescaled, first_row, head_major);
}

extern "C" int etainv_op_rows_broadcast(void* x, int rows, int n_src, int64_t row_elems, int dtype, void* stream) {
  return launch_rows_broadcast(x, rows, n_src, row_elems, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_cross_attention(const void* q, const void* kv, void* out, int b, int n, int heads, int d, int n_ctx,
                                         const etainv_attn_ctrl* ctrl, int map_layer, int n_img_cap, float* maps_acc, int dtype,
                                         void* stream) {
  CrossParams cp;
  cp.N = n;
  cp.heads = heads;
  cp.n_ctx = n_ctx;
  cp.scale_log2 = (1.0f / std::sqrt((float)d)) * 1.4426950408889634f;
  cp.rows = b;
  cp.n_img_cap = n_img_cap;
  cp.maps_acc = maps_acc;
  cross_params_from_ctrl(cp, ctrl);
  if (cp.layout && ctrl->store_maps && map_layer >= 0) cp.map_layer = map_layer;   // (without maps_acc: the launcher's refusal, not a silent loss of maps)
  return launch_cross_attention_p(q, kv, out, b, d, cp, dtype, (hipStream_t)stream);
}

// the GEMM of all time-embedding projections as etainv_unet_forward launches it: fp32 output [m][n]
extern "C" int etainv_op_gemm_f32out(const void* a, const void* w, const float* bias, float* out_f32, int m, int n, int k, int dtype, void* stream) {
  IGemmParams p = igemm_linear(a, w, bias, out_f32, m, n, k);
  p.out_f32 = 1;
  return launch_igemm(p, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_gn_fold(const float* w, const float* gamma, const float* beta, const float* bias, const float* stats, int groups, int b, int n,
                                 int k, void* wb_out, float* cb_out, int dtype, void* stream) {
  return launch_gn_fold(w, gamma, beta, bias, stats, groups, b, n, k, wb_out, cb_out, dtype, (hipStream_t)stream);
}

// the 1x1 conv behind a folded GroupNorm (per-image operands): image i (hw rows) multiplies wb[i] [n][k] and adds cb[i] [n]
extern "C" int etainv_op_gemm_per_image(const void* a, const void* wb, const float* cb, const void* residual, void* out, int b, int hw, int n, int k,
                                        int dtype, void* stream) {
  ETAINV_CHECK(b > 0 && hw > 0, "bad sizes");
  IGemmParams p = igemm_linear(a, wb, cb, out, b * hw, n, k);
  p.residual = residual;
  p.rows_per_batch = hw;
  p.w_batch_stride = (int64_t)n * k;
  p.bias_batch_stride = n;
  return launch_igemm(p, dtype, (hipStream_t)stream);
}

// the route, tile and K split of this thread's last launch_igemm (kernels.h: IGemmPlan); no device state, no launch
extern "C" int etainv_op_last_igemm_plan(int* out, int n) {
  const IGemmPlan& plan = igemm_last_plan();
  const int v[5] = {plan.route, plan.bm, plan.bn, plan.ksplit, plan.form};
  for (int i = 0; i < 5 && i < n; ++i) out[i] = v[i];
  return 5;
}
extern "C" const char* etainv_op_igemm_route_name(int route) { return igemm_route_name(route); }

// timesteps by value in the kernel arguments
extern "C" int etainv_op_time_embedding(const int64_t* t_host, int rows, int dim, void* out, int dtype, void* stream) {
  return launch_time_embedding(t_host, rows, dim, out, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_silu(const void* x, void* out, int64_t n, int dtype, void* stream) {
  ETAINV_CHECK(x && out && n >= 0, "null pointer or negative size");
  if (n == 0) return 0;
  return launch_silu(x, out, n, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream) {
  ETAINV_CHECK(src && dst && n >= 0, "null pointer or negative size");
  if (n == 0) return 0;
  return launch_cast_f32(src, src_dtype, dst, dst_dtype, n, (hipStream_t)stream);
}

extern "C" int etainv_op_im2col_in(const void* latent, int io_dtype, int n_lat, int rows, int l, void* out, int dtype, void* stream) {
  ETAINV_CHECK(l > 0, "bad sizes");
  return launch_im2col_in(latent, io_dtype, n_lat, rows, l, out, dtype, (hipStream_t)stream);
}

extern "C" int etainv_op_pack_weight(const float* src, void* dst, int64_t rows, int64_t cols, int mode, int taps, float scale, const float* colscale,
                                     int dtype, void* stream) {
  return launch_pack_weight(src, dst, rows, cols, mode, taps, dtype, (hipStream_t)stream, scale, colscale);
}

extern "C" int etainv_op_word_maps_ex(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, int n_img, const int32_t* tokens,
                                      int n_tok, int steps_done, int row_sel, unsigned layer_mask, float* out, int accumulate, float scale, void* stream) {
  ETAINV_CHECK(row_sel == 0 || row_sel == 1, "row_sel: 0 = source cond row, 1 = target cond row");
  ETAINV_CHECK(n_img <= n_img_cap && heads > 0 && res > 0 && L > 0, "bad sizes");
  return launch_word_maps(maps_acc, n_layers, n_img_cap, 2, row_sel, heads, res, L, n_img, tokens, n_tok, steps_done, out, accumulate, scale,
                          (hipStream_t)stream, layer_mask);
}

extern "C" int etainv_op_word_maps(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, int n_img,
                                   const int32_t* tokens, int n_tok, int steps_done, float* out, int accumulate, float scale,
                                   void* stream) {
  return launch_word_maps(maps_acc, n_layers, n_img_cap, 2, 0, heads, res, L, n_img, tokens, n_tok, steps_done, out, accumulate, scale,
                          (hipStream_t)stream);
}

extern "C" int etainv_op_local_blend(const float* maps_acc, int n_layers, int n_img_cap, int heads, int res, int L, float* x, int n_img,
                                     const float* blend_alpha, float thres, void* stream) {
  return launch_local_blend(maps_acc, n_layers, n_img_cap, heads, res, L, x, n_img, blend_alpha, thres, (hipStream_t)stream);
}
