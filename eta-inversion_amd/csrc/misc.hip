// Small kernels around the UNet body: the im2col of conv_in (the only convolution whose input channel count is not
// a multiple of 64; it runs as a K = 64 GEMM), sinusoidal timestep embedding, SiLU, weight packing, dtype casts.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace etainv {

// one thread per (row, pixel): gathers the 3x3x4 patch (zero padded) into 64 contiguous K elements
template <typename T, typename TIO>
__global__ void im2col_in_kernel(const TIO* __restrict__ x, int n_lat, int L, int rows, T* __restrict__ out) {
  const int LL = L * L;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)rows * LL) return;
  const int row = (int)(i / LL), pix = (int)(i - (int64_t)row * LL);
  const int oy = pix / L, ox = pix - oy * L;
  const TIO* xb = x + (int64_t)(row % n_lat) * 4 * LL;
  T v[64];
#pragma unroll
  for (int k = 0; k < 64; ++k) v[k] = (T)0.f;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = oy + t / 3 - 1, ix = ox + t % 3 - 1;
    if (iy >= 0 && iy < L && ix >= 0 && ix < L) {
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) v[t * 4 + ci] = from_f32<T>(to_f32(xb[(int64_t)ci * LL + iy * L + ix]));
    }
  }
  u32x4* o = reinterpret_cast<u32x4*>(out + i * 64);
#pragma unroll
  for (int q = 0; q < (int)(64 * sizeof(T) / 16); ++q) o[q] = reinterpret_cast<u32x4*>(v)[q];
}

// The timesteps travel BY VALUE in the kernel arguments (one scalar when every row shares it -- always the case in the loops -- else
// chunks of 64): no host staging buffer that a later call could overwrite before an asynchronous copy has read it.
struct TimeVec { float t[64]; };
template <typename T>
__global__ void time_embedding_kernel(TimeVec tv, int uniform, int row0, int rows, int dim, T* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * dim) return;
  const int r = i / dim, c = i - r * dim, half = dim / 2;
  const int k = c < half ? c : c - half;
  const float freq = expf(-9.210340371976184f * (float)k / (float)half);  // ln(10000)
  const float a = tv.t[uniform ? 0 : r] * freq;
  out[(int64_t)row0 * dim + i] = from_f32<T>(c < half ? cosf(a) : sinf(a));
}

template <typename T>
__global__ void silu_kernel(const T* x, T* out, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = from_f32<T>(silu_f(to_f32(x[i])));
}

// weight packing (fp32 diffusers layout -> engine layout), one thread per destination element
//   mode 0: [rows][cols] copy/cast
//   mode 1: conv OIHW [rows=O][cols=I*taps] -> [O][tap][I]
//   mode 2: GEGLU row interleave of a [rows=8c][cols] matrix: physical row p <- logical row
//           (p%64 < 32 ? (p/64)*32 + p%64 : rows/2 + (p/64)*32 + p%64 - 32)
//   mode 5: conv_in as a K = 64 GEMM: [O][4][3][3] -> [O][64], k = tap*4 + ci, k >= 36 zero   (rows = O, cols = 36)
template <typename TD>
__global__ void pack_weight_kernel(const float* __restrict__ src, TD* __restrict__ dst, int64_t rows, int64_t cols, int mode, int taps, float scale,
                                   const float* __restrict__ colscale) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (mode == 5) {
    if (i >= rows * 64) return;
    const int64_t o = i / 64, k = i - o * 64, tap = k / 4, ci = k - tap * 4;
    dst[i] = from_f32<TD>(k < 36 ? src[o * 36 + ci * 9 + tap] : 0.f);
    return;
  }
  if (i >= rows * cols) return;
  int64_t s = i;
  if (mode == 1) {
    const int64_t o = i / cols, r = i - o * cols, cin = cols / taps;
    const int64_t t = r / cin, ci = r - t * cin;
    s = o * cols + ci * taps + t;
  } else if (mode == 2) {
    const int64_t p = i / cols, c = i - p * cols;
    const int64_t blk = p / 64, within = p % 64;
    const int64_t logical = within < 32 ? blk * 32 + within : rows / 2 + blk * 32 + within - 32;
    s = logical * cols + c;
  }
  // scale: 1, or a constant folded into the weights in fp32 BEFORE the rounding (softmax scale of to_q); colscale (modes 0 / 2): a per-input-
  // column factor (the gamma of a LayerNorm folded into this Linear)
  float v = src[s] * scale;
  if (colscale) v *= colscale[s % cols];
  dst[i] = from_f32<TD>(v);
}

// LayerNorm folded into the Linear that consumes it (reference: BasicTransformerBlock norm1 -> attn1.to_q/k/v, norm2 -> attn2.to_q,
// norm3 -> ff.net.0.proj):   LN(x) W^T + b  =  rstd * (x W'^T - mean * s) + c   with  W'[n][k] = gamma[k] W[n][k]  (packed by
// pack_weight_kernel with colscale = gamma),  s[n] = sum_k W'[n][k] over the ROUNDED operand the MFMAs multiply,  c[n] = sum_k beta[k] W[n][k] + b[n].
// One wave per packed row; `mode` 0 / 2 as in pack_weight_kernel (2: GEGLU row interleave), bias already in packed order.
template <typename TD>
__global__ void __launch_bounds__(256) ln_fold_vectors_kernel(const float* __restrict__ src, const TD* __restrict__ packed, const float* __restrict__ beta,
                                                              const float* __restrict__ bias_packed, int64_t rows, int64_t cols, int mode, float scale,
                                                              float* __restrict__ s_out, float* __restrict__ c_out) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= rows) return;
  int64_t logical = p;
  if (mode == 2) {
    const int64_t blk = p / 64, within = p % 64;
    logical = within < 32 ? blk * 32 + within : rows / 2 + blk * 32 + within - 32;
  }
  float s = 0.f, c = 0.f;
  for (int64_t k = lane; k < cols; k += 64) {
    s += to_f32(packed[p * cols + k]);
    c += beta[k] * (src[logical * cols + k] * scale);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    c += __shfl_xor(c, o);
  }
  if (lane == 0) {
    s_out[p] = s;
    c_out[p] = c + (bias_packed ? bias_packed[p] : 0.f);
  }
}

template <typename TS, typename TD>
__global__ void cast_kernel(const TS* __restrict__ src, TD* __restrict__ dst, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = from_f32<TD>(to_f32(src[i]));
}

int launch_im2col_in(const void* latent, int io_dtype, int n_lat, int rows, int L, void* out, int dtype, hipStream_t s) {
  ETAINV_CHECK(latent && out && n_lat > 0 && rows > 0, "bad arguments");
  const int64_t n = (int64_t)rows * L * L;
  ETAINV_DISPATCH_DTYPE(dtype, T, ETAINV_DISPATCH_DTYPE(io_dtype, TIO,
      hipLaunchKernelGGL((im2col_in_kernel<T, TIO>), dim3(cdiv(n, 256)), dim3(256), 0, s, (const TIO*)latent, n_lat, L, rows, (T*)out)));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_time_embedding(const int64_t* t_host, int rows, int dim, void* out, int dtype, hipStream_t s) {
  ETAINV_CHECK(t_host && out && dim % 2 == 0 && rows > 0, "bad arguments");
  bool uniform = true;
  for (int i = 1; i < rows; ++i) uniform = uniform && t_host[i] == t_host[0];
  TimeVec tv;
  if (uniform) {
    tv.t[0] = (float)t_host[0];
    ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(time_embedding_kernel<T>, dim3(cdiv(rows * dim, 256)), dim3(256), 0, s, tv, 1, 0, rows, dim, (T*)out));
  } else {
    for (int r0 = 0; r0 < rows; r0 += 64) {
      const int n = std::min(64, rows - r0);
      for (int i = 0; i < n; ++i) tv.t[i] = (float)t_host[r0 + i];
      ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(time_embedding_kernel<T>, dim3(cdiv(n * dim, 256)), dim3(256), 0, s, tv, 0, r0, n, dim, (T*)out));
    }
  }
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_silu(const void* x, void* out, int64_t n, int dtype, hipStream_t s) {
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(silu_kernel<T>, dim3(cdiv(n, 256)), dim3(256), 0, s, (const T*)x, (T*)out, n));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// conv3x3 behind a nearest-2x upsample == four 2x2 convs on the SOURCE image, one per output phase (py, px) = (y & 1, x & 1): the taps of a 3x3 row / column
// that land on the same source pixel are summed.  Phase py = 0 groups kernel rows {0}, {1, 2}; py = 1 groups {0, 1}, {2} (same for columns).
// src [cout][cin][3][3] fp32 -> dst [phase = 2 py + px][cout][tap = 2 ty + tx][cin], summed in fp32, rounded once
template <typename TD>
__global__ void pack_ups4_kernel(const float* __restrict__ src, TD* __restrict__ dst, int cout, int cin) {
  const int64_t total = (int64_t)16 * cout * cin;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % cin);
  const int t = (int)((i / cin) & 3);
  const int n = (int)((i / ((int64_t)4 * cin)) % cout);
  const int ph = (int)(i / ((int64_t)4 * cin * cout));
  const int py = ph >> 1, px = ph & 1, ty = t >> 1, tx = t & 1;
  const int ky0 = py == 0 ? (ty == 0 ? 0 : 1) : (ty == 0 ? 0 : 2), ky1 = py == 0 ? (ty == 0 ? 0 : 2) : (ty == 0 ? 1 : 2);
  const int kx0 = px == 0 ? (tx == 0 ? 0 : 1) : (tx == 0 ? 0 : 2), kx1 = px == 0 ? (tx == 0 ? 0 : 2) : (tx == 0 ? 1 : 2);
  const float* w = src + ((int64_t)n * cin + c) * 9;
  float v = 0.f;
  for (int ky = ky0; ky <= ky1; ++ky)
    for (int kx = kx0; kx <= kx1; ++kx) v += w[ky * 3 + kx];
  dst[i] = from_f32<TD>(v);
}
int launch_pack_ups4(const float* src, void* dst, int cout, int cin, int dtype, hipStream_t s) {
  ETAINV_CHECK(src && dst && cout > 0 && cin > 0, "bad arguments");
  ETAINV_DISPATCH_DTYPE(dtype, TD, hipLaunchKernelGGL(pack_ups4_kernel<TD>, dim3((unsigned)cdiv((int64_t)16 * cout * cin, (int64_t)256)), dim3(256), 0, s, src, (TD*)dst, cout, cin));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_pack_weight(const float* src, void* dst, int64_t rows, int64_t cols, int mode, int taps, int dtype, hipStream_t s, float scale,
                       const float* colscale) {
  ETAINV_CHECK(src && dst && rows > 0 && cols > 0, "bad arguments");
  ETAINV_CHECK(mode == 0 || mode == 1 || mode == 2 || mode == 5, "unknown pack mode");
  ETAINV_CHECK(mode != 1 || (taps > 0 && cols % taps == 0), "conv packing: cols must be cin * taps");
  ETAINV_CHECK(mode != 2 || rows % 64 == 0, "GEGLU packing: rows must be a multiple of 64");
  ETAINV_CHECK(mode != 5 || (cols == 36 && scale == 1.0f), "conv_in packing: [O][4][3][3] sources (cols = 36), no scale");
  ETAINV_CHECK(!colscale || mode == 0 || mode == 2, "column scale: plain / GEGLU packing only");
  const int64_t n = mode == 5 ? rows * 64 : rows * cols;
  ETAINV_DISPATCH_DTYPE(dtype, TD, hipLaunchKernelGGL(pack_weight_kernel<TD>, dim3(cdiv(n, 256)), dim3(256), 0, s, src, (TD*)dst, rows, cols, mode, taps, scale,
                                                      colscale));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// GroupNorm (no activation) folded into the 1x1 conv behind it (Transformer2DModel.norm -> proj_in): per image b the conv sees
// x * a_b + sh_b with a_b[k] = rstd[b][g(k)] * gamma[k], sh_b[k] = beta[k] - mean[b][g(k)] * a_b[k], so W_b = W . diag(a_b) and c_b = W sh_b + bias.
// One wave per (image, output row n).
template <typename TD>
__global__ void __launch_bounds__(256) gn_fold_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      const float* __restrict__ bias, const float* __restrict__ stats, int groups, int n_out, int k_in,
                                                      TD* __restrict__ wb, float* __restrict__ cb) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
  if (n >= n_out) return;
  const int cpg = k_in / groups;
  const float* st = stats + (int64_t)b * groups * 2;
  float c = 0.f;
  for (int k = lane; k < k_in; k += 64) {
    const int g = k / cpg;
    const float a = st[g * 2 + 1] * gamma[k];
    const float wv = w[(int64_t)n * k_in + k];
    const TD wr = from_f32<TD>(wv * a);
    wb[((int64_t)b * n_out + n) * k_in + k] = wr;
    // the mean term against the ROUNDED operand the MFMAs multiply: a group's mean then cancels exactly, whatever its size
    c += beta[k] * wv - st[g * 2] * to_f32(wr);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) cb[(int64_t)b * n_out + n] = c + (bias ? bias[n] : 0.f);
}

int launch_gn_fold(const float* w, const float* gamma, const float* beta, const float* bias, const float* final_stats, int groups, int b, int n, int k,
                   void* wb_out, float* cb_out, int dtype, hipStream_t s) {
  ETAINV_CHECK(w && gamma && beta && final_stats && wb_out && cb_out && b > 0 && n > 0 && k > 0 && k % groups == 0, "bad arguments");
  ProfScope prof(PROF_GROUPNORM, 0.0, s);
  ETAINV_DISPATCH_HALF(dtype, TD, hipLaunchKernelGGL(gn_fold_kernel<TD>, dim3(cdiv(n, 4), b), dim3(256), 0, s, w, gamma, beta, bias, final_stats, groups, n, k,
                                                     (TD*)wb_out, cb_out));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_ln_fold(const float* w_src, const float* gamma, const float* beta, const float* bias_packed, int64_t rows, int64_t cols, int mode, float scale,
                   void* w_dst, float* s_dst, float* c_dst, int dtype, hipStream_t s) {
  ETAINV_CHECK(w_src && gamma && beta && w_dst && s_dst && c_dst && rows > 0 && cols > 0, "bad arguments");
  ETAINV_CHECK(mode == 0 || mode == 2, "plain / GEGLU packing only");
  if (launch_pack_weight(w_src, w_dst, rows, cols, mode, 1, dtype, s, scale, gamma)) return 1;
  ETAINV_DISPATCH_HALF(dtype, TD, hipLaunchKernelGGL(ln_fold_vectors_kernel<TD>, dim3(cdiv(rows, 4)), dim3(256), 0, s, w_src, (const TD*)w_dst, beta, bias_packed,
                                                     rows, cols, mode, scale, s_dst, c_dst));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// Plug-and-play feature injection (reference modules/utils/pnp_utils.py, register_conv_control_efficient): of an activation [rows][row_vecs] (16-byte
// vectors) every row r >= n_src becomes a copy of row r % n_src.  Grid-stride over the destination vectors; source rows are only read.
__global__ void __launch_bounds__(256) rows_broadcast_kernel(u32x4* x, int n_src, int64_t row_vecs, int64_t n_dst) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_dst; i += stride) {
    const int64_t r = n_src + i / row_vecs, c = i - (i / row_vecs) * row_vecs;
    x[r * row_vecs + c] = x[(r % n_src) * row_vecs + c];
  }
}

int launch_rows_broadcast(void* x, int rows, int n_src, int64_t row_elems, int dtype, hipStream_t s) {
  ETAINV_CHECK(x, "rows_broadcast: null activation");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "rows_broadcast: dtype must be f32, f16 or bf16");
  ETAINV_CHECK(rows > 0 && n_src > 0 && row_elems > 0 && rows % n_src == 0, "rows_broadcast: rows must be a positive multiple of n_src");
  const int64_t row_bytes = row_elems * (dtype == ETAINV_F32 ? 4 : 2);
  ETAINV_CHECK(row_bytes % 16 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0, "rows_broadcast: a row must be a whole number of aligned 16-byte vectors");
  if (rows == n_src) return 0;   // nothing to overwrite
  const int64_t row_vecs = row_bytes / 16, n_dst = (int64_t)(rows - n_src) * row_vecs;
  const int64_t blocks = std::min<int64_t>((n_dst + 255) / 256, 2048);
  hipLaunchKernelGGL(rows_broadcast_kernel, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<u32x4*>(x), n_src, row_vecs, n_dst);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_cast_f32(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, hipStream_t s) {
  ETAINV_DISPATCH_DTYPE(src_dtype, TS, ETAINV_DISPATCH_DTYPE(dst_dtype, TD,
      hipLaunchKernelGGL((cast_kernel<TS, TD>), dim3(cdiv(n, 256)), dim3(256), 0, s, (const TS*)src, (TD*)dst, n)));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace etainv
