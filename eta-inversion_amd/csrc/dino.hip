// The dinovitstruct metric's own kernels (reference metrics/dino_vit_structure.py): from B image pairs to B structure distances.  The DINO ViT
// tower between them runs on the GEMM / LayerNorm kernels, etainv_clip_assemble_tokens and etainv_op_vit_attention (etainv/nets.py).
// dinovitstruct_v2 (DINOv2, patch 14) takes the same preprocess kernel with a padded row stride (etainv_dinov2_preprocess: rows of 640 for
// 3 * 14^2 = 588 values, the tail written as zero) and adds etainv_op_layerscale_add_layernorm, whose kernel sits beside LayerNorm in norm.hip.
//   preprocess  grid (R / p, B): SimpleMetric._normalize, Resize(224) on a float tensor and the ImageNet normalisation (:236-241, :258-259) for
//               one band of p output rows of one image.  Per channel: the horizontal pass reads the band's input rows from global memory,
//               (x - lo) / (hi - lo) per tap, into LDS [rows][R] fp32 (never the raw rows at full width: 512 -> 224 at p = 8 spans 21 input rows);
//               the vertical pass reads LDS, and (v - mean) / std in float64, rounded once, lands in the ViT's patch rows [B g g][3 p^2],
//               k = c p^2 + py p + px.  The resampling is float: the tables (first tap, tap count, fp32 weights) come from the caller, who builds
//               them in float64 as torch's antialiased bilinear interpolation does (or its 2-tap form without antialiasing).
//   gelu_erf    the exact (erf) GELU of the DINO blocks, element-wise, on gelu_pair (common.h)
//   selfsim_mse grid (tiles (ti <= tj) of 64 x 64, B): attn_cosine_sim (:15-20) of the source's and of the edit's keys and F.mse_loss (:262) between
//               them, without writing either n x n matrix.  A pre-pass gives every key row's fp32 norm (one wave per row: a lane's terms in index
//               order, then the butterfly; the same value whatever tile uses it).  16-bit: a block computes its tile of BOTH Gram matrices on
//               mfma_f32_16x16x32 over 64-wide slabs of d staged in LDS (row stride 72 elements, as vit_attention_kernel's K tile); a wave owns
//               16 rows i and all 64 columns j, acc[t][r] = <k_(i0 + 16 w + 4 g + r), k_(j0 + 16 t + c)>.  fp32: a thread owns 4 x 4 entries on
//               plain FMA (the correctness twin).  Epilogue: acc / max(norm_i norm_j, eps) in fp32 for both, the difference and its square in
//               float64, zero where i or j >= n; one float64 partial per tile, doubled off the diagonal (the matrices are symmetric: tiles with
//               tj < ti are not launched).  A finalizer adds a pair's partials in tile order and divides by n^2.
// Order of every sum: a thread's terms in index order, a wave by the xor butterfly, the waves of a block in index order; no atomics.  A pair's
// score does not depend on B or on the pair's position and is bit-identical from run to run.
#include <cmath>

#include "kernels.h"

namespace etainv {

constexpr int DINO_THREADS = 256, DINO_WAVES = DINO_THREADS / 64;

// ------------------------------------------------------------------------------------------------------------------ preprocess
struct DinoPreParams {
  const float* x;             // [B][3][S][S]
  const int32_t* bh;          // horizontal: bounds [R][2] = (first tap, taps)
  const float* wh;            //             weights [R][ks_h]
  const int32_t* bv;          // vertical
  const float* wv;
  void* rows;                 // [B g g][ld], ld >= 3 p^2: columns 3 p^2 .. ld-1 are written as zero
  int S, R, P, ld, ks_h, ks_v, max_rows;
  float lo, span;
};

template <typename T>
__global__ void __launch_bounds__(DINO_THREADS) dino_preprocess_kernel(DinoPreParams p) {
  extern __shared__ float dino_smem[];                     // [max_rows][R]: the band's input rows of one channel after the horizontal pass
  const int S = p.S, R = p.R, P = p.P, g = R / P, K = 3 * P * P, ld = p.ld;
  const int tid = threadIdx.x, band = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int y0 = band * P, y1 = y0 + P - 1;
  // every table value is clamped where it is used: a wrong table gives wrong pixels, never an access outside the image, the tables or LDS
  const int row0 = min(max(p.bv[2 * y0], 0), S - 1);
  const int nrows = min(min(max(p.bv[2 * y1] + p.bv[2 * y1 + 1], row0 + 1), S) - row0, p.max_rows);
  // normalised in float64 and rounded once: (v - mean) cancels near the mean
  const double mean[3] = {0.485, 0.456, 0.406}, stdv[3] = {0.229, 0.224, 0.225};
  T* rows = (T*)p.rows + ((b * g + band) * g) * (int64_t)ld;
  for (int i = tid; i < g * (ld - K); i += DINO_THREADS) {            // the padding of the band's g rows
    const int patch = i / (ld - K);
    rows[(int64_t)patch * ld + K + (i - patch * (ld - K))] = from_f32<T>(0.f);
  }

  for (int c = 0; c < 3; ++c) {
    const float* src = p.x + ((b * 3 + c) * S + row0) * (int64_t)S;
    for (int i = tid; i < nrows * R; i += DINO_THREADS) {
      const int r = i / R, xo = i - r * R;
      const int x0 = p.bh[2 * xo], cnt = min(p.bh[2 * xo + 1], p.ks_h);
      const float* w = p.wh + (int64_t)xo * p.ks_h;
      const float* line = src + (int64_t)r * S;
      float acc = 0.f;
      for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], (line[min(max(x0 + j, 0), S - 1)] - p.lo) / p.span, acc);
      dino_smem[i] = acc;
    }
    __syncthreads();
    for (int i = tid; i < P * R; i += DINO_THREADS) {
      const int py = i / R, xo = i - py * R, yo = y0 + py;
      const int r0 = p.bv[2 * yo] - row0, cnt = min(p.bv[2 * yo + 1], p.ks_v);
      const float* w = p.wv + (int64_t)yo * p.ks_v;
      float acc = 0.f;
      for (int j = 0; j < cnt; ++j) acc = fmaf(w[j], dino_smem[min(max(r0 + j, 0), nrows - 1) * R + xo], acc);
      const int patch = xo / P, pxx = xo - patch * P;
      rows[(int64_t)patch * ld + (c * P + py) * P + pxx] = from_f32<T>((float)(((double)acc - mean[c]) / stdv[c]));
    }
    __syncthreads();                    // (the next channel's horizontal pass overwrites what the vertical pass reads)
  }
}

// ld: the row stride of rows_out in elements (3 p^2 for DINO; 640 for DINOv2's patch 14).  The entry points check p; everything else is checked here.
static int launch_dino_preprocess(const float* x, int b, int s, int r, int p, int ld, float lo, float hi, const int32_t* bh, const float* wh, int ks_h,
                                  const int32_t* bv, const float* wv, int ks_v, int max_rows, void* rows, int dtype, hipStream_t st) {
  ETAINV_CHECK(x && bh && wh && bv && wv && rows, "null pointer: x, the four tables and rows_out are required");
  ETAINV_CHECK((((uintptr_t)x | (uintptr_t)bh | (uintptr_t)wh | (uintptr_t)bv | (uintptr_t)wv) & 3) == 0 && ((uintptr_t)rows & 15) == 0,
               "x and the tables must be 4-byte aligned, rows_out 16-byte aligned");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(p >= 1 && ld >= 3 * p * p && (ld * (dtype == ETAINV_F32 ? 4 : 2)) % 16 == 0, "the row stride must hold 3 p^2 values and be whole 16-byte vectors");
  ETAINV_CHECK(r >= p && r % p == 0 && r <= 4096, "the resized side R must be a multiple of the patch size (at most 4096)");
  ETAINV_CHECK(b >= 0 && b <= 65535 && s >= 1 && s <= 16384, "b must be in [0, 65535] and s in [1, 16384]");
  ETAINV_CHECK(ks_h >= 1 && ks_v >= 1 && max_rows >= 1 && max_rows <= s, "tap counts and max_rows must be positive, max_rows at most s");
  ETAINV_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "input_range must be finite with hi > lo");
  const size_t lds = (size_t)max_rows * (size_t)r * sizeof(float);
  ETAINV_CHECK(lds <= 65536, "a band of p output rows needs max_rows * r * 4 bytes of LDS, at most 65536: the image is too large for this resize");
  if (b == 0) return 0;
  DinoPreParams q = {x, bh, wh, bv, wv, rows, s, r, p, ld, ks_h, ks_v, max_rows, lo, hi - lo};
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(dino_preprocess_kernel<T>, dim3(r / p, b), dim3(DINO_THREADS), lds, st, q));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ erf GELU
template <typename T>
__global__ void gelu_erf_kernel(const T* x, T* out, int64_t n) {
  const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  const bool two = i + 1 < n;
  gelu_f32x2 v;
  v[0] = to_f32(x[i]);
  v[1] = two ? to_f32(x[i + 1]) : 0.f;
  const gelu_f32x2 y = gelu_pair(v);
  out[i] = from_f32<T>(y[0]);
  if (two) out[i + 1] = from_f32<T>(y[1]);
}

// ------------------------------------------------------------------------------------------------------------------ self-similarity
constexpr int SS_TILE = 64, SS_SLAB = 64;
constexpr int SS_KS = SS_SLAB + 8;      // 16-bit slab row stride in elements (144 B: 16-byte aligned rows)
constexpr int SS_FSLAB = 32, SS_FS = SS_FSLAB + 1;   // fp32 twin: 32-wide slabs, row stride 33 floats

struct SelfSimParams {
  const void* keys;           // [2 B][n][ld]: rows 0 .. B-1 source, B .. 2B-1 edit
  const float* norms;         // [2 B][n]
  double* partials;           // [B][npairs]
  int B, n, d, nt, npairs;
  int64_t ld;
  float eps;
};

template <typename T>
__global__ void __launch_bounds__(DINO_THREADS) dino_row_norm_kernel(const T* __restrict__ keys, int64_t ld, int d, int64_t rows, float* __restrict__ norms) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * DINO_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const T* k = keys + row * ld;
  float acc = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float v = to_f32(k[i]);
    acc = fmaf(v, v, acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) norms[row] = sqrtf(acc);
}

// tile t of the upper triangle, row by row: (0, 0) (0, 1) .. (0, nt-1) (1, 1) ..
__device__ __forceinline__ void ss_tile_of(int t, int nt, int& ti, int& tj) {
  ti = 0;
  while (t >= nt - ti) {
    t -= nt - ti;
    ++ti;
  }
  tj = ti + t;
}

__device__ __forceinline__ double ss_term(float acc_s, float acc_e, float ns_i, float ns_j, float ne_i, float ne_j, bool live, float eps) {
  const float cs = acc_s / fmaxf(ns_i * ns_j, eps), ce = acc_e / fmaxf(ne_i * ne_j, eps);
  const double dlt = (double)ce - (double)cs;
  return live ? dlt * dlt : 0.0;
}

__device__ __forceinline__ void ss_store_partial(double v, bool offdiag, double* dst, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < DINO_WAVES; ++w) s += red[w];
    *dst = offdiag ? 2.0 * s : s;
  }
}

template <typename T>
__global__ void __launch_bounds__(DINO_THREADS) dino_selfsim_kernel(SelfSimParams p) {
  typedef typename ClipFrag<T>::v8 v8;
  __shared__ __attribute__((aligned(16))) T s_t[4][SS_TILE * SS_KS];     // source rows i, source rows j, edit rows i, edit rows j
  __shared__ double red[DINO_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int n = p.n;
  const int64_t ld = p.ld;
  int ti, tj;
  ss_tile_of(blockIdx.x, p.nt, ti, tj);
  const int i0 = ti * SS_TILE, j0 = tj * SS_TILE;
  const int64_t b = blockIdx.y;
  const T* src = (const T*)p.keys + b * n * ld;
  const T* edt = src + (int64_t)p.B * n * ld;

  f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int sdc = (tid & 7) * 8;                   // staging: two 16-byte pieces per thread and tile; rows >= n hold zero
  for (int k0 = 0; k0 < p.d; k0 += SS_SLAB) {
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const T* base = x < 2 ? src : edt;
      const int r0 = (x & 1) ? j0 : i0;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int row = (tid + DINO_THREADS * h) >> 3;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r0 + row < n) v = *reinterpret_cast<const u32x4*>(base + (int64_t)(r0 + row) * ld + k0 + sdc);
        *reinterpret_cast<u32x4*>(&s_t[x][row * SS_KS + sdc]) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        // A[row = key i0 + 16 wave + c][k = 32 ks + 8 g + j], B[k][col = key j0 + 16 t + c]: acc[m][t][r] = entry (16 wave + 4 g + r, 16 t + c)
        const v8 a = *reinterpret_cast<const v8*>(&s_t[2 * m][(16 * wave + c) * SS_KS + 32 * ks + 8 * g]);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const v8 bf = *reinterpret_cast<const v8*>(&s_t[2 * m + 1][(16 * t + c) * SS_KS + 32 * ks + 8 * g]);
          acc[m][t] = ClipFrag<T>::mfma(a, bf, acc[m][t]);
        }
      }
  }

  const float* ns = p.norms + b * n;
  const float* ne = ns + (int64_t)p.B * n;
  float ns_i[4], ne_i[4], ns_j[4], ne_j[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 16 * wave + 4 * g + r, j = j0 + 16 * r + c;      // (r doubles as the column tile t here)
    ns_i[r] = i < n ? ns[i] : 0.f;
    ne_i[r] = i < n ? ne[i] : 0.f;
    ns_j[r] = j < n ? ns[j] : 0.f;
    ne_j[r] = j < n ? ne[j] : 0.f;
  }
  double sum = 0.0;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool live = i0 + 16 * wave + 4 * g + r < n && j0 + 16 * t + c < n;
      sum += ss_term(acc[0][t][r], acc[1][t][r], ns_i[r], ns_j[t], ne_i[r], ne_j[t], live, p.eps);
    }
  ss_store_partial(sum, tj != ti, p.partials + b * p.npairs + blockIdx.x, red);
}

// fp32 twin: thread (ty, tx) owns entries (4 ty + r, tx + 16 q); k ascending, one FMA per term
__global__ void __launch_bounds__(DINO_THREADS) dino_selfsim_f32_kernel(SelfSimParams p) {
  __shared__ float s_t[4][SS_TILE * SS_FS];
  __shared__ double red[DINO_WAVES];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
  const int n = p.n;
  const int64_t ld = p.ld;
  int ti, tj;
  ss_tile_of(blockIdx.x, p.nt, ti, tj);
  const int i0 = ti * SS_TILE, j0 = tj * SS_TILE;
  const int64_t b = blockIdx.y;
  const float* src = (const float*)p.keys + b * n * ld;
  const float* edt = src + (int64_t)p.B * n * ld;
  float acc[2][4][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[m][r][q] = 0.f;

  for (int k0 = 0; k0 < p.d; k0 += SS_FSLAB) {
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const float* base = x < 2 ? src : edt;
      const int r0 = (x & 1) ? j0 : i0;
      for (int e = tid; e < SS_TILE * SS_FSLAB; e += DINO_THREADS) {
        const int row = e >> 5, col = e & 31;
        s_t[x][row * SS_FS + col] = r0 + row < n ? base[(int64_t)(r0 + row) * ld + k0 + col] : 0.f;
      }
    }
    __syncthreads();
    for (int k = 0; k < SS_FSLAB; ++k)
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float a[4], bb[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = s_t[2 * m][(4 * ty + r) * SS_FS + k];
#pragma unroll
        for (int q = 0; q < 4; ++q) bb[q] = s_t[2 * m + 1][(tx + 16 * q) * SS_FS + k];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[m][r][q] = fmaf(a[r], bb[q], acc[m][r][q]);
      }
  }

  const float* ns = p.norms + b * n;
  const float* ne = ns + (int64_t)p.B * n;
  double sum = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 4 * ty + r;
    const float nsi = i < n ? ns[i] : 0.f, nei = i < n ? ne[i] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + tx + 16 * q;
      const float nsj = j < n ? ns[j] : 0.f, nej = j < n ? ne[j] : 0.f;
      sum += ss_term(acc[0][r][q], acc[1][r][q], nsi, nsj, nei, nej, i < n && j < n, p.eps);
    }
  }
  ss_store_partial(sum, tj != ti, p.partials + b * p.npairs + blockIdx.x, red);
}

// a pair's partials in tile order, divided by n^2
__global__ void dino_selfsim_finalize_kernel(const double* __restrict__ partials, int npairs, int n, double* __restrict__ scores) {
  if (threadIdx.x != 0) return;
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int t = 0; t < npairs; ++t) s += partials[b * npairs + t];
  scores[b] = s / ((double)n * (double)n);
}

constexpr int SS_MAX_N = 16384;

static int64_t selfsim_partial_bytes(int b, int n) {
  const int64_t nt = cdiv(n, SS_TILE);
  return (int64_t)b * (nt * (nt + 1) / 2) * (int64_t)sizeof(double);
}

static int64_t selfsim_workspace_bytes(int b, int n) {
  if (b < 0 || b > 32767 || n < 1 || n > SS_MAX_N) {
    set_error("etainv_dino_selfsim_workspace_bytes: b must be in [0, 32767] and n in [1, 16384]");
    return -1;
  }
  return selfsim_partial_bytes(b, n) + 2 * (int64_t)b * n * (int64_t)sizeof(float);
}

static int launch_dino_selfsim(const void* keys, int b, int n, int d, int64_t ld, float eps, double* scores, float* norms_out, void* ws,
                               int64_t ws_bytes, int dtype, hipStream_t st) {
  ETAINV_CHECK(keys && scores && ws, "null pointer: keys, scores_out and workspace are required (norms_out is optional)");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(b >= 0 && b <= 32767 && n >= 1 && n <= SS_MAX_N, "b must be in [0, 32767] (2 b rows of keys) and n in [1, 16384]");
  ETAINV_CHECK(d >= 64 && d % 64 == 0 && d <= (1 << 20), "the key width d must be a multiple of 64");
  const int64_t esize = dtype == ETAINV_F32 ? 4 : 2;
  ETAINV_CHECK(ld >= d && (ld * esize) % 16 == 0, "the row stride ld must be at least d and a whole number of 16-byte vectors");
  ETAINV_CHECK(((uintptr_t)keys & 15) == 0, "keys must be 16-byte aligned");
  ETAINV_CHECK(((uintptr_t)ws & 7) == 0 && ((uintptr_t)scores & 7) == 0 && ((uintptr_t)norms_out & 3) == 0,
               "workspace and scores_out must be 8-byte aligned, norms_out 4-byte aligned");
  ETAINV_CHECK(std::isfinite(eps) && eps > 0.f, "eps must be positive: a zero key row would divide 0 by 0");
  const int64_t need = selfsim_workspace_bytes(b, n);
  ETAINV_CHECK(ws_bytes >= need, "workspace too small: see etainv_dino_selfsim_workspace_bytes");
  if (b == 0) return 0;
  const int nt = cdiv(n, SS_TILE), npairs = nt * (nt + 1) / 2;
  double* partials = (double*)ws;
  float* norms = norms_out ? norms_out : (float*)((char*)ws + selfsim_partial_bytes(b, n));
  const int64_t rows = 2 * (int64_t)b * n;
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(dino_row_norm_kernel<T>, dim3(cdiv(rows, DINO_WAVES)), dim3(DINO_THREADS), 0, st, (const T*)keys,
                                                    ld, d, rows, norms));
  ETAINV_LAUNCH_CHECK();
  SelfSimParams q = {keys, norms, partials, b, n, d, nt, npairs, ld, eps};
  if (dtype == ETAINV_F32) {
    hipLaunchKernelGGL(dino_selfsim_f32_kernel, dim3(npairs, b), dim3(DINO_THREADS), 0, st, q);
  } else {
    ETAINV_DISPATCH_HALF(dtype, T, hipLaunchKernelGGL(dino_selfsim_kernel<T>, dim3(npairs, b), dim3(DINO_THREADS), 0, st, q));
  }
  ETAINV_LAUNCH_CHECK();
  hipLaunchKernelGGL(dino_selfsim_finalize_kernel, dim3(b), dim3(64), 0, st, (const double*)partials, npairs, n, scores);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace etainv

using namespace etainv;

#define DINO_ENTRY(name, call)                                        \
  const int rc = call;                                                \
  if (rc) set_error(std::string(name ": ") + etainv_last_error());    \
  return rc

extern "C" int etainv_dino_preprocess(const float* x, int b, int s, int r, int p, float lo, float hi, const int32_t* bounds_h, const float* coef_h,
                                      int ksize_h, const int32_t* bounds_v, const float* coef_v, int ksize_v, int max_rows, void* rows_out, int dtype,
                                      void* stream) {
  if (p != 8 && p != 16) {
    set_error("etainv_dino_preprocess: patch size must be 8 or 16");
    return 1;
  }
  DINO_ENTRY("etainv_dino_preprocess", launch_dino_preprocess(x, b, s, r, p, 3 * p * p, lo, hi, bounds_h, coef_h, ksize_h, bounds_v, coef_v, ksize_v,
                                                              max_rows, rows_out, dtype, (hipStream_t)stream));
}

extern "C" int etainv_dinov2_preprocess(const float* x, int b, int s, int r, float lo, float hi, const int32_t* bounds_h, const float* coef_h, int ksize_h,
                                        const int32_t* bounds_v, const float* coef_v, int ksize_v, int max_rows, void* rows_out, int dtype,
                                        void* stream) {
  DINO_ENTRY("etainv_dinov2_preprocess", launch_dino_preprocess(x, b, s, r, 14, ETAINV_DINOV2_KP, lo, hi, bounds_h, coef_h, ksize_h, bounds_v, coef_v,
                                                                ksize_v, max_rows, rows_out, dtype, (hipStream_t)stream));
}

extern "C" int etainv_op_layerscale_add_layernorm(const void* y, const float* ls_gamma, const void* x, const float* ln_gamma, const float* ln_beta,
                                                  float eps, void* x_out, void* h_out, int rows, int c, int dtype, void* stream) {
  DINO_ENTRY("etainv_op_layerscale_add_layernorm", launch_layerscale_add_layernorm(y, ls_gamma, x, ln_gamma, ln_beta, eps, x_out, h_out, rows, c, dtype,
                                                                                   (hipStream_t)stream));
}

extern "C" int etainv_op_gelu_erf(const void* x, void* out, int64_t n, int dtype, void* stream) {
  ETAINV_CHECK(x && out, "null pointer: x and out are required");
  ETAINV_CHECK(n >= 0 && n <= ((int64_t)1 << 36), "n must be in [0, 2^36]");
  if (n == 0) return 0;
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(gelu_erf_kernel<T>, dim3(cdiv((n + 1) / 2, 256)), dim3(256), 0, (hipStream_t)stream,
                                                    (const T*)x, (T*)out, n));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t etainv_dino_selfsim_workspace_bytes(int b, int n) { return selfsim_workspace_bytes(b, n); }

extern "C" int etainv_dino_selfsim_mse(const void* keys, int b, int n, int d, int64_t ld, float eps, double* scores_out, float* norms_out,
                                       void* workspace, int64_t workspace_bytes, int dtype, void* stream) {
  DINO_ENTRY("etainv_dino_selfsim_mse", launch_dino_selfsim(keys, b, n, d, ld, eps, scores_out, norms_out, workspace, workspace_bytes, dtype,
                                                            (hipStream_t)stream));
}
