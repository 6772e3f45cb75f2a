// The CLIP metrics' own kernels (reference metrics/clip_similarity.py): from B image pairs and their prompts to B scores.
//   preprocess   grid (R / p, B): torch_to_pil (:223-239) + clip's transform (:201) for one band of p output rows of one image.  Per channel: the
//                input rows the band needs become uint8 in LDS ((x - lo) / (hi - lo), * 255, clamped, TRUNCATED), Pillow's horizontal bicubic pass
//                writes them as uint8 again, the vertical pass gives the resized byte, and / 255, - mean, / std (float64, rounded once) lands in the ViT's patch rows
//                [B g g][Kp], k = c p^2 + py p + px, zero from 3 p^2 to Kp.  The resampling is integer: the coefficient tables (first tap, tap count,
//                weights in 22-bit fixed point) come from the caller, who builds them in float64 as Pillow does.
//   assemble     [B][1 + g^2][d] = (class token | patch GEMM output) + position embedding
//   attention    grid (query tiles of 64, heads, B): non-causal flash attention at head_dim 64 for any n.  16-bit: a wave owns 16 queries; a 32-key
//                tile of K (row-major) and V (transposed) is staged in LDS, zero beyond n.  S^T = K Q^T on mfma_16x16x32 leaves a query on the lane
//                (lane & 15) and four keys per 16-key tile in its registers, which IS the B operand of O^T = V^T P^T when k slot (lane >> 4, j) means
//                key 4 (lane >> 4) + j (j < 4) or 16 + 4 (lane >> 4) + j - 4: V^T is read from LDS in that key order, no lane movement, no P in LDS.
//                Online softmax in fp32 on exp2 with scale * log2(e) folded into the argument; P is rounded to the operand type and the denominator
//                sums the rounded values.  fp32: one query per thread on plain FMA (the correctness twin).
//   embed head   grid (B): the pooled token's row -> optional LayerNorm -> bias-free projection [P][d] -> L2 normalisation, fp32 [B][P]
//   similarity   grid (B): the four scores from the unit embeddings, float64
// Order of every sum: a thread's terms in index order, a wave by the xor butterfly, the waves of a block in index order; no atomics.  A row's
// result does not depend on B or on the row's position and is bit-identical from run to run.
#include <cmath>

#include "kernels.h"

namespace etainv {

constexpr int CLIP_THREADS = 256, CLIP_WAVES = CLIP_THREADS / 64;

// ------------------------------------------------------------------------------------------------------------------ preprocess
struct ClipPreParams {
  const float* x;             // [B][3][S][S]
  const int32_t *bh, *ch;     // horizontal: bounds [R][2] = (first tap, taps), weights [R][ks_h]
  const int32_t *bv, *cv;     // vertical
  void* rows;                 // [B g g][Kp]
  uint8_t* u8;                // [B][3][R][R] or null
  int S, R, P, Kp, ks_h, ks_v, max_rows;
  float lo, span;
};

__device__ __forceinline__ uint8_t clip8(int v) { return (uint8_t)min(max(v >> 22, 0), 255); }

template <typename T>
__global__ void __launch_bounds__(CLIP_THREADS) clip_preprocess_kernel(ClipPreParams p) {
  extern __shared__ uint8_t clip_smem[];
  const int S = p.S, R = p.R, P = p.P, g = R / P;
  uint8_t* s_in = clip_smem;                               // [max_rows][S]: the band's input rows of one channel, uint8
  uint8_t* s_h = clip_smem + (size_t)p.max_rows * S;       // [max_rows][R]: ... after the horizontal pass
  const int tid = threadIdx.x, band = blockIdx.x;
  const int64_t b = blockIdx.y;
  const int y0 = band * P, y1 = y0 + P - 1;
  // every table value is clamped where it is used: a wrong table gives wrong pixels, never an access outside the image, the tables or LDS
  const int row0 = min(max(p.bv[2 * y0], 0), S - 1);
  const int nrows = min(min(max(p.bv[2 * y1] + p.bv[2 * y1 + 1], row0 + 1), S) - row0, p.max_rows);
  // normalised in float64 and rounded once: (px / 255 - mean) cancels near the mean, where three fp32 roundings would cost many ulp of the result
  const double mean[3] = {0.48145466, 0.4578275, 0.40821073}, stdv[3] = {0.26862954, 0.26130258, 0.27577711};
  T* rows = (T*)p.rows + ((b * g + band) * g) * (int64_t)p.Kp;

  for (int c = 0; c < 3; ++c) {
    const float* src = p.x + ((b * 3 + c) * S + row0) * (int64_t)S;
    for (int i = tid; i < nrows * S; i += CLIP_THREADS) {
      const float v = (src[i] - p.lo) / p.span;
      s_in[i] = (uint8_t)(int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f);
    }
    __syncthreads();
    for (int i = tid; i < nrows * R; i += CLIP_THREADS) {
      const int r = i / R, xo = i - r * R;
      const int x0 = p.bh[2 * xo], cnt = min(p.bh[2 * xo + 1], p.ks_h);
      const int32_t* w = p.ch + (int64_t)xo * p.ks_h;
      int acc = 1 << 21;
      for (int j = 0; j < cnt; ++j) acc += w[j] * (int)s_in[r * S + min(max(x0 + j, 0), S - 1)];
      s_h[i] = clip8(acc);
    }
    __syncthreads();
    for (int i = tid; i < P * R; i += CLIP_THREADS) {
      const int py = i / R, xo = i - py * R, yo = y0 + py;
      const int r0 = p.bv[2 * yo] - row0, cnt = min(p.bv[2 * yo + 1], p.ks_v);
      const int32_t* w = p.cv + (int64_t)yo * p.ks_v;
      int acc = 1 << 21;
      for (int j = 0; j < cnt; ++j) acc += w[j] * (int)s_h[min(max(r0 + j, 0), nrows - 1) * R + xo];
      const uint8_t px = clip8(acc);
      if (p.u8) p.u8[((b * 3 + c) * R + yo) * (int64_t)R + xo] = px;
      const int patch = xo / P, pxx = xo - patch * P;
      rows[(int64_t)patch * p.Kp + (c * P + py) * P + pxx] = from_f32<T>((float)(((double)px / 255.0 - mean[c]) / stdv[c]));
    }
    // (the next channel's first pass writes s_in, which the vertical pass does not read; its second pass writes s_h behind a barrier)
  }
  const int k3 = 3 * P * P, padk = p.Kp - k3;
  for (int i = tid; i < g * padk; i += CLIP_THREADS) {
    const int patch = i / padk, k = i - patch * padk;
    rows[(int64_t)patch * p.Kp + k3 + k] = from_f32<T>(0.0f);
  }
}

static int launch_clip_preprocess(const float* x, int b, int s, int r, int p, float lo, float hi, const int32_t* bh, const int32_t* ch, int ks_h,
                                  const int32_t* bv, const int32_t* cv, int ks_v, int max_rows, void* rows, uint8_t* u8, int dtype, hipStream_t st) {
  ETAINV_CHECK(x && bh && ch && bv && cv && rows, "null pointer: x, the four tables and rows_out are required (u8_out is optional)");
  ETAINV_CHECK(p == 14 || p == 16 || p == 32, "patch size must be 14, 16 or 32");
  ETAINV_CHECK(r >= p && r % p == 0 && r <= 4096, "the resized side R must be a multiple of the patch size (at most 4096)");
  ETAINV_CHECK(b >= 0 && b <= 65535 && s >= 1 && s <= 16384, "b must be in [0, 65535] and s in [1, 16384]");
  ETAINV_CHECK(ks_h >= 1 && ks_v >= 1 && max_rows >= 1 && max_rows <= s, "tap counts and max_rows must be positive, max_rows at most s");
  ETAINV_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "input_range must be finite with hi > lo");
  const size_t lds = (size_t)max_rows * ((size_t)s + r);
  ETAINV_CHECK(lds <= 65536, "a band of p output rows needs max_rows * (s + r) bytes of LDS, at most 65536: the image is too large for this resize");
  if (b == 0) return 0;
  ClipPreParams q = {x, bh, ch, bv, cv, rows, u8, s, r, p, cdiv(3 * p * p, 64) * 64, ks_h, ks_v, max_rows, lo, hi - lo};
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(clip_preprocess_kernel<T>, dim3(r / p, b), dim3(CLIP_THREADS), lds, st, q));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ token assembly
template <typename T>
__global__ void clip_assemble_kernel(const T* __restrict__ patches, const T* __restrict__ cls, const T* __restrict__ pos, T* __restrict__ out, int g2,
                                     int d, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int64_t row = i / d;
  const int c = (int)(i - row * d), t = (int)(row % (g2 + 1));
  const int64_t bi = row / (g2 + 1);
  const float v = t == 0 ? to_f32(cls[c]) : to_f32(patches[(bi * g2 + t - 1) * d + c]);
  out[i] = from_f32<T>(v + to_f32(pos[(int64_t)t * d + c]));
}

// ------------------------------------------------------------------------------------------------------------------ attention
constexpr int VA_D = 64, VA_BQ = 64, VA_BK = 32;
constexpr int VA_KS = VA_D + 8;      // K tile row stride in elements (144 B: 16-byte aligned rows)
constexpr int VA_VS = VA_BK + 8;     // V^T tile row stride in elements (80 B: 8-byte aligned rows)

template <typename T>
__global__ void __launch_bounds__(CLIP_THREADS) vit_attention_kernel(const T* __restrict__ qkv, T* __restrict__ out, int n, int heads, float scale_log2) {
  typedef typename ClipFrag<T>::v8 v8;
  typedef typename ClipFrag<T>::v4 v4;
  __shared__ __attribute__((aligned(16))) T s_k[VA_BK * VA_KS];
  __shared__ __attribute__((aligned(16))) T s_vt[VA_D * VA_VS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int C = heads * VA_D;
  const T* base = qkv + (int64_t)blockIdx.z * n * 3 * C + blockIdx.y * VA_D;
  const int qi = blockIdx.x * VA_BQ + wave * 16 + c;
  const float ninf = -__builtin_inff();

  // B operand of S^T = K Q^T: B[k = dim 32 ks + 8 g + j][col = query c]; a query past n is zero (its result is not stored)
  v8 qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (qi < n) raw = *reinterpret_cast<const u32x4*>(base + (int64_t)qi * 3 * C + 32 * ks + 8 * g);
    qf[ks] = *reinterpret_cast<v8*>(&raw);
  }
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = ninf, l = 0.f;

  const int skey = tid >> 3, sdc = (tid & 7) * 8;   // staging: one 16-byte piece of K and of V per thread
  for (int k0 = 0; k0 < n; k0 += VA_BK) {
    __syncthreads();
    {
      u32x4 kr = {0u, 0u, 0u, 0u}, vr = {0u, 0u, 0u, 0u};
      if (k0 + skey < n) {                          // rows >= n are never read: their slots hold zero
        const T* row = base + (int64_t)(k0 + skey) * 3 * C + sdc;
        kr = *reinterpret_cast<const u32x4*>(row + C);
        vr = *reinterpret_cast<const u32x4*>(row + 2 * C);
      }
      *reinterpret_cast<u32x4*>(&s_k[skey * VA_KS + sdc]) = kr;
      const T* ve = reinterpret_cast<const T*>(&vr);
#pragma unroll
      for (int i = 0; i < 8; ++i) s_vt[(sdc + i) * VA_VS + skey] = ve[i];
    }
    __syncthreads();

    // S^T: s[t][r] = score of key k0 + 16 t + 4 g + r against query c
    f32x4 s[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const v8 a = *reinterpret_cast<const v8*>(&s_k[(16 * t + c) * VA_KS + 32 * ks + 8 * g]);
        s[t] = ClipFrag<T>::mfma(a, qf[ks], s[t]);
      }
    }
    float mx = ninf;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool live = k0 + 16 * t + 4 * g + r < n;
        s[t][r] = live ? s[t][r] * scale_log2 : ninf;
        mx = fmaxf(mx, s[t][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);                  // finite: key k0 of every tile is live
    const float alpha = __builtin_amdgcn_exp2f(m - mn);
    v8 pf;
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T pr = from_f32<T>(__builtin_amdgcn_exp2f(s[t][r] - mn));
        pf[4 * t + r] = pr;
        ps += to_f32(pr);
      }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    // O^T += V^T P^T: A[row = dim 16 dt + c][k slot (g, j)] = V[key of slot][dim], B = pf
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const T* vrow = &s_vt[(16 * dt + c) * VA_VS + 4 * g];
      const v4 lo4 = *reinterpret_cast<const v4*>(vrow), hi4 = *reinterpret_cast<const v4*>(vrow + 16);
      v8 a;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = lo4[j];
        a[4 + j] = hi4[j];
      }
      o[dt] *= alpha;
      o[dt] = ClipFrag<T>::mfma(a, pf, o[dt]);
    }
  }
  // o[dt][r] = O[query c][dim 16 dt + 4 g + r]
  if (qi < n) {
    T* op = out + ((int64_t)blockIdx.z * n + qi) * C + blockIdx.y * VA_D + 4 * g;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      v4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] = from_f32<T>(o[dt][r] / l);
      *reinterpret_cast<v4*>(op + 16 * dt) = w;
    }
  }
}

// fp32 twin: one query per thread, keys and values through LDS, the same online softmax per key
__global__ void __launch_bounds__(VA_BQ) vit_attention_f32_kernel(const float* __restrict__ qkv, float* __restrict__ out, int n, int heads,
                                                                   float scale_log2) {
  __shared__ float s_k[VA_BK][VA_D], s_v[VA_BK][VA_D];
  const int tid = threadIdx.x, C = heads * VA_D;
  const float* base = qkv + (int64_t)blockIdx.z * n * 3 * C + blockIdx.y * VA_D;
  const int qi = blockIdx.x * VA_BQ + tid;
  float q[VA_D], o[VA_D];
#pragma unroll
  for (int c = 0; c < VA_D; ++c) {
    q[c] = qi < n ? base[(int64_t)qi * 3 * C + c] * scale_log2 : 0.f;
    o[c] = 0.f;
  }
  float m = -__builtin_inff(), l = 0.f;
  for (int k0 = 0; k0 < n; k0 += VA_BK) {
    const int live = min(VA_BK, n - k0);
    __syncthreads();
    for (int i = tid; i < VA_BK * VA_D; i += VA_BQ) {
      const int j = i / VA_D, c = i - j * VA_D;
      const bool in = j < live;
      s_k[j][c] = in ? base[(int64_t)(k0 + j) * 3 * C + C + c] : 0.f;
      s_v[j][c] = in ? base[(int64_t)(k0 + j) * 3 * C + 2 * C + c] : 0.f;
    }
    __syncthreads();
    if (qi < n)
      for (int j = 0; j < live; ++j) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < VA_D; ++c) s = fmaf(q[c], s_k[j][c], s);
        const float mn = fmaxf(m, s), a = __builtin_amdgcn_exp2f(m - mn), pj = __builtin_amdgcn_exp2f(s - mn);
        l = l * a + pj;
#pragma unroll
        for (int c = 0; c < VA_D; ++c) o[c] = fmaf(pj, s_v[j][c], o[c] * a);
        m = mn;
      }
  }
  if (qi < n) {
    float* op = out + ((int64_t)blockIdx.z * n + qi) * C + blockIdx.y * VA_D;
#pragma unroll
    for (int c = 0; c < VA_D; ++c) op[c] = o[c] / l;
  }
}

static int launch_vit_attention(const void* qkv, void* out, int b, int n, int heads, int d, int dtype, hipStream_t s) {
  ETAINV_CHECK(qkv && out, "null pointer: qkv and out are required");
  ETAINV_CHECK(d == VA_D, "ViT attention is built for head_dim 64 only");
  ETAINV_CHECK(b >= 1 && b <= 65535 && heads >= 1 && heads <= 65535 && n >= 1 && n <= (1 << 20), "b and heads must be in [1, 65535], n in [1, 2^20]");
  ETAINV_CHECK((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "qkv and out must be 16-byte aligned");
  const float scale_log2 = 0.125f * 1.4426950408889634f;
  const dim3 grid(cdiv(n, VA_BQ), heads, b);
  if (dtype == ETAINV_F32) {
    hipLaunchKernelGGL(vit_attention_f32_kernel, grid, dim3(VA_BQ), 0, s, (const float*)qkv, (float*)out, n, heads, scale_log2);
  } else {
    ETAINV_DISPATCH_HALF(dtype, T, hipLaunchKernelGGL(vit_attention_kernel<T>, grid, dim3(CLIP_THREADS), 0, s, (const T*)qkv, (T*)out, n, heads,
                                                     scale_log2));
  }
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ embedding head
// 1024 threads: the projection is P dot products of length d, one per wave at a time, and a block of 4 waves left them waiting on each other's loads
constexpr int HEAD_THREADS = 1024, HEAD_WAVES = HEAD_THREADS / 64;

__device__ __forceinline__ float clip_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();                      // (the previous call's readers are done with red)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int w = 0; w < HEAD_WAVES; ++w) r += red[w];
  return r;
}

struct ClipHeadParams {
  const void* x;          // [B][n][d], TX
  const int32_t* index;   // [B] pooled token of every row, or null: token 0
  const float *gamma, *beta;
  const void* proj;       // [P][d], TW
  float* out;             // [B][P]
  int n, d, P;
  float eps;
};

template <typename TX, typename TW>
__global__ void __launch_bounds__(HEAD_THREADS) clip_embed_head_kernel(ClipHeadParams p) {
  extern __shared__ float clip_head_smem[];
  __shared__ float red[HEAD_WAVES];
  float* s_x = clip_head_smem;          // [d]
  float* s_e = clip_head_smem + p.d;    // [P]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, d = p.d;
  const int64_t b = blockIdx.x;
  const int tok = p.index ? min(max(p.index[b], 0), p.n - 1) : 0;
  const TX* x = (const TX*)p.x + (b * p.n + tok) * (int64_t)d;
  for (int i = tid; i < d; i += HEAD_THREADS) s_x[i] = to_f32(x[i]);
  __syncthreads();
  if (p.gamma) {
    float s = 0.f;
    for (int i = tid; i < d; i += HEAD_THREADS) s += s_x[i];
    const float mean = clip_block_sum(s, red) / (float)d;
    float v = 0.f;
    for (int i = tid; i < d; i += HEAD_THREADS) v = fmaf(s_x[i] - mean, s_x[i] - mean, v);
    const float rstd = 1.0f / sqrtf(clip_block_sum(v, red) / (float)d + p.eps);
    for (int i = tid; i < d; i += HEAD_THREADS) s_x[i] = (s_x[i] - mean) * rstd * p.gamma[i] + (p.beta ? p.beta[i] : 0.f);
    __syncthreads();
  }
  for (int j = wave; j < p.P; j += HEAD_WAVES) {
    const TW* w = (const TW*)p.proj + (int64_t)j * d;
    float a = 0.f;
    for (int i = lane; i < d; i += 64) a = fmaf(to_f32(w[i]), s_x[i], a);
    a = wave_sum(a);
    if (lane == 0) s_e[j] = a;
  }
  __syncthreads();
  float q = 0.f;
  for (int j = tid; j < p.P; j += HEAD_THREADS) q = fmaf(s_e[j], s_e[j], q);
  const float norm = sqrtf(clip_block_sum(q, red));
  for (int j = tid; j < p.P; j += HEAD_THREADS) p.out[b * p.P + j] = s_e[j] / norm;
}

static int launch_clip_embed_head(const void* x, int x_dtype, const int32_t* index, int b, int n, int d, const float* gamma, const float* beta, float eps,
                                  const void* proj, int w_dtype, int P, float* out, hipStream_t s) {
  ETAINV_CHECK(x && proj && out, "null pointer: x, proj and out are required (index, gamma and beta are optional)");
  ETAINV_CHECK(!beta || gamma, "beta without gamma");
  ETAINV_CHECK(b >= 0 && n >= 1 && d >= 1 && P >= 1 && (int64_t)d + P <= 12288, "b >= 0, n >= 1 and d + P in [2, 12288]");
  if (b == 0) return 0;
  ClipHeadParams q = {x, index, gamma, beta, proj, out, n, d, P, eps};
  const size_t lds = (size_t)(d + P) * sizeof(float);
  ETAINV_DISPATCH_DTYPE(x_dtype, TX, ETAINV_DISPATCH_DTYPE(w_dtype, TW,
      hipLaunchKernelGGL((clip_embed_head_kernel<TX, TW>), dim3(b), dim3(HEAD_THREADS), lds, s, q)));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ scores
constexpr int CLIP_SIM_VALS = 7;

__device__ __forceinline__ double clip_wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// mode 0 text_img, 1 img_img, 2 textdir_imgdir, 3 text_img_acc -> out [B]; 4: all four of a pair, out [B][4] in that order.  A prompt's embedding is the mean of its T unit embeddings, renormalised
// (:118-125; with T = 1 the reference renormalises too).  With a = img_tgt, s = img_src, t / u = the unnormalised means of txt_tgt / txt_src:
//   text_img = a.t / |t|;  img_img = s.a;  textdir_imgdir = (a.t - s.t) / |t| - (a.u - s.u) / |u|;  acc = a.t / |t| > a.u / |u|
__global__ void __launch_bounds__(CLIP_THREADS) clip_similarity_kernel(const float* img_src, const float* img_tgt, const float* txt_src,
                                                                       const float* txt_tgt, int T, int P, int mode, float* out) {
  __shared__ double red[CLIP_WAVES][CLIP_SIM_VALS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t b = blockIdx.x;
  double v[CLIP_SIM_VALS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // t.t, u.u, a.t, a.u, s.t, s.u, a.s
  for (int k = tid; k < P; k += CLIP_THREADS) {
    const double a = img_tgt ? (double)img_tgt[b * P + k] : 0.0, s = img_src ? (double)img_src[b * P + k] : 0.0;
    double t = 0.0, u = 0.0;
    for (int i = 0; i < T; ++i) {
      if (txt_tgt) t += (double)txt_tgt[(b * T + i) * P + k];
      if (txt_src) u += (double)txt_src[(b * T + i) * P + k];
    }
    t /= (double)T;
    u /= (double)T;
    v[0] = fma(t, t, v[0]);
    v[1] = fma(u, u, v[1]);
    v[2] = fma(a, t, v[2]);
    v[3] = fma(a, u, v[3]);
    v[4] = fma(s, t, v[4]);
    v[5] = fma(s, u, v[5]);
    v[6] = fma(a, s, v[6]);
  }
#pragma unroll
  for (int q = 0; q < CLIP_SIM_VALS; ++q) v[q] = clip_wave_sum_f64(v[q]);
  if (lane == 0)
    for (int q = 0; q < CLIP_SIM_VALS; ++q) red[wave][q] = v[q];
  __syncthreads();
  if (tid == 0) {
    double r[CLIP_SIM_VALS];
    for (int q = 0; q < CLIP_SIM_VALS; ++q) {
      r[q] = 0.0;
      for (int w = 0; w < CLIP_WAVES; ++w) r[q] += red[w][q];
    }
    const double nt = sqrt(r[0]), nu = sqrt(r[1]);
    const double res[4] = {r[2] / nt, r[6], (r[2] - r[4]) / nt - (r[3] - r[5]) / nu, (r[2] / nt > r[3] / nu) ? 1.0 : 0.0};
    if (mode == 4) {
      for (int q = 0; q < 4; ++q) out[4 * b + q] = (float)res[q];
    } else {
      out[b] = (float)res[mode];
    }
  }
}

static int launch_clip_similarity(const float* img_src, const float* img_tgt, const float* txt_src, const float* txt_tgt, int b, int T, int P, int mode,
                                  float* out, hipStream_t s) {
  ETAINV_CHECK(mode >= 0 && mode <= 4, "unknown metric mode: 0 text_img, 1 img_img, 2 textdir_imgdir, 3 text_img_acc, 4 all four");
  ETAINV_CHECK(T >= 1, "templates per prompt (t) must be at least 1");
  ETAINV_CHECK(out && img_tgt, "null pointer: out and img_tgt are required");
  ETAINV_CHECK(mode == 1 || txt_tgt, "null pointer: txt_tgt is required by every mode but img_img");
  ETAINV_CHECK((mode != 1 && mode != 2 && mode != 4) || img_src, "null pointer: img_src is required by img_img and textdir_imgdir");
  ETAINV_CHECK((mode != 2 && mode != 3 && mode != 4) || txt_src, "null pointer: txt_src is required by textdir_imgdir and text_img_acc");
  ETAINV_CHECK(b >= 0 && P >= 1, "b >= 0 and p >= 1");
  if (b == 0) return 0;
  hipLaunchKernelGGL(clip_similarity_kernel, dim3(b), dim3(CLIP_THREADS), 0, s, img_src, img_tgt, txt_src, txt_tgt, T, P, mode, out);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace etainv

using namespace etainv;

#define CLIP_ENTRY(name, call)                                        \
  const int rc = call;                                                \
  if (rc) set_error(std::string(name ": ") + etainv_last_error());    \
  return rc

extern "C" int etainv_clip_preprocess(const float* x, int b, int s, int r, int p, float lo, float hi, const int32_t* bounds_h, const int32_t* coef_h,
                                      int ksize_h, const int32_t* bounds_v, const int32_t* coef_v, int ksize_v, int max_rows, void* rows_out,
                                      uint8_t* u8_out, int dtype, void* stream) {
  CLIP_ENTRY("etainv_clip_preprocess", launch_clip_preprocess(x, b, s, r, p, lo, hi, bounds_h, coef_h, ksize_h, bounds_v, coef_v, ksize_v, max_rows,
                                                              rows_out, u8_out, dtype, (hipStream_t)stream));
}

extern "C" int etainv_clip_assemble_tokens(const void* patches, const void* cls, const void* pos, void* out, int b, int g2, int d, int dtype,
                                           void* stream) {
  ETAINV_CHECK(patches && cls && pos && out, "null pointer");
  ETAINV_CHECK(b >= 0 && g2 >= 1 && d >= 1, "b >= 0, g2 >= 1, d >= 1");
  const int64_t total = (int64_t)b * (g2 + 1) * d;
  if (total == 0) return 0;
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(clip_assemble_kernel<T>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream,
                                                    (const T*)patches, (const T*)cls, (const T*)pos, (T*)out, g2, d, total));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

extern "C" int etainv_op_vit_attention(const void* qkv, void* out, int b, int n, int heads, int d, int dtype, void* stream) {
  CLIP_ENTRY("etainv_op_vit_attention", launch_vit_attention(qkv, out, b, n, heads, d, dtype, (hipStream_t)stream));
}

extern "C" int etainv_clip_embed_head(const void* x, int x_dtype, const int32_t* index, int b, int n, int d, const float* gamma, const float* beta,
                                      float eps, const void* proj, int w_dtype, int p, float* out, void* stream) {
  CLIP_ENTRY("etainv_clip_embed_head", launch_clip_embed_head(x, x_dtype, index, b, n, d, gamma, beta, eps, proj, w_dtype, p, out, (hipStream_t)stream));
}

extern "C" int etainv_clip_similarity(const float* img_src, const float* img_tgt, const float* txt_src, const float* txt_tgt, int b, int t, int p,
                                      int mode, float* out, void* stream) {
  CLIP_ENTRY("etainv_clip_similarity", launch_clip_similarity(img_src, img_tgt, txt_src, txt_tgt, b, t, p, mode, out, (hipStream_t)stream));
}
