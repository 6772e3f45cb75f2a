// The LPIPS metrics' kernels (reference metrics/metrics.py:40-61 `lpips`, metrics/bglpips.py:27-52 and :141-148 `bglpips`): from 2 B images to
// B perceptual distances through torchvision's AlexNet `features`, LPIPS v0.1 (net='alex', lpips=True, spatial=False, eval mode).
//   preprocess      one thread per pixel of the 2 B images: (x - lo) / (hi - lo), 2 v - 1, (bglpips) v (1 - mask), the scaling layer
//                   (v - shift) / scale, NCHW fp32 -> NHWC with four channels (the fourth 0: one kernel row of conv1 is 44 contiguous values).
//                   The arithmetic is float64 and the result is rounded once: v - shift cancels near v = shift, where a chain of fp32 roundings
//                   would leave the fp32 output several units off the exact value.
//   conv2d_relu     implicit GEMM over NHWC, out[m = (image, oy, ox)][n = cout] = sum_k x[pixel(m, tap(k))][c(k)] w[n][k], k = (ky kw + kx) cin + c,
//                   any kh, kw <= 11, stride 1 / 4, pad <= 2, bias and optional ReLU.  A block owns 128 output pixels x 64 channels; per 32-wide
//                   K chunk it gathers its own activation tile into LDS (zero where a tap is in the pad, where the row is past M, where k is past
//                   K; nothing is im2col'ed to memory) and the weight tile next to it.  cin == 4 (conv1): a piece of 4 values is one pixel, and
//                   the K = 484 tail of the last chunk is zero; cin % 32 == 0: a chunk lies inside one tap.  A wave owns 32 pixels x 64 channels:
//                   16-bit on mfma_f32_16x16x32 (ClipFrag), fp32 operands on mfma_f32_16x16x4f32 (the parity mode: correct, not tuned).  The
//                   weights are the MFMA's A operand and the pixels its B operand, so a lane ends with 4 consecutive channels of one pixel
//                   and stores them as one vector.
//   maxpool3s2      NHWC, window 3, stride 2, floor mode: one thread per output pixel and 16-byte channel vector; starts from the window's first
//                   element (any sign of input), keeps the earlier of equal values as F.max_pool2d does.
//   layer_distance  one tap of B pairs: per pixel alpha = sqrt(sum a^2) + 1e-10 (the epsilon is added to the norm), beta likewise, and
//                   sum_c w_c (a_c / alpha - b_c / beta)^2, float64 from the loaded features on; neither normalised map is written.  A wave owns
//                   a pixel at a time (lane = channel mod 64), a block 64 pixels; one float64 partial per block, a finalizer adds a pair's
//                   partials in index order, divides by the pixel count and writes or adds to out[pair].
// Order of every sum: a lane's terms in index order, a wave by the xor butterfly, the waves of a block in index order, the blocks in index
// order; no atomics.  A pair's value does not depend on B or on its position, is bit-identical from run to run, exactly 0.0 for identical
// features ((a / alpha - b / beta) is then exactly 0) and unchanged by swapping the two sides (the difference only changes sign).
#include <cmath>

#include "kernels.h"

namespace etainv {

namespace {

template <typename T> struct LpVec {
  typedef T v4 __attribute__((ext_vector_type(4)));
  typedef T v16b __attribute__((ext_vector_type(16 / sizeof(T))));
};
template <int BYTES> struct LpRaw;
template <> struct LpRaw<8> { typedef u32x2 type; };
template <> struct LpRaw<16> { typedef u32x4 type; };

// ------------------------------------------------------------------------------------------------------------------ preprocess
struct LpipsPreParams {
  const float* x;             // [n][3][H][W]
  const float* mask;          // [n_mask][H][W] or null
  void* out;                  // [n][H][W][4]
  int64_t total, hw;          // n H W, H W
  int n_mask;
  double lo, span;
};

template <typename T>
__global__ void __launch_bounds__(256) lpips_preprocess_kernel(LpipsPreParams p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.total) return;
  const int64_t img = i / p.hw, pix = i - img * p.hw;
  const double shift[3] = {-0.030, -0.088, -0.188}, scale[3] = {0.458, 0.448, 0.450};
  const double keep = p.mask ? 1.0 - (double)p.mask[(img % p.n_mask) * p.hw + pix] : 1.0;
  typename LpVec<T>::v4 o;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double v = 2.0 * (((double)p.x[(img * 3 + c) * p.hw + pix] - p.lo) / p.span) - 1.0;
    if (p.mask) v *= keep;                                 // after the map to [-1, 1], before the scaling layer: the foreground becomes 0
    o[c] = from_f32<T>((float)((v - shift[c]) / scale[c]));
  }
  o[3] = from_f32<T>(0.f);
  *reinterpret_cast<typename LpVec<T>::v4*>((T*)p.out + i * 4) = o;
}

// ------------------------------------------------------------------------------------------------------------------ convolution
constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 32, CV_THREADS = 256;

struct ConvParams {
  const void* x;              // [n][H][W][cin]
  const void* w;              // [cout][kh kw][cin]
  const float* bias;          // [cout] or null
  void* out;                  // [n][Ho][Wo][cout]
  int64_t M;                  // n Ho Wo
  int H, W, cin, cout, kh, kw, stride, pad, Ho, Wo, K, relu;
};

__device__ __forceinline__ f32x4 mfma_f32_k4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

template <typename T, bool SMALLC>
__global__ void __launch_bounds__(CV_THREADS) lpips_conv2d_kernel(ConvParams p) {
  constexpr bool F32 = sizeof(T) == 4;
  constexpr int G = (F32 || SMALLC) ? 4 : 8;               // values per staged piece (8 or 16 bytes)
  constexpr int GPR = CV_BK / G;                           // pieces per tile row
  constexpr int ROWS_PER_PASS = CV_THREADS / GPR;
  constexpr int A_PER = CV_BM / ROWS_PER_PASS, B_PER = CV_BN / ROWS_PER_PASS;
  constexpr int LDK = F32 ? CV_BK + 4 : CV_BK + 8;         // row stride in elements: 16-byte aligned rows (144 B / 80 B)
  typedef typename LpRaw<G * sizeof(T)>::type piece_t;
  __shared__ __attribute__((aligned(16))) T sA[CV_BM * LDK];
  __shared__ __attribute__((aligned(16))) T sB[CV_BN * LDK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, c = lane & 15;
  const int64_t m0 = (int64_t)blockIdx.x * CV_BM;
  const int n0 = blockIdx.y * CV_BN;
  const T* x = (const T*)p.x;
  const T* w = (const T*)p.w;
  const int H = p.H, W = p.W, cin = p.cin, K = p.K, kw = p.kw;

  // the rows this thread stages: their image and the input pixel of tap (0, 0)
  const int kg = tid % GPR, srow = tid / GPR;
  int a_iy0[A_PER], a_ix0[A_PER];
  int64_t a_img[A_PER];
  bool a_ok[A_PER];
  const int64_t hw_out = (int64_t)p.Ho * p.Wo;
#pragma unroll
  for (int j = 0; j < A_PER; ++j) {
    const int64_t m = m0 + srow + j * ROWS_PER_PASS;
    a_ok[j] = m < p.M;
    const int64_t mm = a_ok[j] ? m : 0;
    const int64_t img = mm / hw_out;
    const int rem = (int)(mm - img * hw_out);
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    a_img[j] = img * H * W;
    a_iy0[j] = oy * p.stride - p.pad;
    a_ix0[j] = ox * p.stride - p.pad;
  }

  f32x4 acc[2][4];
#pragma unroll
  for (int pt = 0; pt < 2; ++pt)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[pt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < K; k0 += CV_BK) {
    __syncthreads();
    const int k = k0 + kg * G;
    const bool k_ok = k < K;                               // (only the 4-channel form has a K tail: 484 = 15 chunks + 4 values)
    int tap, c0;
    if (SMALLC) {
      tap = k >> 2;
      c0 = 0;
    } else {
      tap = k0 / cin;
      c0 = k - tap * cin;
    }
    const int ky = tap / kw, kx = tap - ky * kw;
#pragma unroll
    for (int j = 0; j < A_PER; ++j) {
      const int iy = a_iy0[j] + ky, ix = a_ix0[j] + kx;
      piece_t v = {};
      if (a_ok[j] && k_ok && iy >= 0 && iy < H && ix >= 0 && ix < W)
        v = *reinterpret_cast<const piece_t*>(x + (a_img[j] + (int64_t)iy * W + ix) * cin + c0);
      *reinterpret_cast<piece_t*>(&sA[(srow + j * ROWS_PER_PASS) * LDK + kg * G]) = v;
    }
#pragma unroll
    for (int j = 0; j < B_PER; ++j) {
      const int row = srow + j * ROWS_PER_PASS, n = n0 + row;
      piece_t v = {};
      if (n < p.cout && k_ok) v = *reinterpret_cast<const piece_t*>(w + (int64_t)n * K + k);
      *reinterpret_cast<piece_t*>(&sB[row * LDK + kg * G]) = v;
    }
    __syncthreads();
    // A[row = channel 16 t + c][k], B[k][col = pixel 32 wave + 16 pt + c]: acc[pt][t][r] = (channel 16 t + 4 g + r, pixel 32 wave + 16 pt + c)
    if constexpr (F32) {
#pragma unroll
      for (int kk = 0; kk < CV_BK / 4; ++kk) {
        float xb[2];
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) xb[pt] = sA[(32 * wave + 16 * pt + c) * LDK + 4 * kk + g];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const float wa = sB[(16 * t + c) * LDK + 4 * kk + g];
#pragma unroll
          for (int pt = 0; pt < 2; ++pt) acc[pt][t] = mfma_f32_k4(wa, xb[pt], acc[pt][t]);
        }
      }
    } else {
      typedef typename ClipFrag<T>::v8 v8;
      v8 xb[2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) xb[pt] = *reinterpret_cast<const v8*>(&sA[(32 * wave + 16 * pt + c) * LDK + 8 * g]);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const v8 wa = *reinterpret_cast<const v8*>(&sB[(16 * t + c) * LDK + 8 * g]);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) acc[pt][t] = ClipFrag<T>::mfma(wa, xb[pt], acc[pt][t]);
      }
    }
  }

  T* out = (T*)p.out;
#pragma unroll
  for (int pt = 0; pt < 2; ++pt) {
    const int64_t m = m0 + 32 * wave + 16 * pt + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int n = n0 + 16 * t + 4 * g;
      if (m >= p.M || n >= p.cout) continue;               // (cout % 4 == 0: the four channels are inside or outside together)
      typename LpVec<T>::v4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[pt][t][r] + (p.bias ? p.bias[n + r] : 0.f);
        if (p.relu) v = fmaxf(v, 0.f);
        o[r] = from_f32<T>(v);
      }
      *reinterpret_cast<typename LpVec<T>::v4*>(out + m * p.cout + n) = o;
    }
  }
}

int launch_conv2d_relu(const void* x, const void* w, const float* bias, void* out, int n, int h, int wd, int cin, int cout, int kh, int kw, int stride,
                       int pad, int relu, int dtype, hipStream_t st) {
  ETAINV_CHECK(x && w && out, "null pointer: x, w and out are required (bias is optional)");
  ETAINV_CHECK((((uintptr_t)x | (uintptr_t)w | (uintptr_t)out) & 15) == 0 && ((uintptr_t)bias & 3) == 0,
               "x, w and out must be 16-byte aligned, bias 4-byte aligned");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(kh >= 1 && kh <= 11 && kw >= 1 && kw <= 11, "kh and kw must be in [1, 11]");
  ETAINV_CHECK(stride == 1 || stride == 4, "stride must be 1 or 4");
  ETAINV_CHECK(pad >= 0 && pad <= 2, "pad must be in [0, 2]");
  ETAINV_CHECK(n >= 0 && n <= 65535 && h >= 1 && h <= 16384 && wd >= 1 && wd <= 16384, "n must be in [0, 65535], h and w in [1, 16384]");
  ETAINV_CHECK(h + 2 * pad >= kh && wd + 2 * pad >= kw, "the output would be smaller than 1 x 1: h + 2 pad < kh or w + 2 pad < kw");
  ETAINV_CHECK(cin == 4 || (cin >= 32 && cin % 32 == 0 && cin <= 4096), "cin must be 4 (three channels padded with a zero one) or a multiple of 32: a K chunk of 32 lies inside one tap");
  ETAINV_CHECK(cout >= 4 && cout % 4 == 0 && cout <= 65536, "cout must be a multiple of 4: a lane stores four channels as one vector");
  if (n == 0) return 0;
  ConvParams p;
  p.x = x;
  p.w = w;
  p.bias = bias;
  p.out = out;
  p.H = h;
  p.W = wd;
  p.cin = cin;
  p.cout = cout;
  p.kh = kh;
  p.kw = kw;
  p.stride = stride;
  p.pad = pad;
  p.Ho = (h + 2 * pad - kh) / stride + 1;
  p.Wo = (wd + 2 * pad - kw) / stride + 1;
  p.K = kh * kw * cin;
  p.relu = relu ? 1 : 0;
  p.M = (int64_t)n * p.Ho * p.Wo;
  ETAINV_CHECK(p.M <= ((int64_t)1 << 31) - CV_BM, "n * Ho * Wo must stay below 2^31");
  const dim3 grid(cdiv(p.M, CV_BM), cdiv(cout, CV_BN));
  if (cin == 4) {
    ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((lpips_conv2d_kernel<T, true>), grid, dim3(CV_THREADS), 0, st, p));
  } else {
    ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL((lpips_conv2d_kernel<T, false>), grid, dim3(CV_THREADS), 0, st, p));
  }
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ max pooling
template <typename T>
__global__ void __launch_bounds__(256) maxpool3s2_kernel(const T* __restrict__ x, T* __restrict__ out, int64_t total, int H, int W, int C, int Ho, int Wo) {
  constexpr int V = 16 / sizeof(T);
  typedef typename LpVec<T>::v16b vec;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int cv = C / V;
  const int cg = (int)(i % cv);
  int64_t t = i / cv;
  const int ox = (int)(t % Wo);
  t /= Wo;
  const int oy = (int)(t % Ho);
  const int64_t img = t / Ho;
  // floor mode: 2 oy + 2 <= H - 1 and 2 ox + 2 <= W - 1 for every output pixel
  const T* base = x + ((img * H + 2 * oy) * W + 2 * ox) * (int64_t)C + cg * V;
  vec best = *reinterpret_cast<const vec*>(base);
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      if (dy == 0 && dx == 0) continue;
      const vec v = *reinterpret_cast<const vec*>(base + ((int64_t)dy * W + dx) * C);
#pragma unroll
      for (int e = 0; e < V; ++e)
        if (to_f32<T>(v[e]) > to_f32<T>(best[e])) best[e] = v[e];
    }
  *reinterpret_cast<vec*>(out + i * V) = best;
}

int launch_maxpool3s2(const void* x, void* out, int n, int h, int w, int c, int dtype, hipStream_t st) {
  ETAINV_CHECK(x && out, "null pointer: x and out are required");
  ETAINV_CHECK((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "x and out must be 16-byte aligned");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(n >= 0 && n <= 65535 && h >= 3 && h <= 16384 && w >= 3 && w <= 16384, "n must be in [0, 65535], h and w in [3, 16384] (a window of 3)");
  const int v = dtype == ETAINV_F32 ? 4 : 8;
  ETAINV_CHECK(c >= v && c % v == 0 && c <= 65536, "c must be a whole number of 16-byte vectors (a multiple of 8, fp32: of 4)");
  if (n == 0) return 0;
  const int ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
  const int64_t total = (int64_t)n * ho * wo * (c / v);
  ETAINV_CHECK(total <= ((int64_t)1 << 38), "n * Ho * Wo * c is too large");
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(maxpool3s2_kernel<T>, dim3(cdiv(total, 256)), dim3(256), 0, st, (const T*)x, (T*)out, total, h, w, c,
                                                    ho, wo));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ layer distance
constexpr int LD_THREADS = 256, LD_WAVES = LD_THREADS / 64, LD_PIX = 64;      // pixels per block

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
__global__ void __launch_bounds__(LD_THREADS) lpips_distance_kernel(const T* __restrict__ f, const float* __restrict__ w, int B, int pixels, int C, int nblk,
                                                                    double* __restrict__ partials) {
  __shared__ double red[LD_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.y;
  const T* fa = f + b * pixels * (int64_t)C;
  const T* fb = f + (b + B) * pixels * (int64_t)C;
  double dsum = 0.0;
  for (int q = wave; q < LD_PIX; q += LD_WAVES) {
    const int px = blockIdx.x * LD_PIX + q;
    if (px >= pixels) break;
    const T* a = fa + (int64_t)px * C;
    const T* e = fb + (int64_t)px * C;
    double sa = 0.0, sb = 0.0;
    for (int ch = lane; ch < C; ch += 64) {
      const double va = (double)to_f32<T>(a[ch]), vb = (double)to_f32<T>(e[ch]);
      sa = fma(va, va, sa);
      sb = fma(vb, vb, sb);
    }
    const double alpha = sqrt(wave_sum_f64(sa)) + 1e-10, beta = sqrt(wave_sum_f64(sb)) + 1e-10;
    for (int ch = lane; ch < C; ch += 64) {
      const double d = (double)to_f32<T>(a[ch]) / alpha - (double)to_f32<T>(e[ch]) / beta;
      dsum = fma((double)w[ch] * d, d, dsum);
    }
  }
  dsum = wave_sum_f64(dsum);
  if (lane == 0) red[wave] = dsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < LD_WAVES; ++i) s += red[i];
    partials[b * nblk + blockIdx.x] = s;
  }
}

// a pair's partials in block order, divided by the pixel count; written, or added to what out[pair] holds
__global__ void lpips_distance_finalize_kernel(const double* __restrict__ partials, int nblk, int pixels, int accumulate, double* __restrict__ out) {
  if (threadIdx.x != 0) return;
  const int64_t b = blockIdx.x;
  double s = 0.0;
  for (int t = 0; t < nblk; ++t) s += partials[b * nblk + t];
  const double mean = s / (double)pixels;
  out[b] = accumulate ? out[b] + mean : mean;
}

constexpr int LD_MAX_B = 32767, LD_MAX_PIXELS = 1 << 24;

int64_t distance_workspace_bytes(int b, int pixels) {
  if (b < 0 || b > LD_MAX_B || pixels < 1 || pixels > LD_MAX_PIXELS) {
    set_error("etainv_lpips_distance_workspace_bytes: b must be in [0, 32767] and pixels in [1, 2^24]");
    return -1;
  }
  return (int64_t)b * cdiv(pixels, LD_PIX) * (int64_t)sizeof(double);
}

int launch_layer_distance(const void* feats, const float* lin_w, int b, int pixels, int c, int accumulate, double* out, void* ws, int64_t ws_bytes, int dtype,
                          hipStream_t st) {
  ETAINV_CHECK(feats && lin_w && out && ws, "null pointer: feats, lin_w, out and workspace are required");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(((uintptr_t)feats & 15) == 0 && ((uintptr_t)lin_w & 3) == 0 && ((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0,
               "feats must be 16-byte aligned, lin_w 4-byte aligned, out and workspace 8-byte aligned");
  ETAINV_CHECK(b >= 0 && b <= LD_MAX_B && pixels >= 1 && pixels <= LD_MAX_PIXELS, "b must be in [0, 32767] (2 b feature maps) and pixels in [1, 2^24]");
  ETAINV_CHECK(c >= 1 && c <= 65536, "c must be in [1, 65536]");
  ETAINV_CHECK(accumulate == 0 || accumulate == 1, "accumulate must be 0 or 1");
  ETAINV_CHECK(ws_bytes >= distance_workspace_bytes(b, pixels), "workspace too small: see etainv_lpips_distance_workspace_bytes");
  if (b == 0) return 0;
  const int nblk = cdiv(pixels, LD_PIX);
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(lpips_distance_kernel<T>, dim3(nblk, b), dim3(LD_THREADS), 0, st, (const T*)feats, lin_w, b, pixels, c,
                                                    nblk, (double*)ws));
  ETAINV_LAUNCH_CHECK();
  hipLaunchKernelGGL(lpips_distance_finalize_kernel, dim3(b), dim3(64), 0, st, (const double*)ws, nblk, pixels, accumulate, out);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_lpips_preprocess(const float* x, const float* mask, int n, int n_mask, int h, int w, float lo, float hi, void* out, int dtype, hipStream_t st) {
  ETAINV_CHECK(x && out, "null pointer: x and out are required (mask is optional)");
  ETAINV_CHECK((((uintptr_t)x | (uintptr_t)mask) & 3) == 0 && ((uintptr_t)out & 15) == 0, "x and mask must be 4-byte aligned, out 16-byte aligned");
  ETAINV_CHECK(dtype == ETAINV_F32 || dtype == ETAINV_F16 || dtype == ETAINV_BF16, "bad dtype");
  ETAINV_CHECK(n >= 0 && n <= 65535 && h >= 1 && h <= 16384 && w >= 1 && w <= 16384, "n must be in [0, 65535], h and w in [1, 16384]");
  ETAINV_CHECK(!mask || (n_mask >= 1 && n_mask <= 65535), "n_mask must be in [1, 65535] when a mask is given");
  ETAINV_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "input_range must be finite with hi > lo");
  if (n == 0) return 0;
  LpipsPreParams p = {x, mask, out, (int64_t)n * h * w, (int64_t)h * w, mask ? n_mask : 1, (double)lo, (double)hi - (double)lo};
  ETAINV_DISPATCH_DTYPE(dtype, T, hipLaunchKernelGGL(lpips_preprocess_kernel<T>, dim3(cdiv(p.total, 256)), dim3(256), 0, st, p));
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace

}  // namespace etainv

using namespace etainv;

#define LPIPS_ENTRY(name, call)                                       \
  const int rc = call;                                                \
  if (rc) set_error(std::string(name ": ") + etainv_last_error());    \
  return rc

extern "C" int etainv_lpips_preprocess(const float* x, const float* mask, int n, int n_mask, int h, int w, float lo, float hi, void* out, int dtype,
                                       void* stream) {
  LPIPS_ENTRY("etainv_lpips_preprocess", launch_lpips_preprocess(x, mask, n, n_mask, h, w, lo, hi, out, dtype, (hipStream_t)stream));
}

extern "C" int etainv_op_conv2d_relu(const void* x, const void* w, const float* bias, void* out, int n, int h, int wd, int cin, int cout, int kh, int kw,
                                     int stride, int pad, int relu, int dtype, void* stream) {
  LPIPS_ENTRY("etainv_op_conv2d_relu", launch_conv2d_relu(x, w, bias, out, n, h, wd, cin, cout, kh, kw, stride, pad, relu, dtype, (hipStream_t)stream));
}

extern "C" int etainv_op_maxpool3s2(const void* x, void* out, int n, int h, int w, int c, int dtype, void* stream) {
  LPIPS_ENTRY("etainv_op_maxpool3s2", launch_maxpool3s2(x, out, n, h, w, c, dtype, (hipStream_t)stream));
}

extern "C" int64_t etainv_lpips_distance_workspace_bytes(int b, int pixels) { return distance_workspace_bytes(b, pixels); }

extern "C" int etainv_lpips_layer_distance(const void* feats, const float* lin_w, int b, int pixels, int c, int accumulate, double* out, void* workspace,
                                           int64_t workspace_bytes, int dtype, void* stream) {
  LPIPS_ENTRY("etainv_lpips_layer_distance", launch_layer_distance(feats, lin_w, b, pixels, c, accumulate, out, workspace, workspace_bytes, dtype,
                                                                   (hipStream_t)stream));
}
