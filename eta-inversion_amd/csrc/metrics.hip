// Image metrics without a pretrained network: MSE, PSNR, SSIM and MS-SSIM of B image pairs [B][3][H][W] in one call.
//   metrics/metrics.py:7-17 (mse), :23-34 (psnr); metrics/msssim.py:61-106, :168-247 (ms_ssim, data_range 1);
//   metrics/ssim.py:8-30 -> torchmetrics.image.StructuralSimilarityIndexMeasure() with its defaults [3P] (restated, see include/etainv.h)
// Launches, all on the caller's stream:
//   prep       grid (P, B): per pair and block, min / max of both images and the sum of squared differences -> partials
//   level l    grid (tiles_x, tiles_y, 3 B): a 16 x 32 tile of window positions of one (pair, channel) plane.  The tile and its 10-pixel halo of both
//              images are staged in LDS, normalised on the way ((x - lo) / (hi - lo); levels above 0 read the pooled planes, already normalised);
//              the five window moments E[x], E[y], E[x^2], E[y^2], E[xy] are formed separably, along H into LDS and along W from there; a position
//              gives three values: cs and ssim with the fixed constants of ms_ssim, and (level 0) ssim with the constants of the range taken from
//              the data, which every block reduces from the prep partials; their block sums -> partials.  The block also writes the 2 x 2
//              average-pooled pixels of the next level whose window starts in its tile rows / columns (the last tile of a row / column: up to the edge),
//              read from the staged tile: no pooling pass.
//   finalize   grid (B): sums every list of partials in index order and writes the four results of the pair
// Arithmetic is float64 from the normalisation on.  sigma = E[x^2] - mu^2 cancels: in float32 that costs about 1e-7 absolute, which against
// C2 = 9e-4 (or (0.03 range)^2) is what makes a float32 run of the same formulas differ from the exact value in the fifth decimal on smooth
// images.  The window is the float32 window of the reference (exp and normalisation rounded to float32), as constants.
// Order: a thread's values in index order, a wave by the xor butterfly, the waves of a block in index order, the blocks in index order.  No
// floating-point atomics: a pair's four results do not depend on B, on the pair's position or on the other metrics asked for, and are
// bit-identical from run to run.
#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace etainv {

constexpr int MET_THREADS = 256, MET_WAVES = MET_THREADS / 64;
constexpr int MET_WIN = 11, MET_HALO = MET_WIN - 1;
constexpr int MET_TH = 16, MET_TW = 32;                             // window positions per tile (both even: pooling windows never straddle tiles)
constexpr int MET_SH = MET_TH + MET_HALO, MET_SW = MET_TW + MET_HALO;   // staged pixels per tile
constexpr int MET_LEVELS = 5, MET_PREP_MAX = 64, MET_PREP_VALS = 5, MET_PART_VALS = 3;
constexpr int MET_MSE = 1, MET_PSNR = 2, MET_SSIM = 4, MET_MSSSIM = 8;

// torch.exp(-(arange(11) - 5)^2 / (2 * 1.5^2)) / its sum, in float32 (metrics/msssim.py:15-29)
__device__ constexpr float MET_WINDOW[MET_WIN] = {0x1.0d957p-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,
                                                  0x1.b43c3ep-3f, 0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d957p-10f};
__device__ constexpr double MET_WEIGHTS[MET_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};

__device__ __forceinline__ double met_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double met_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double met_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// the range of the normalised pair from the prep partials of its P blocks (minimum and maximum: no order); every lane of the calling wave gets it
__device__ __forceinline__ double met_data_range(const double* prep, int P, double span, int lane) {
  const bool have = lane < P;
  const double* q = prep + (have ? lane : 0) * MET_PREP_VALS;
  const double inf = __builtin_inf();
  const double pmin = met_wave_min(have ? q[0] : inf), pmax = met_wave_max(have ? q[1] : -inf);
  const double tmin = met_wave_min(have ? q[2] : inf), tmax = met_wave_max(have ? q[3] : -inf);
  return fmax(pmax - pmin, tmax - tmin) / span;
}

// ---- prep: partials [B][P][5] = (min pred, max pred, min target, max target, sum of squared raw differences)
__global__ void __launch_bounds__(MET_THREADS) metrics_prep_kernel(const float* pred, const float* target, int64_t n, double* part) {
  __shared__ double red[MET_WAVES][MET_PREP_VALS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* p = pred + (int64_t)blockIdx.y * n;
  const float* t = target + (int64_t)blockIdx.y * n;
  const double inf = __builtin_inf();
  double v[MET_PREP_VALS] = {inf, -inf, inf, -inf, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * MET_THREADS + tid; i < n; i += (int64_t)gridDim.x * MET_THREADS) {
    const double a = p[i], b = t[i], d = a - b;
    v[0] = fmin(v[0], a);
    v[1] = fmax(v[1], a);
    v[2] = fmin(v[2], b);
    v[3] = fmax(v[3], b);
    v[4] = fma(d, d, v[4]);
  }
  v[0] = met_wave_min(v[0]);
  v[1] = met_wave_max(v[1]);
  v[2] = met_wave_min(v[2]);
  v[3] = met_wave_max(v[3]);
  v[4] = met_wave_sum(v[4]);
  if (lane == 0)
    for (int q = 0; q < MET_PREP_VALS; ++q) red[wave][q] = v[q];
  __syncthreads();
  if (tid == 0) {
    double* o = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * MET_PREP_VALS;
    double s = 0.0, lo0 = inf, hi0 = -inf, lo1 = inf, hi1 = -inf;
    for (int w = 0; w < MET_WAVES; ++w) {
      lo0 = fmin(lo0, red[w][0]);
      hi0 = fmax(hi0, red[w][1]);
      lo1 = fmin(lo1, red[w][2]);
      hi1 = fmax(hi1, red[w][3]);
      s += red[w][4];
    }
    o[0] = lo0;
    o[1] = hi0;
    o[2] = lo1;
    o[3] = hi1;
    o[4] = s;
  }
}

struct MetLevelParams {
  const void* x;        // [B][3][H][W], TIn
  const void* y;
  double* px;           // [B][3][Hp][Wp] pooled planes of the next level, or null
  double* py;
  double* part;         // [3 B][tiles_y * tiles_x][3] = block sums of (cs, ssim with C of range 1, ssim with C of the data range)
  const double* prep;   // level 0: the prep partials [B][prep_P][5]; null: no data-range value (it repeats the range-1 one)
  int prep_P;
  int H, W, Hp, Wp;
  double lo, span;      // normalisation of the staged pixels: (v - lo) / span
};

template <typename TIn>
__global__ void __launch_bounds__(MET_THREADS) metrics_level_kernel(MetLevelParams p) {
  __shared__ double sx[MET_SH][MET_SW], sy[MET_SH][MET_SW];
  __shared__ double mom[5][MET_TH][MET_SW];
  __shared__ double red[MET_WAVES][MET_PART_VALS];
  __shared__ double range_s;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = p.H, W = p.W, Ho = H - MET_HALO, Wo = W - MET_HALO;
  const int ty0 = blockIdx.y * MET_TH, tx0 = blockIdx.x * MET_TW;
  const int64_t z = blockIdx.z;
  const TIn* x = (const TIn*)p.x + z * H * W;
  const TIn* y = (const TIn*)p.y + z * H * W;

  if (p.prep && wave == 0) {
    const double r = met_data_range(p.prep + (z / 3) * p.prep_P * MET_PREP_VALS, p.prep_P, p.span, lane);
    if (lane == 0) range_s = r;
  }
  // ---- stage the tile and its halo, normalised; outside the image: zero (read by the pooling only, as its padding)
  for (int i = tid; i < MET_SH * MET_SW; i += MET_THREADS) {
    const int r = i / MET_SW, c = i - r * MET_SW;
    const int gy = ty0 + r, gx = tx0 + c;
    double a = 0.0, b = 0.0;
    if (gy < H && gx < W) {
      a = ((double)x[(int64_t)gy * W + gx] - p.lo) / p.span;
      b = ((double)y[(int64_t)gy * W + gx] - p.lo) / p.span;
    }
    sx[r][c] = a;
    sy[r][c] = b;
  }
  __syncthreads();

  // ---- the next level: pooled pixel (i, j) averages rows 2 i - pad, 2 i - pad + 1 (pad = size % 2; row -1 is padding and counts in the divisor).
  // This block writes the pixels whose window starts in its tile rows (tile 0: from the padding row on; the last tile: up to the edge), same for columns
  if (p.px) {
    const int pad_h = H & 1, pad_w = W & 1;
    const bool last_y = blockIdx.y == gridDim.y - 1, last_x = blockIdx.x == gridDim.x - 1;
    const int i_lo = ty0 == 0 ? 0 : ty0 / 2 + pad_h, j_lo = tx0 == 0 ? 0 : tx0 / 2 + pad_w;
    const int i_hi = min(p.Hp, ((last_y ? H : ty0 + MET_TH) + pad_h + 1) / 2), j_hi = min(p.Wp, ((last_x ? W : tx0 + MET_TW) + pad_w + 1) / 2);
    const int nr = i_hi - i_lo, nc = j_hi - j_lo;
    double* px = p.px + z * p.Hp * p.Wp;
    double* py = p.py + z * p.Hp * p.Wp;
    for (int k = tid; k < (nr > 0 && nc > 0 ? nr * nc : 0); k += MET_THREADS) {
      const int i = i_lo + k / nc, j = j_lo + k % nc;
      const int r0 = 2 * i - pad_h - ty0, c0 = 2 * j - pad_w - tx0;      // -1: the padding
      double a = 0.0, b = 0.0;
#pragma unroll
      for (int dr = 0; dr < 2; ++dr)
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
          const int r = r0 + dr, c = c0 + dc;
          if (r >= 0 && c >= 0 && r < MET_SH && c < MET_SW) {
            a += sx[r][c];
            b += sy[r][c];
          }
        }
      px[(int64_t)i * p.Wp + j] = 0.25 * a;
      py[(int64_t)i * p.Wp + j] = 0.25 * b;
    }
  }

  // ---- moments along H: window row r of the tile, every staged column
  for (int i = tid; i < MET_TH * MET_SW; i += MET_THREADS) {
    const int r = i / MET_SW, c = i - r * MET_SW;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MET_WIN; ++k) {
      const double w = (double)MET_WINDOW[k], a = sx[r + k][c], b = sy[r + k][c];
      m[0] = fma(w, a, m[0]);
      m[1] = fma(w, b, m[1]);
      m[2] = fma(w, a * a, m[2]);
      m[3] = fma(w, b * b, m[3]);
      m[4] = fma(w, a * b, m[4]);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) mom[q][r][c] = m[q];
  }
  __syncthreads();

  // ---- moments along W and the three values of every window position of the tile
  const double R = p.prep ? range_s : 1.0;
  const double C1 = 1e-4, C2 = 9e-4;                                  // (0.01 * 1)^2, (0.03 * 1)^2
  const double C1r = (0.01 * R) * (0.01 * R), C2r = (0.03 * R) * (0.03 * R);
  double acc[MET_PART_VALS] = {0.0, 0.0, 0.0};
  for (int i = tid; i < MET_TH * MET_TW; i += MET_THREADS) {
    const int r = i / MET_TW, c = i - r * MET_TW;
    if (ty0 + r >= Ho || tx0 + c >= Wo) continue;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < MET_WIN; ++k) {
      const double w = (double)MET_WINDOW[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] = fma(w, mom[q][r][c + k], m[q]);
    }
    const double mu11 = m[0] * m[0], mu22 = m[1] * m[1], mu12 = m[0] * m[1];
    const double s11 = m[2] - mu11, s22 = m[3] - mu22, s12 = m[4] - mu12;
    const double cs = (2.0 * s12 + C2) / (s11 + s22 + C2);
    acc[0] += cs;
    acc[1] += (2.0 * mu12 + C1) / (mu11 + mu22 + C1) * cs;
    double v;
    if (R > 0.0) {
      v = ((2.0 * mu12 + C1r) * (2.0 * s12 + C2r)) / ((mu11 + mu22 + C1r) * (s11 + s22 + C2r));
    } else {
      // two constant images: both constants of the formula are 0 and so, but for rounding, are the variances.  The structure term is 1 (its value
      // at zero variance for every C2 > 0), the luminance term is taken with C1 = 0, and 0 / 0 (both images 0) is 1
      const double den = mu11 + mu22;
      v = den > 0.0 ? 2.0 * mu12 / den : 1.0;
    }
    acc[2] += v;
  }
#pragma unroll
  for (int q = 0; q < MET_PART_VALS; ++q) acc[q] = met_wave_sum(acc[q]);
  if (lane == 0)
    for (int q = 0; q < MET_PART_VALS; ++q) red[wave][q] = acc[q];
  __syncthreads();
  if (tid < MET_PART_VALS) {
    double s = 0.0;
    for (int w = 0; w < MET_WAVES; ++w) s += red[w][tid];
    const int64_t blk = (int64_t)blockIdx.y * gridDim.x + blockIdx.x, nblk = (int64_t)gridDim.x * gridDim.y;
    p.part[(z * nblk + blk) * MET_PART_VALS + tid] = s;
  }
}

struct MetFinalParams {
  const double* prep;   // [B][prep_P][5]
  int prep_P;
  const double* part[MET_LEVELS];   // level l: [3 B][nblk[l]][3]
  int nblk[MET_LEVELS];
  double npos[MET_LEVELS];          // window positions of a plane
  int levels;                       // 0: no ssim / msssim; 1: level 0 only; 5
  int mask;
  double n, span;                   // elements of a pair (3 H W), hi - lo
  float* out;                       // [B][4]
};

// sum of count values at v[i * stride] in a fixed order: thread t takes i = t, t + 256, ..; butterfly; the waves in index order
__device__ double met_block_sum(const double* v, int count, int stride, double (*red)[MET_WAVES]) {
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < count; i += MET_THREADS) s += v[(int64_t)i * stride];
  s = met_wave_sum(s);
  __syncthreads();                    // (the previous call's readers are done with red)
  if ((tid & 63) == 0) (*red)[tid >> 6] = s;
  __syncthreads();
  double r = 0.0;
  for (int w = 0; w < MET_WAVES; ++w) r += (*red)[w];
  return r;
}

__global__ void __launch_bounds__(MET_THREADS) metrics_finalize_kernel(MetFinalParams p) {
  __shared__ double red[MET_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float nan = __builtin_nanf("");
  float* out = p.out + 4 * b;
  const double sse = met_block_sum(p.prep + (int64_t)b * p.prep_P * MET_PREP_VALS + 4, p.prep_P, MET_PREP_VALS, &red);
  const double mse = sse / (p.span * p.span) / p.n;
  if (tid == 0) {
    out[0] = (p.mask & MET_MSE) ? (float)mse : nan;
    out[1] = (p.mask & MET_PSNR) ? (float)(10.0 * log10(1.0 / mse)) : nan;
  }
  double ssim = 0.0, ms = 0.0;
  for (int c = 0; c < 3; ++c) {
    double prod = 1.0;
    for (int l = 0; l < p.levels; ++l) {
      const double* v = p.part[l] + ((int64_t)b * 3 + c) * p.nblk[l] * MET_PART_VALS;
      if (l == 0) ssim += met_block_sum(v + 2, p.nblk[l], MET_PART_VALS, &red);
      // relu on every level's cs and on the last level's ssim (msssim.py:234-240)
      const double m = met_block_sum(v + (l == MET_LEVELS - 1 ? 1 : 0), p.nblk[l], MET_PART_VALS, &red) / p.npos[l];
      prod *= pow(fmax(m, 0.0), MET_WEIGHTS[l]);
    }
    ms += prod;
  }
  if (tid == 0) {
    out[2] = (p.mask & MET_SSIM) ? (float)(ssim / (3.0 * p.npos[0])) : nan;
    out[3] = (p.mask & MET_MSSSIM) ? (float)(ms / 3.0) : nan;
  }
}

// ---- host side
static int met_levels(int mask) { return (mask & MET_MSSSIM) ? MET_LEVELS : (mask & MET_SSIM) ? 1 : 0; }
static int met_prep_blocks(int64_t n) { return (int)std::min<int64_t>(MET_PREP_MAX, (n + MET_THREADS * 16 - 1) / (MET_THREADS * 16)); }

struct MetPlan {
  int h[MET_LEVELS], w[MET_LEVELS], tx[MET_LEVELS], ty[MET_LEVELS];
  int64_t prep_off, part_off[MET_LEVELS], pool_off[MET_LEVELS];   // in doubles; pool_off[l]: the x planes of level l >= 1, the y planes follow
  int64_t total;
  int prep_P, levels;
};

static int met_check_shape(int b, int h, int w, int mask) {
  ETAINV_CHECK(b >= 0, "negative b");
  ETAINV_CHECK(mask > 0 && mask < 16, "mask must be a non-empty combination of 1 (mse), 2 (psnr), 4 (ssim), 8 (msssim)");
  ETAINV_CHECK(h >= 1 && w >= 1 && h <= 16384 && w <= 16384, "h and w must be in [1, 16384]");
  ETAINV_CHECK(!(mask & MET_SSIM) || (h >= MET_WIN && w >= MET_WIN), "ssim needs h >= 11 and w >= 11");
  ETAINV_CHECK(!(mask & MET_MSSSIM) || (h > 160 && w > 160), "msssim needs min(h, w) > 160 (four downsamplings of an 11-tap window)");
  ETAINV_CHECK((int64_t)b * 3 <= 65535, "b must be at most 21845");
  return 0;
}

static void met_plan(MetPlan& pl, int b, int h, int w, int mask) {
  pl.levels = met_levels(mask);
  pl.prep_P = met_prep_blocks((int64_t)3 * h * w);
  int64_t off = 0;
  pl.prep_off = off;
  off += (int64_t)b * pl.prep_P * MET_PREP_VALS;
  for (int l = 0; l < pl.levels; ++l) {
    pl.h[l] = l ? (pl.h[l - 1] + 1) / 2 : h;       // floor((s + 2 (s % 2) - 2) / 2) + 1
    pl.w[l] = l ? (pl.w[l - 1] + 1) / 2 : w;
    pl.ty[l] = cdiv(pl.h[l] - MET_HALO, MET_TH);
    pl.tx[l] = cdiv(pl.w[l] - MET_HALO, MET_TW);
    pl.part_off[l] = off;
    off += (int64_t)b * 3 * pl.ty[l] * pl.tx[l] * MET_PART_VALS;
    pl.pool_off[l] = off;
    if (l) off += (int64_t)2 * b * 3 * pl.h[l] * pl.w[l];
  }
  pl.total = off;
}

int launch_image_metrics(const float* pred, const float* target, int b, int h, int w, float lo, float hi, int mask, float* out, void* workspace,
                         int64_t workspace_bytes, hipStream_t s) {
  if (met_check_shape(b, h, w, mask)) return 1;
  ETAINV_CHECK(pred && target && out, "null pointer: pred, target and out are required");
  ETAINV_CHECK(std::isfinite(lo) && std::isfinite(hi) && hi > lo, "input_range must be finite with hi > lo");
  if (b == 0) return 0;
  MetPlan pl;
  met_plan(pl, b, h, w, mask);
  ETAINV_CHECK(workspace && ((uintptr_t)workspace & 7) == 0, "workspace must be an 8-byte aligned device buffer");
  ETAINV_CHECK(workspace_bytes >= pl.total * (int64_t)sizeof(double), "workspace is smaller than etainv_image_metrics_workspace_bytes reports");
  double* ws = (double*)workspace;
  const int64_t n = (int64_t)3 * h * w;
  const double span = (double)hi - (double)lo;

  hipLaunchKernelGGL(metrics_prep_kernel, dim3(pl.prep_P, b), dim3(MET_THREADS), 0, s, pred, target, n, ws + pl.prep_off);
  ETAINV_LAUNCH_CHECK();
  MetFinalParams f = {};
  for (int l = 0; l < pl.levels; ++l) {
    MetLevelParams p = {};
    const bool pool = l + 1 < pl.levels;
    p.x = l ? (const void*)(ws + pl.pool_off[l]) : (const void*)pred;
    p.y = l ? (const void*)(ws + pl.pool_off[l] + (int64_t)b * 3 * pl.h[l] * pl.w[l]) : (const void*)target;
    p.px = pool ? ws + pl.pool_off[l + 1] : nullptr;
    p.py = pool ? ws + pl.pool_off[l + 1] + (int64_t)b * 3 * pl.h[l + 1] * pl.w[l + 1] : nullptr;
    p.part = ws + pl.part_off[l];
    p.prep = l ? nullptr : ws + pl.prep_off;
    p.prep_P = pl.prep_P;
    p.H = pl.h[l];
    p.W = pl.w[l];
    p.Hp = pool ? pl.h[l + 1] : 0;
    p.Wp = pool ? pl.w[l + 1] : 0;
    p.lo = l ? 0.0 : (double)lo;
    p.span = l ? 1.0 : span;
    const dim3 grid(pl.tx[l], pl.ty[l], 3 * b);
    if (l == 0)
      hipLaunchKernelGGL((metrics_level_kernel<float>), grid, dim3(MET_THREADS), 0, s, p);
    else
      hipLaunchKernelGGL((metrics_level_kernel<double>), grid, dim3(MET_THREADS), 0, s, p);
    ETAINV_LAUNCH_CHECK();
    f.part[l] = p.part;
    f.nblk[l] = pl.tx[l] * pl.ty[l];
    f.npos[l] = (double)(pl.h[l] - MET_HALO) * (double)(pl.w[l] - MET_HALO);
  }
  f.prep = ws + pl.prep_off;
  f.prep_P = pl.prep_P;
  f.levels = pl.levels;
  f.mask = mask;
  f.n = (double)n;
  f.span = span;
  f.out = out;
  hipLaunchKernelGGL(metrics_finalize_kernel, dim3(b), dim3(MET_THREADS), 0, s, f);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace etainv

using namespace etainv;

extern "C" int64_t etainv_image_metrics_workspace_bytes(int b, int h, int w, int mask) {
  if (met_check_shape(b, h, w, mask)) {
    set_error(std::string("etainv_image_metrics_workspace_bytes: ") + etainv_last_error());
    return -1;
  }
  MetPlan pl;
  met_plan(pl, b, h, w, mask);
  return std::max<int64_t>(pl.total, 1) * (int64_t)sizeof(double);
}

extern "C" int etainv_image_metrics(const float* pred, const float* target, int b, int h, int w, float lo, float hi, int mask, float* out,
                                    void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = launch_image_metrics(pred, target, b, h, w, lo, hi, mask, out, workspace, workspace_bytes, (hipStream_t)stream);
  if (rc) set_error(std::string("etainv_image_metrics: ") + etainv_last_error());
  return rc;
}
