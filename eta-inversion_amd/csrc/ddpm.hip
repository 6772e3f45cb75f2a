// Edit-friendly DDPM inversion (reference modules/inverse_schedulers/ddpm_inverse_scheduler.py, modules/inversion/ddpm_inversion.py): three
// elementwise passes over fp32 latents of [4][l][l], every thread on one float4 (4 l l is a multiple of 4 and the rows are 16-byte aligned).
//   ddpm_sample_*        DDPMInverseScheduler.sample_latents  :86-129   all noised latents x_t from x_0, one launch
//   ddpm_invert_steps    DDPMInverseScheduler.step            :156-199  CFG, x0_pred, mu, noise map z, corrected x_{t-1} for k steps, one launch
//   ddpm_backward_step   DDPMInversion.predict_step_backward  ddpm_inversion.py:135-166  per-prompt CFG + DDIM step at eta = 1 with the map as noise
// The schedule coefficients are host scalars; they travel in the kernel arguments (a table of at most 2.5 KB), so no host table outlives a call
// and nothing is allocated or copied.
// Rounding.  The first two evaluate the reference's expressions operation by operation (contraction off: torch rounds after every op).  The third
// spells out the roundings of cfg_combine_kernel and ddim_eta_step_kernel (step_kernels.hip), so that it rounds as those two launches do.
#include <cmath>

#include "common.h"

namespace etainv {

constexpr int DDPM_MAX_STEPS = ETAINV_DDPM_MAX_STEPS;   // sample_latents: all steps of a schedule
constexpr int DDPM_MAX_CHUNK = ETAINV_DDPM_MAX_CHUNK;   // invert_steps: steps per launch

struct DdpmSampleTab { float a[DDPM_MAX_STEPS], b[DDPM_MAX_STEPS]; };
struct DdpmStepTab { float s1m_t[DDPM_MAX_CHUNK], sa_t[DDPM_MAX_CHUNK], sa_p[DDPM_MAX_CHUNK], dir[DDPM_MAX_CHUNK], sigma[DDPM_MAX_CHUNK]; };
struct DdpmScales { float g[4]; };

// a x + b r as torch evaluates `x * a + r * b`: two products, one sum
__device__ __forceinline__ float ddpm_axbr(float x, float a, float r, float b) {
#pragma clang fp contract(off)
  const float p = x * a, q = r * b;
  return p + q;
}

__device__ __forceinline__ float ddpm_cfg(float u, float c, float g) {
#pragma clang fp contract(off)
  const float d = c - u;
  const float s = g * d;
  return u + s;
}

// :178-196 for one element.  sigma == 0 (t = 0 under steps_offset = 0): the reference divides by zero; here z = 0 and the latent is mu.
__device__ __forceinline__ void ddpm_invert_one(float xt, float xm, float eps, float s1m_t, float sa_t, float sa_p, float dir, float sigma,
                                                float& z, float& xo) {
#pragma clang fp contract(off)
  const float se = s1m_t * eps;
  const float x0 = (xt - se) / sa_t;
  const float d = dir * eps;
  const float m = sa_p * x0;
  const float mu = m + d;
  if (sigma == 0.f) {
    z = 0.f;
    xo = mu;
    return;
  }
  const float r = xm - mu;
  z = r / sigma;
  const float sz = sigma * z;
  xo = mu + sz;
}

// x_t from x_0 (:118): grid.y = step in draw order (ascending t), plus one row that copies x_0 to xts[n_steps]
__global__ void __launch_bounds__(256) ddpm_sample_x0_kernel(const f32x4* __restrict__ x0, const f32x4* __restrict__ noise, DdpmSampleTab tab,
                                                             int n_steps, int64_t row4, f32x4* __restrict__ xts) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= row4) return;
  const int s = blockIdx.y;
  const f32x4 x = x0[i];
  if (s == n_steps) {
    xts[(int64_t)n_steps * row4 + i] = x;
    return;
  }
  const f32x4 r = noise[(int64_t)s * row4 + i];
  const float a = tab.a[s], b = tab.b[s];
  f32x4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o[c] = ddpm_axbr(x[c], a, r[c], b);
  xts[(int64_t)(n_steps - 1 - s) * row4 + i] = o;
}

// x_t from x_{t-1} (:121-125): every element walks the steps in its own thread; the noise loads do not depend on the chain
__global__ void __launch_bounds__(64) ddpm_sample_chain_kernel(const f32x4* __restrict__ x0, const f32x4* __restrict__ noise, DdpmSampleTab tab,
                                                               int n_steps, int64_t row4, f32x4* __restrict__ xts) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= row4) return;
  f32x4 cur = x0[i];
  xts[(int64_t)n_steps * row4 + i] = cur;
#pragma unroll 4
  for (int s = 0; s < n_steps; ++s) {
    const f32x4 r = noise[(int64_t)s * row4 + i];
    const float a = tab.a[s], b = tab.b[s];
#pragma unroll
    for (int c = 0; c < 4; ++c) cur[c] = ddpm_axbr(cur[c], a, r[c], b);
    xts[(int64_t)(n_steps - 1 - s) * row4 + i] = cur;
  }
}

// grid.y = step of the chunk; step j works on xts[first + j] (x_t) and xts[first + j + 1] (x_{t-1})
__global__ void __launch_bounds__(256) ddpm_invert_steps_kernel(const f32x4* __restrict__ xts, int first, const f32x4* __restrict__ eps_u,
                                                                const f32x4* __restrict__ eps_c, float g, DdpmStepTab tab, int64_t row4,
                                                                f32x4* __restrict__ z_out, f32x4* __restrict__ x_out, f32x4* __restrict__ eps_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= row4) return;
  const int j = blockIdx.y;
  const int64_t o = (int64_t)j * row4 + i;
  const f32x4 xt = xts[(int64_t)(first + j) * row4 + i], xm = xts[(int64_t)(first + j + 1) * row4 + i];
  f32x4 eps = eps_c[o];
  if (eps_u) {
    const f32x4 u = eps_u[o];
#pragma unroll
    for (int c = 0; c < 4; ++c) eps[c] = ddpm_cfg(u[c], eps[c], g);
  }
  const float s1m_t = tab.s1m_t[j], sa_t = tab.sa_t[j], sa_p = tab.sa_p[j], dir = tab.dir[j], sigma = tab.sigma[j];
  f32x4 z, xo;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    float zc, xc;
    ddpm_invert_one(xt[c], xm[c], eps[c], s1m_t, sa_t, sa_p, dir, sigma, zc, xc);
    z[c] = zc;
    xo[c] = xc;
  }
  z_out[o] = z;
  x_out[o] = xo;
  if (eps_out) eps_out[o] = eps;
}

// The roundings of cfg_combine_kernel and ddim_eta_step_kernel (step_kernels.hip; fp32, no mask, with noise) as the compiler contracts them
// under build.sh's flags, written out so that they do not depend on how it contracts THIS kernel (a first version repeated their expressions
// and was contracted differently: a fused sum where ddim_eta_step_kernel has two products and an add).  tests/test_ddpm_kernels_gpu.py
// holds the two forms together bit for bit; if a compiler changes the contraction of those kernels, it fails and these follow.
//   eps = fma(g, c - u, u)                                   x0 = fma(-s1m_t, eps, x) / sa_t
//   dir = sqrt(fma(-std_t, std_t, 1 - a_p))                  x' = fma(std_t, z, sa_p x0 + dir eps)   (two products, one sum, then the fma)
__device__ __forceinline__ float ddpm_cfg_fused(float u, float c, float g) {
#pragma clang fp contract(off)
  return fmaf(g, c - u, u);
}
__device__ __forceinline__ float ddpm_dir(float a_p, float std_t) {
#pragma clang fp contract(off)
  return sqrtf(fmaf(-std_t, std_t, 1.f - a_p));
}
__device__ __forceinline__ float ddpm_eta_step(float x, float eps, float z, float sa_t, float s1m_t, float sa_p, float dir, float std_t) {
#pragma clang fp contract(off)
  const float x0 = fmaf(-s1m_t, eps, x) / sa_t;
  const float m = sa_p * x0, d = dir * eps;
  const float s = m + d;
  return fmaf(std_t, z, s);
}

// grid.y = prompt; rows [p0 x n_img, p1 x n_img, ..]; z [n_img] is shared by the prompt rows of an image.
__global__ void __launch_bounds__(256) ddpm_backward_step_kernel(const f32x4* __restrict__ x, const f32x4* __restrict__ eps_u,
                                                                 const f32x4* __restrict__ eps_c, DdpmScales gs, const f32x4* __restrict__ noise,
                                                                 float eta, float sa_t, float s1m_t, float sa_p, float a_p, float var,
                                                                 int64_t img4, f32x4* __restrict__ out_x, f32x4* __restrict__ out_eps) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= img4) return;
  const int p = blockIdx.y;
  const float g = gs.g[p];
  const int64_t o = (int64_t)p * img4 + i;
  const f32x4 xv = x[o], u = eps_u[o], cc = eps_c[o], zv = noise[i];
  const float std_t = eta * sqrtf(var);
  const float dir = ddpm_dir(a_p, std_t);
  f32x4 xo, eo;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    eo[c] = ddpm_cfg_fused(u[c], cc[c], g);
    xo[c] = ddpm_eta_step(xv[c], eo[c], zv[c], sa_t, s1m_t, sa_p, dir, std_t);
  }
  out_x[o] = xo;
  if (out_eps) out_eps[o] = eo;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace etainv

using namespace etainv;

extern "C" int etainv_ddpm_sample_latents(const float* x0, const float* noise, const double* ab_host, int markovian, float* xts, int n_steps,
                                          int n_img, int l, void* stream) {
  ETAINV_CHECK(x0 && noise && ab_host && xts, "null pointer");
  ETAINV_CHECK(l >= 8 && l <= 96, "latent side l must be in [8, 96]");
  ETAINV_CHECK(n_steps >= 1 && n_img >= 1, "n_steps and n_img must be at least 1");
  ETAINV_CHECK(n_steps <= DDPM_MAX_STEPS, "more steps than the table in the kernel arguments holds (ETAINV_DDPM_MAX_STEPS)");
  ETAINV_CHECK(markovian == 0 || markovian == 1, "markovian must be 0 or 1");
  ETAINV_CHECK(aligned16(x0) && aligned16(noise) && aligned16(xts), "tensors must be 16-byte aligned");
  DdpmSampleTab tab;
  for (int s = 0; s < n_steps; ++s) {
    ETAINV_CHECK(std::isfinite(ab_host[2 * s]) && std::isfinite(ab_host[2 * s + 1]), "non-finite coefficient");
    tab.a[s] = (float)ab_host[2 * s];
    tab.b[s] = (float)ab_host[2 * s + 1];
  }
  for (int s = n_steps; s < DDPM_MAX_STEPS; ++s) tab.a[s] = tab.b[s] = 0.f;
  const int64_t row4 = (int64_t)n_img * l * l;   // float4s of one step: n_img * 4 l l / 4
  ETAINV_CHECK(row4 / 64 + 1 < 2147483647LL, "too many images");
  const f32x4 *x4 = (const f32x4*)x0, *r4 = (const f32x4*)noise;
  if (markovian)
    hipLaunchKernelGGL(ddpm_sample_chain_kernel, dim3(cdiv(row4, 64)), dim3(64), 0, (hipStream_t)stream, x4, r4, tab, n_steps, row4, (f32x4*)xts);
  else
    hipLaunchKernelGGL(ddpm_sample_x0_kernel, dim3(cdiv(row4, 256), n_steps + 1), dim3(256), 0, (hipStream_t)stream, x4, r4, tab, n_steps, row4,
                       (f32x4*)xts);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

extern "C" int etainv_ddpm_invert_steps(const float* xts, int n_steps, int first, int k, const float* eps_u, const float* eps_c, float g,
                                        const double* coef_host, float* z, float* x_out, float* eps_out, int n_img, int l, void* stream) {
  ETAINV_CHECK(xts && eps_c && coef_host && z && x_out, "null pointer");
  ETAINV_CHECK(l >= 8 && l <= 96, "latent side l must be in [8, 96]");
  ETAINV_CHECK(n_steps >= 1 && k >= 1 && n_img >= 1, "n_steps, k and n_img must be at least 1");
  ETAINV_CHECK(k <= DDPM_MAX_CHUNK, "more steps in one launch than the table in the kernel arguments holds (ETAINV_DDPM_MAX_CHUNK)");
  ETAINV_CHECK(first >= 0 && (int64_t)first + k <= n_steps, "steps [first, first + k) must lie inside [0, n_steps)");
  ETAINV_CHECK(std::isfinite(g), "the guidance scale must be finite");
  ETAINV_CHECK(aligned16(xts) && aligned16(eps_u) && aligned16(eps_c) && aligned16(z) && aligned16(x_out) && aligned16(eps_out),
               "tensors must be 16-byte aligned");
  DdpmStepTab tab;
  for (int j = 0; j < DDPM_MAX_CHUNK; ++j) {
    float v[5] = {0.f, 1.f, 0.f, 0.f, 0.f};
    if (j < k)
      for (int q = 0; q < 5; ++q) {
        ETAINV_CHECK(std::isfinite(coef_host[5 * j + q]), "non-finite coefficient");
        v[q] = (float)coef_host[5 * j + q];
      }
    ETAINV_CHECK(v[1] > 0.f && v[4] >= 0.f, "sqrt(alpha_bar_t) must be positive and sigma non-negative");
    tab.s1m_t[j] = v[0];
    tab.sa_t[j] = v[1];
    tab.sa_p[j] = v[2];
    tab.dir[j] = v[3];
    tab.sigma[j] = v[4];
  }
  const int64_t row4 = (int64_t)n_img * l * l;
  ETAINV_CHECK(row4 / 256 + 1 < 2147483647LL, "too many images");
  hipLaunchKernelGGL(ddpm_invert_steps_kernel, dim3(cdiv(row4, 256), k), dim3(256), 0, (hipStream_t)stream, (const f32x4*)xts, first,
                     (const f32x4*)eps_u, (const f32x4*)eps_c, g, tab, row4, (f32x4*)z, (f32x4*)x_out, (f32x4*)eps_out);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

extern "C" int etainv_ddpm_backward_step(const float* x, const float* eps_u, const float* eps_c, const float* g_host, int n_prompts,
                                         const float* z, float a_t, float a_p, float var, float* out_x, float* out_eps, int n_img, int l,
                                         void* stream) {
  ETAINV_CHECK(x && eps_u && eps_c && g_host && z && out_x, "null pointer");
  ETAINV_CHECK(l >= 8 && l <= 96, "latent side l must be in [8, 96]");
  ETAINV_CHECK(n_img >= 1, "n_img must be at least 1");
  ETAINV_CHECK(n_prompts >= 1 && n_prompts <= 4, "n_prompts must be in [1, 4]");
  ETAINV_CHECK(a_t > 0.f && a_t < 1.f && a_p > 0.f && a_p <= 1.f, "alphas_cumprod out of range");
  ETAINV_CHECK(std::isfinite(var) && var >= 0.f, "the variance must be finite and non-negative");
  ETAINV_CHECK(aligned16(x) && aligned16(eps_u) && aligned16(eps_c) && aligned16(z) && aligned16(out_x) && aligned16(out_eps),
               "tensors must be 16-byte aligned");
  DdpmScales gs = {{0.f, 0.f, 0.f, 0.f}};
  for (int p = 0; p < n_prompts; ++p) {
    ETAINV_CHECK(std::isfinite(g_host[p]), "every guidance scale must be finite");
    gs.g[p] = g_host[p];
  }
  const int64_t img4 = (int64_t)n_img * l * l;
  ETAINV_CHECK(img4 / 256 + 1 < 2147483647LL, "too many images");
  hipLaunchKernelGGL(ddpm_backward_step_kernel, dim3(cdiv(img4, 256), n_prompts), dim3(256), 0, (hipStream_t)stream, (const f32x4*)x,
                     (const f32x4*)eps_u, (const f32x4*)eps_c, gs, (const f32x4*)z, 1.0f, (float)sqrt((double)a_t),
                     (float)sqrt(1.0 - (double)a_t), (float)sqrt((double)a_p), a_p, var, img4, (f32x4*)out_x, (f32x4*)out_eps);
  ETAINV_LAUNCH_CHECK();
  return 0;
}
