// Noise regularisation of pix2pix-zero's regularised DDIM inversion, one launch per inversion step:
//   CFG combine -> num_reg_steps x (num_ac_rolls autocorrelation-gradient steps + 1 KL-gradient step) -> DDIM inverse step
//   regularized_diffusion_inversion.py:42-69 (auto_corr_loss), :71-83 (kl_divergence), :86-114 (regularize_noise_pred), :116-137
// The reference differentiates the two losses with autograd (well over a thousand eager launches per step); both gradients are closed-form:
//   L_ac  = sum over channels and pyramid levels of mean(n roll(n, r, rows))^2 + mean(n roll(n, r, cols))^2, level k+1 = avg_pool2d(level k, 2)
//           d/dn at a level of size s, m = that mean: 2 m / s^2 (roll(n, r) + roll(n, -r)) per axis; to the finer level through the pool's
//           adjoint: value / 4 over the 2 x 2 block, nothing for a dropped last row / column
//   L_kl  = var + mu^2 - 1 - log(var + 1e-7) over all N = 4 l^2 values (unbiased var): d/de = 2 (e - mu) / (N - 1) (1 - 1 / (var + 1e-7)) + 2 mu / N
//
// One workgroup of 1024 threads per image; channel c runs on the four waves [4c, 4c + 4), the channels in lock-step (same levels, own
// shifts).  A thread owns the level-0 values tc + 256 q of its channel and keeps them in registers for the whole call; neighbours read the
// published copy of level 0 -- in LDS up to l = 64, in eps_out (L2-resident, visible inside the workgroup after a barrier) above, where
// level 0 does not fit beside the pyramids.  Levels >= 1 and their gradients live in LDS.  One autocorrelation step:
//   publish level 0 | per level: partial sums of both products + pool the next level | wave + LDS reduction, fixed order | gradient per
//   level from coarse to fine, each adding a quarter of its parent's | level 0: e -= lambda_ac / rolls * gradient, in registers
// Every reduction has a fixed order and nothing depends on the grid: an image's result is independent of n_img and of its position, and
// bit-identical from run to run.  No atomics.
#include <cmath>

#include "common.h"

namespace etainv {

constexpr int REG_THREADS = 1024;   // 4 channels x 256
constexpr int REG_MAXLEV = 5;       // 96 -> 48 -> 24 -> 12 -> 6
constexpr int REG_LMIN = 8, REG_LMAX = 96;

struct RegParams {
  const float* eps_u;
  const float* eps_c;
  float* eps_out;
  const float* x;
  float* x_out;
  const int32_t* shifts;
  float g, s1f, isf, st, s1t;   // DDIM inverse step scalars as in etainv_ddim_step
  float lam_ac_roll, lam_kl;    // lambda_ac / num_ac_rolls, lambda_kl
  int do_ac, do_kl, n_reg, n_roll;
  int l, nlev;
  int size[REG_MAXLEV];         // side of level k
  int off[REG_MAXLEV];          // float offset of level k >= 1 inside one channel's pyramid block
  int pyr;                      // floats of one channel's levels >= 1
};

// a shift read from device memory addresses LDS: anything outside [0, s) is taken as 0 instead of being trusted
__device__ __forceinline__ int reg_shift(const int32_t* sh, int k, int s) {
  const int r = __builtin_amdgcn_readfirstlane(sh[k]);
  return (unsigned)r < (unsigned)s ? r : 0;
}

// g(i, j) = wr (n[i - r][j] + n[i + r][j]) + wc (n[i][j - r] + n[i][j + r]), indices mod s
__device__ __forceinline__ float reg_level_grad(const float* n, int s, int i, int j, int r, float wr, float wc) {
  int im = i - r, ip = i + r, jm = j - r, jp = j + r;
  im += im < 0 ? s : 0;
  ip -= ip >= s ? s : 0;
  jm += jm < 0 ? s : 0;
  jp -= jp >= s ? s : 0;
  return wr * (n[im * s + j] + n[ip * s + j]) + wc * (n[i * s + jm] + n[i * s + jp]);
}

// partial sums of n[i][j] n[i - r][j] and n[i][j] n[i][j - r] over the elements tc, tc + 256, .. of a level held in `n`
__device__ __forceinline__ void reg_level_products(const float* n, int s, int r, int tc, float& pr, float& pc) {
  const int s2 = s * s, di = 256 / s, dj = 256 % s;
  int i = tc / s, j = tc - i * s;
  float ar = 0.f, ac = 0.f;
#pragma nounroll
  for (int idx = tc; idx < s2; idx += 256) {
    int im = i - r, jm = j - r;
    im += im < 0 ? s : 0;
    jm += jm < 0 ? s : 0;
    const float v = n[idx];
    ar = fmaf(v, n[im * s + j], ar);
    ac = fmaf(v, n[i * s + jm], ac);
    i += di;
    j += dj;
    if (j >= s) { j -= s; ++i; }
  }
  pr = ar;
  pc = ac;
}

// next[i][j] = mean of the 2 x 2 block of `n` (side s) at (2i, 2j); next has side s / 2 (floor: a last odd row / column is dropped)
__device__ __forceinline__ void reg_pool(const float* n, int s, float* next, int tc) {
  const int h = s >> 1, h2 = h * h, di = 256 / h, dj = 256 % h;
  int i = tc / h, j = tc - i * h;
#pragma nounroll
  for (int idx = tc; idx < h2; idx += 256) {
    const float* p = n + (2 * i) * s + 2 * j;
    next[idx] = 0.25f * (((p[0] + p[1]) + p[s]) + p[s + 1]);
    i += di;
    j += dj;
    if (j >= h) { j -= h; ++i; }
  }
}

template <int MAXQ, bool L0_LDS>
__global__ void __launch_bounds__(REG_THREADS) noise_regularize_kernel(RegParams p) {
  extern __shared__ float smem[];
  __shared__ float red_ac[4][4][2 * REG_MAXLEV];
  __shared__ float red_kl[2][16];
  const int tid = threadIdx.x, tc = tid & 255, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = wave >> 2, wg = wave & 3;   // wave-uniform: scalar bases, vector offsets
  const int l = p.l, l2 = l * l;
  const int64_t ch_off = ((int64_t)blockIdx.x * 4 + c) * l2;
  float* l0;
  if constexpr (L0_LDS) l0 = smem + c * l2;
  else l0 = p.eps_out + ch_off;
  float* pyr_n = smem + (L0_LDS ? 4 * l2 : 0) + c * p.pyr;
  float* pyr_g = smem + (L0_LDS ? 4 * l2 : 0) + (4 + c) * p.pyr;
  const int di0 = 256 / l, dj0 = 256 % l;

  // ---- guided noise into registers (element tc + 256 q of channel c); every element is read by its owner only, so eps_out may be eps_c
  // (the loops over the owned elements are branch-free: a slot without an element -- tc + 256 q >= l^2 -- works on element 0 and keeps its 0)
  float e[MAXQ];
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    const bool own = tc + 256 * q < l2;
    const int64_t a = ch_off + (own ? tc + 256 * q : 0);
    const float cv = p.eps_c[a];
    const float u = p.eps_u ? p.eps_u[a] : cv;
    e[q] = own ? (p.eps_u ? u + p.g * (cv - u) : cv) : 0.f;
    if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }

  const float n_all = 4.f * (float)l2;
  for (int outer = 0; outer < p.n_reg; ++outer) {
    if (p.do_ac) {
      for (int roll = 0; roll < p.n_roll; ++roll) {
        // the index chains below (row / column of every owned element at every level) do not change from step to step; left visible as
        // loop invariants they are all hoisted and kept live across the step loops, where the registers are needed for e[] -- so each
        // step derives them from a copy of the thread index the optimiser cannot see through
        int tl = tc;
        asm volatile("" : "+v"(tl));
        const int32_t* sh = p.shifts + ((int64_t)(outer * p.n_roll + roll) * 4 + c) * p.nlev;
        // publish level 0
#pragma unroll
        for (int q = 0; q < MAXQ; ++q) {
          const int idx = tl + 256 * q;
          if (idx < l2) l0[idx] = e[q];
          if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
        __syncthreads();
        // products of every level, pooling the next one on the way
        float pr[REG_MAXLEV], pc[REG_MAXLEV];
        int rk[REG_MAXLEV];
        {
          const int r = reg_shift(sh, 0, l);
          rk[0] = r;
          float ar = 0.f, ac = 0.f;
          int i = tl / l, j = tl - (tl / l) * l;
#pragma unroll
          for (int q = 0; q < MAXQ; ++q) {
            const bool own = tl + 256 * q < l2;                    // (e[q] == 0 otherwise: the products add nothing)
            const int ii = own ? i : 0, jj = own ? j : 0;
            int im = ii - r, jm = jj - r;
            im += im < 0 ? l : 0;
            jm += jm < 0 ? l : 0;
            ar = fmaf(e[q], l0[im * l + jj], ar);
            ac = fmaf(e[q], l0[ii * l + jm], ac);
            i += di0;
            j += dj0;
            if (j >= l) { j -= l; ++i; }
            if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four elements in flight, not MAXQ: the registers hold e[]
          }
          pr[0] = ar;
          pc[0] = ac;
          if (p.nlev > 1) {
            reg_pool(l0, l, pyr_n + p.off[1], tl);
            __syncthreads();
          }
        }
#pragma unroll
        for (int k = 1; k < REG_MAXLEV; ++k) {
          pr[k] = pc[k] = 0.f;
          rk[k] = 0;
          if (k < p.nlev) {
            const int s = p.size[k];
            rk[k] = reg_shift(sh, k, s);
            reg_level_products(pyr_n + p.off[k], s, rk[k], tl, pr[k], pc[k]);
            if (k + 1 < p.nlev) {
              reg_pool(pyr_n + p.off[k], s, pyr_n + p.off[k + 1], tl);
              __syncthreads();
            }
          }
        }
        // the means: wave sums, then the four waves of the channel in a fixed order
#pragma unroll
        for (int k = 0; k < REG_MAXLEV; ++k) {
          if (k < p.nlev) {
            const float a = wave_sum(pr[k]), b = wave_sum(pc[k]);
            if (lane == 0) {
              red_ac[c][wg][2 * k] = a;
              red_ac[c][wg][2 * k + 1] = b;
            }
          }
        }
        __syncthreads();
        float wr[REG_MAXLEV], wc[REG_MAXLEV];
#pragma unroll
        for (int k = 0; k < REG_MAXLEV; ++k) {
          wr[k] = wc[k] = 0.f;
          if (k < p.nlev) {
            const float cnt = (float)(p.size[k] * p.size[k]);
            const float sr = (red_ac[c][0][2 * k] + red_ac[c][1][2 * k]) + (red_ac[c][2][2 * k] + red_ac[c][3][2 * k]);
            const float sc = (red_ac[c][0][2 * k + 1] + red_ac[c][1][2 * k + 1]) + (red_ac[c][2][2 * k + 1] + red_ac[c][3][2 * k + 1]);
            wr[k] = 2.f * (sr / cnt) / cnt;
            wc[k] = 2.f * (sc / cnt) / cnt;
          }
        }
        // gradients from coarse to fine
#pragma unroll
        for (int k = REG_MAXLEV - 1; k >= 1; --k) {
          if (k < p.nlev) {
            const int s = p.size[k], s2 = s * s, dis = 256 / s, djs = 256 % s;
            const bool child = k + 1 < p.nlev;
            const int sc = child ? p.size[k + 1] : 0;
            const float* n = pyr_n + p.off[k];
            const float* gc = pyr_g + (child ? p.off[k + 1] : 0);
            float* gk = pyr_g + p.off[k];
            int i = tl / s, j = tl - (tl / s) * s;
#pragma nounroll
            for (int idx = tl; idx < s2; idx += 256) {
              float g = reg_level_grad(n, s, i, j, rk[k], wr[k], wc[k]);
              if (child && i < 2 * sc && j < 2 * sc) g += 0.25f * gc[(i >> 1) * sc + (j >> 1)];
              gk[idx] = g;
              i += dis;
              j += djs;
              if (j >= s) { j -= s; ++i; }
            }
            __syncthreads();
          }
        }
        {
          const bool child = p.nlev > 1;
          const int sc = child ? p.size[1] : 0;
          const float* gc = pyr_g + (child ? p.off[1] : 0);
          int tg = tc;                            // (a copy of its own: the products' row / column chain is not kept for this loop)
          asm volatile("" : "+v"(tg));
          int i = tg / l, j = tg - (tg / l) * l;
#pragma unroll
          for (int q = 0; q < MAXQ; ++q) {
            const bool own = tg + 256 * q < l2;
            const int ii = own ? i : 0, jj = own ? j : 0;
            float g = reg_level_grad(l0, l, ii, jj, rk[0], wr[0], wc[0]);
            const bool par = child && ii < 2 * sc && jj < 2 * sc;
            g += par ? 0.25f * gc[par ? (ii >> 1) * sc + (jj >> 1) : 0] : 0.f;
            e[q] = own ? fmaf(-p.lam_ac_roll, g, e[q]) : 0.f;
            i += di0;
            j += dj0;
            if (j >= l) { j -= l; ++i; }
            if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // four elements in flight, not MAXQ: the registers hold e[]
          }
        }
        __syncthreads();   // every read of the published level 0 is done before the next step overwrites it
      }
    }
    if (p.do_kl) {
      int tk = tc;                              // (as in the step loop: the ownership predicates are derived here)
      asm volatile("" : "+v"(tk));
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < MAXQ; ++q) s += e[q];      // (unowned slots hold 0)
      s = wave_sum(s);
      if (lane == 0) red_kl[0][wave] = s;
      __syncthreads();
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) tot += red_kl[0][w];
      const float mu = tot / n_all;
      float v = 0.f;
#pragma unroll
      for (int q = 0; q < MAXQ; ++q) {
        const float d = tk + 256 * q < l2 ? e[q] - mu : 0.f;
        v = fmaf(d, d, v);
      }
      v = wave_sum(v);
      if (lane == 0) red_kl[1][wave] = v;
      __syncthreads();
      float totv = 0.f;
#pragma unroll
      for (int w = 0; w < 16; ++w) totv += red_kl[1][w];
      const float var = totv / (n_all - 1.f);
      const float ka = 2.f / (n_all - 1.f) * (1.f - 1.f / (var + 1e-7f)), kb = 2.f * mu / n_all;
#pragma unroll
      for (int q = 0; q < MAXQ; ++q)
        e[q] = tk + 256 * q < l2 ? fmaf(-p.lam_kl, fmaf(ka, e[q] - mu, kb), e[q]) : 0.f;
    }
  }

  // ---- regularised noise out, and the DDIM inverse step on it (ddim_step_kernel's arithmetic)
  int tf = tc;                                  // (as in the step loop: addresses derived here, not carried from the load)
  asm volatile("" : "+v"(tf));
#pragma unroll
  for (int q = 0; q < MAXQ; ++q) {
    const int idx = tf + 256 * q;
    if (idx < l2) {
      p.eps_out[ch_off + idx] = e[q];
      if (p.x) {
        const float x0 = (p.x[ch_off + idx] - p.s1f * e[q]) * p.isf;
        p.x_out[ch_off + idx] = p.st * x0 + p.s1t * e[q];
      }
    }
    if ((q & 3) == 3) __builtin_amdgcn_sched_barrier(0);
  }
}

template <int MAXQ, bool L0_LDS>
static int launch_noise_regularize(const RegParams& p, int n_img, size_t lds, hipStream_t s) {
  allow_dynamic_lds<&noise_regularize_kernel<MAXQ, L0_LDS>>(160 * 1024 - sizeof(float) * (4 * 4 * 2 * REG_MAXLEV + 2 * 16));
  hipLaunchKernelGGL((noise_regularize_kernel<MAXQ, L0_LDS>), dim3(n_img), dim3(REG_THREADS), lds, s, p);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

}  // namespace etainv

using namespace etainv;

extern "C" int etainv_noise_regularize(const float* eps_u, const float* eps_c, float g, float* eps_out, const float* x, float a_from, float a_to,
                                       float* x_out, int n_img, int l, const int32_t* shifts_dev, int num_reg_steps, int num_ac_rolls,
                                       float lambda_ac, float lambda_kl, void* stream) {
  ETAINV_CHECK(eps_c && eps_out, "null pointer: eps_c and eps_out are required");
  ETAINV_CHECK(!x || x_out, "x given without x_out");
  ETAINV_CHECK(l >= REG_LMIN && l <= REG_LMAX, "l must be in [8, 96]");
  ETAINV_CHECK(n_img >= 0 && num_reg_steps >= 0 && num_ac_rolls >= 0, "negative count (n_img, num_reg_steps, num_ac_rolls)");
  ETAINV_CHECK(!eps_u || std::isfinite(g), "g must be finite");
  ETAINV_CHECK(std::isfinite(lambda_ac) && std::isfinite(lambda_kl), "lambda_ac and lambda_kl must be finite");
  ETAINV_CHECK(std::isfinite(a_from) && std::isfinite(a_to), "a_from and a_to must be finite");
  ETAINV_CHECK(!x || (a_from > 0.f && a_from <= 1.f && a_to > 0.f && a_to <= 1.f), "alphas_cumprod must be in (0,1]");
  ETAINV_CHECK(!(lambda_ac > 0.f) || num_ac_rolls > 0, "num_ac_rolls must be positive when lambda_ac > 0");
  const bool do_ac = lambda_ac > 0.f && num_reg_steps > 0 && num_ac_rolls > 0;
  ETAINV_CHECK(!do_ac || shifts_dev, "null pointer: shifts_dev is required when the autocorrelation steps run");
  if (n_img == 0) return 0;
  RegParams p = {};
  p.eps_u = eps_u;
  p.eps_c = eps_c;
  p.eps_out = eps_out;
  p.x = x;
  p.x_out = x_out;
  p.shifts = shifts_dev;
  p.g = g;
  if (x) {
    p.s1f = (float)sqrt(1.0 - (double)a_from);
    p.isf = (float)(1.0 / sqrt((double)a_from));
    p.st = (float)sqrt((double)a_to);
    p.s1t = (float)sqrt(1.0 - (double)a_to);
  }
  p.do_ac = do_ac;
  p.do_kl = lambda_kl > 0.f && num_reg_steps > 0;
  p.n_reg = (p.do_ac || p.do_kl) ? num_reg_steps : 0;
  p.n_roll = num_ac_rolls;
  p.lam_ac_roll = do_ac ? lambda_ac / (float)num_ac_rolls : 0.f;
  p.lam_kl = lambda_kl;
  p.l = l;
  int s = l, off = 0;
  for (;;) {                                       // auto_corr_loss :61-68: the loss at a level, then pool while the level is above 8
    ETAINV_CHECK(p.nlev < REG_MAXLEV, "pyramid deeper than the kernel's levels");
    p.size[p.nlev] = s;
    p.off[p.nlev] = p.nlev ? off : 0;
    if (p.nlev) off += s * s;
    ++p.nlev;
    if (s <= 8) break;
    s /= 2;
  }
  p.pyr = off;
  const bool l0_lds = l <= 64;
  const size_t lds = sizeof(float) * ((l0_lds ? 4 * (size_t)l * l : 0) + 8 * (size_t)p.pyr);
  ETAINV_CHECK(lds <= 150 * 1024, "LDS plan above the workgroup's share");
  hipStream_t st = (hipStream_t)stream;
  if (l <= 32) return launch_noise_regularize<4, true>(p, n_img, lds, st);
  if (l <= 64) return launch_noise_regularize<16, true>(p, n_img, lds, st);
  return launch_noise_regularize<36, false>(p, n_img, lds, st);
}
