// Proximal guidance of proximal negative-prompt inversion, one launch per backward step:
//   d = eps_c - eps_u -> threshold = a quantile of |d| over the group -> shrink d -> eps_u + g d' -> DDIM step
//   proximal_negative_prompt_inversion.py:61-128 (proximal_guidance), :130-151 (predict_noise)
// The reference takes the threshold from torch.quantile, which sorts.  Here it is an exact selection: |d| is non-negative, so the values order as
// their bit patterns, and a radix select over the patterns (four 8-bit digits, from the top) finds the order statistic v_k with integer
// histograms only; v_k+1 is v_k again when rank k + 1 still falls inside the run of values equal to v_k, else the smallest value above v_k (an
// integer minimum).  The host splits the rank (etainv.pipeline.ProximalGuidance.rank_split); the kernel selects and interpolates with torch's
// lerp rule.
//
// One workgroup of 1024 threads per group (the rows of one image pair: they share a threshold).  A thread owns the values tid + 1024 q of the
// group.  Up to 32,768 values they stay in registers for the whole call; above, d is written to eps_out once and each pass reads its own
// values back (a thread reads what it wrote itself: no barrier, and eps_out may be eps_c).  One digit:
//   16 copies of the LDS histogram, a lane adds to copy (lane & 15), integer atomics | merged by 256 threads | one wave scans the 256 bins
//   and picks the digit
// (the copies: a wave's 64 values share a handful of leading digits -- sign and seven exponent bits -- and 64 atomics on one address take 64
// LDS cycles, which made a pass cost one cycle per value; copy c of bin b lies at word 16 b + c, so the 16 copies of a bin are 16 banks)
// Every sum and every minimum is over integers, so nothing depends on the order of arrival; nothing depends on the grid: a group's result is
// independent of n_groups and of its position, and bit-identical from run to run.  No floating-point atomics.
#include <cmath>

#include "kernels.h"

namespace etainv {

constexpr int PROX_THREADS = 1024, PROX_COPIES = 16, PROX_BINS = 256;
constexpr int PROX_LMIN = 8, PROX_LMAX = 96, PROX_MAXROWS = 4;
constexpr unsigned PROX_INF = 0x7f800000u;

struct ProxParams {
  const float* eps_u;
  const float* eps_c;
  float* eps_out;
  const float* x;
  float* x_out;
  float* thr_out;
  float g, thr_fixed, rank_w;
  float s1f, isf, st, s1t;      // DDIM step scalars as in etainv_ddim_step
  int l1, use_rank;
  int rank_lo, rank_hi;         // k and min(k + 1, n - 1)
  int n, row_len, n_groups;     // values of a group, values of a row (4 l^2)
};

// the three reference lines (:88-90 for l1, :108 for l0) and the guided noise (:119); no contraction: every operation rounds once, as torch's does
__device__ __forceinline__ float prox_guide(float d, float u, float thr, float g, bool l1) {
#pragma clang fp contract(off)
  float dp = d - fminf(fmaxf(d, -thr), thr);
  if (l1) {
    dp = dp > 0.f ? dp - thr : dp;
    dp = dp < 0.f ? dp + thr : dp;
  }
  dp = thr != thr ? thr : dp;     // a NaN threshold: clamp gives NaN everywhere (fminf / fmaxf would drop it)
  return u + g * dp;
}

// torch.lerp(v_k, v_k+1, w)
__device__ __forceinline__ float prox_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float diff = b - a;
  return w < 0.5f ? a + w * diff : b - diff * (1.f - w);
}

template <int Q>   // Q > 0: the owned values live in registers (n <= 1024 Q); Q == 0: in eps_out
__global__ void __launch_bounds__(PROX_THREADS) prox_guidance_kernel(ProxParams p) {
  __shared__ unsigned copy_hist[PROX_BINS][PROX_COPIES];
  __shared__ unsigned hist[PROX_BINS];
  __shared__ unsigned sel[4];   // digit chosen, rank inside its bin, size of its bin, a NaN was seen
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), copy = lane & (PROX_COPIES - 1);
  const int n = p.n, R = p.row_len;
  // value i of group g is element i - r R of tensor row r n_groups + g, r = i / R (at most PROX_MAXROWS rows: three compares, no division)
  const int64_t base = (int64_t)blockIdx.x * R, row_skip = (int64_t)(p.n_groups - 1) * R;
  auto addr = [&](int i) -> int64_t {
    const int r = (i >= R) + (i >= 2 * R) + (i >= 3 * R);
    return base + i + r * row_skip;
  };

  float d[Q > 0 ? Q : 1];
  if constexpr (Q > 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const bool own = tid + PROX_THREADS * q < n;
      const int64_t a = addr(own ? tid + PROX_THREADS * q : 0);
      d[q] = own ? p.eps_c[a] - p.eps_u[a] : 0.f;
    }
  } else if (p.use_rank) {
#pragma unroll 4
    for (int i = tid; i < n; i += PROX_THREADS) {
      const int64_t a = addr(i);
      p.eps_out[a] = p.eps_c[a] - p.eps_u[a];
    }
  }
  // f(pattern of |d|) over the owned values; -0.0 is 0
  auto each_key = [&](auto&& f) {
    if constexpr (Q > 0) {
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (tid + PROX_THREADS * q < n) f(__float_as_uint(d[q]) & 0x7fffffffu);
    } else {
#pragma unroll 4
      for (int i = tid; i < n; i += PROX_THREADS) f(__float_as_uint(p.eps_out[addr(i)]) & 0x7fffffffu);
    }
  };

  float thr = p.thr_fixed, vk = p.thr_fixed, vk1 = p.thr_fixed;
  if (p.use_rank) {
    for (int j = tid; j < PROX_BINS * PROX_COPIES; j += PROX_THREADS) (&copy_hist[0][0])[j] = 0u;
    if (tid == 0) sel[3] = 0u;
    __syncthreads();
    unsigned prefix = 0u, rank = (unsigned)p.rank_lo, run = 0u;   // rank: among the values whose leading digits are `prefix`
#pragma unroll
    for (int shift = 24; shift >= 0; shift -= 8) {
      bool nan = false;
      each_key([&](unsigned key) {
        if (shift == 24) nan |= key > PROX_INF;
        if (shift == 24 || (key >> ((shift + 8) & 31)) == prefix) atomicAdd(&copy_hist[(key >> shift) & 255u][copy], 1u);
      });
      if (shift == 24 && nan) sel[3] = 1u;
      __syncthreads();
      if (tid < PROX_BINS) {
        unsigned s = 0u;
#pragma unroll
        for (int c = 0; c < PROX_COPIES; ++c) {      // (starting at copy tid: neighbouring threads on different banks; integer sums have no order)
          const int cc = (c + tid) & (PROX_COPIES - 1);
          s += copy_hist[tid][cc];
          copy_hist[tid][cc] = 0u;
        }
        hist[tid] = s;
      }
      __syncthreads();
      if (wave == 0) {
        // lane j holds bins 4 j .. 4 j + 3; inclusive scan of the lane sums, then the one lane whose bins hold the rank walks its four
        unsigned b[4], s = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          b[i] = hist[4 * lane + i];
          s += b[i];
        }
        unsigned incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const unsigned t = __shfl_up(incl, o, 64);
          incl += lane >= o ? t : 0u;
        }
        unsigned below = incl - s;
        if (rank >= below && rank < incl) {
          bool found = false;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (!found && rank < below + b[i]) {
              sel[0] = (unsigned)(4 * lane + i);
              sel[1] = rank - below;
              sel[2] = b[i];
              found = true;
            }
            below += b[i];
          }
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | sel[0];
      rank = sel[1];
      run = sel[2];
    }
    // `prefix` is v_k's pattern, `rank` its place inside the run of `run` values equal to it
    unsigned next = prefix;
    if (p.rank_hi > p.rank_lo && rank + 1u >= run) {
      if (tid == 0) hist[0] = 0xffffffffu;       // (hist is free: its last reader passed the barrier above)
      __syncthreads();
      unsigned m = 0xffffffffu;
      each_key([&](unsigned key) { m = key > prefix ? min(m, key) : m; });
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor(m, o, 64));
      if (lane == 0) atomicMin(&hist[0], m);
      __syncthreads();
      next = hist[0];
    }
    vk = __uint_as_float(prefix);
    vk1 = __uint_as_float(next);
    thr = sel[3] ? __uint_as_float(0x7fc00000u) : prox_lerp(vk, vk1, p.rank_w);
  }
  if (p.thr_out && tid == 0) {
    p.thr_out[3 * blockIdx.x + 0] = thr;
    p.thr_out[3 * blockIdx.x + 1] = vk;
    p.thr_out[3 * blockIdx.x + 2] = vk1;
  }

  // ---- guided noise out, and the DDIM step on it (ddim_step_kernel's arithmetic); every element is read and written by its owner only
  auto finish = [&](int i, float dv, bool have_d) {
    const int64_t a = addr(i);
    const float u = p.eps_u[a];
    const float e = prox_guide(have_d ? dv : p.eps_c[a] - u, u, thr, p.g, p.l1 != 0);
    p.eps_out[a] = e;
    if (p.x) {
      const float x0 = (p.x[a] - p.s1f * e) * p.isf;
      p.x_out[a] = p.st * x0 + p.s1t * e;
    }
  };
  if constexpr (Q > 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q)
      if (tid + PROX_THREADS * q < n) finish(tid + PROX_THREADS * q, d[q], true);
  } else if (p.use_rank) {
#pragma unroll 4
    for (int i = tid; i < n; i += PROX_THREADS) finish(i, p.eps_out[addr(i)], true);
  } else {
#pragma unroll 4
    for (int i = tid; i < n; i += PROX_THREADS) finish(i, 0.f, false);
  }
}

template <int Q>
static int launch_prox_guidance_q(const ProxParams& p, hipStream_t s) {
  hipLaunchKernelGGL((prox_guidance_kernel<Q>), dim3(p.n_groups), dim3(PROX_THREADS), 0, s, p);
  ETAINV_LAUNCH_CHECK();
  return 0;
}

int launch_prox_guidance(const float* eps_u, const float* eps_c, float g, int mode, int use_rank, int rank_lo, float rank_w, float thr_fixed,
                         float* eps_out, const float* x, float a_from, float a_to, float* x_out, float* thr_out, int n_groups, int rows_per_group,
                         int l, hipStream_t s) {
  ETAINV_CHECK(eps_u && eps_c && eps_out, "null pointer: eps_u, eps_c and eps_out are required");
  ETAINV_CHECK(eps_out != eps_u, "eps_out may alias eps_c, not eps_u");
  ETAINV_CHECK(!x || x_out, "x given without x_out");
  ETAINV_CHECK(mode >= 0 && mode <= 2, "mode must be 0 (plain CFG), 1 (l0) or 2 (l1)");
  ETAINV_CHECK(l >= PROX_LMIN && l <= PROX_LMAX, "l must be in [8, 96]");
  ETAINV_CHECK(rows_per_group >= 1 && rows_per_group <= PROX_MAXROWS, "rows_per_group must be in [1, 4]");
  ETAINV_CHECK(n_groups >= 0, "negative n_groups");
  ETAINV_CHECK(std::isfinite(g), "g must be finite");
  ETAINV_CHECK(std::isfinite(a_from) && std::isfinite(a_to), "a_from and a_to must be finite");
  ETAINV_CHECK(!x || (a_from > 0.f && a_from <= 1.f && a_to > 0.f && a_to <= 1.f), "alphas_cumprod must be in (0,1]");
  const int row_len = 4 * l * l, n = rows_per_group * row_len;
  const bool select = mode != 0 && use_rank;
  if (select) {
    ETAINV_CHECK(rank_lo >= 0 && rank_lo <= n - 1, "rank_lo must be in [0, n - 1]");
    ETAINV_CHECK(rank_w >= 0.f && rank_w < 1.f, "rank_w must be in [0, 1)");
  } else if (mode != 0) {
    ETAINV_CHECK(std::isfinite(thr_fixed) && thr_fixed >= 0.f, "a fixed threshold must be finite and not negative");
  }
  if (n_groups == 0) return 0;
  ProxParams p = {};
  p.eps_u = eps_u;
  p.eps_c = eps_c;
  p.eps_out = eps_out;
  p.x = x;
  p.x_out = x_out;
  p.thr_out = thr_out;
  p.g = g;
  p.thr_fixed = mode == 0 ? 0.f : thr_fixed;     // plain CFG is the shrinkage with threshold 0: d - clamp(d, -0, 0) = d
  p.rank_w = rank_w;
  if (x) {
    p.s1f = (float)sqrt(1.0 - (double)a_from);
    p.isf = (float)(1.0 / sqrt((double)a_from));
    p.st = (float)sqrt((double)a_to);
    p.s1t = (float)sqrt(1.0 - (double)a_to);
  }
  p.l1 = mode == 2;
  p.use_rank = select;
  p.rank_lo = rank_lo;
  p.rank_hi = rank_lo + 1 < n ? rank_lo + 1 : n - 1;
  p.n = n;
  p.row_len = row_len;
  p.n_groups = n_groups;
  if (n <= 4 * PROX_THREADS) return launch_prox_guidance_q<4>(p, s);
  if (n <= 32 * PROX_THREADS) return launch_prox_guidance_q<32>(p, s);
  return launch_prox_guidance_q<0>(p, s);
}

}  // namespace etainv

using namespace etainv;

extern "C" int etainv_prox_guidance(const float* eps_u, const float* eps_c, float g, int mode, int use_rank, int rank_lo, float rank_w,
                                    float thr_fixed, float* eps_out, const float* x, float a_from, float a_to, float* x_out, float* thr_out,
                                    int n_groups, int rows_per_group, int l, void* stream) {
  // (the launcher's refusals carry its own name; repeat the entry point's for the caller)
  const int rc = launch_prox_guidance(eps_u, eps_c, g, mode, use_rank, rank_lo, rank_w, thr_fixed, eps_out, x, a_from, a_to, x_out, thr_out, n_groups,
                                      rows_per_group, l, (hipStream_t)stream);
  if (rc) set_error(std::string("etainv_prox_guidance: ") + etainv_last_error());
  return rc;
}
