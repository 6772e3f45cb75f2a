// Which kernel a 16-bit self-attention launch takes: the one dispatch rule of launch_self_attention_mode (attention.hip).  Plain C++ with no HIP
// include, so that a host compiler can build it: tests/test_attention_ref.py compares it with the rule the GPU tests assert their premises with.
#pragma once
#include <stdint.h>

namespace etainv {

enum SelfAttnRoute {
  SELF_D40_ONE_BLOCK_PER_WAVE,   // self_attn40_kernel<T, 40, XCD, 1, 2>: few blocks (single-image calls)
  SELF_D40_PERSISTENT,           // self_attn40q_kernel<T, 40, 4, 4>: items of 512 queries
  SELF_D40_TWO_BLOCK,            // self_attn40_kernel<T, 40, XCD, 2, 2>
  SELF_D80_PERSISTENT,           // self_attn40q_kernel<T, 80, 2, 4>: items of 256 queries
  SELF_D80,                      // self_attn40_kernel<T, 80, XCD, 1, 2>
  SELF_D160                      // self_attn40_kernel<T, 160, XCD, 1, 1>: one block per CU (104 KB of K / V tiles, ~300 registers)
};

// what self_attn40q_kernel asks of a launch: whole items, a tile count the four-buffer ring divides, a tensor one buffer descriptor spans, two items per CU
inline bool persistent_self_ok(int b, int n, int heads, int d, int item_queries, int n_cu) {
  return n % item_queries == 0 && n % 256 == 0 && n >= 1024 && (int64_t)3 * b * n * heads * d * 2 < ((int64_t)1 << 32) && (int64_t)(n / item_queries) * heads * b >= 2 * n_cu;
}

// d is 40, 80 or 160 (the launcher checks); persist40 / persist80: the switches ETAINV_A40_PERSIST / ETAINV_A80_PERSIST
inline SelfAttnRoute self_attn_route(int b, int n, int heads, int d, int n_cu, bool persist40, bool persist80) {
  if (d == 40) {
    // few blocks (single-image calls: N = 4096, 8 heads, 1 row = 128 blocks of 256 queries on 256 CUs): one 32-query block per wave, twice the blocks
    if (((int64_t)n + 255) / 256 * heads * b <= 256 && n > 128) return SELF_D40_ONE_BLOCK_PER_WAVE;
    // enough (row, head, query block) items for two per CU: the persistent one-wave-per-SIMD kernel
    if (persist40 && persistent_self_ok(b, n, heads, d, 512, n_cu)) return SELF_D40_PERSISTENT;
    // two 32-query blocks per wave, 2 waves per SIMD (one block per wave with 3 / 4 waves per SIMD: +10 % / +52 % time, re-measured in round 6 on the lean staging:
    // profiles/r06_attention_experiments.log)
    return SELF_D40_TWO_BLOCK;
  }
  if (d == 80) return persist80 && persistent_self_ok(b, n, heads, d, 256, n_cu) ? SELF_D80_PERSISTENT : SELF_D80;
  return SELF_D160;
}

}  // namespace etainv
