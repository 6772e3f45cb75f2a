// UNet executor + C ABI of libetainv_hip.so: the model, the workspace, the forward, the attention-map store and the event profiler (the per-op
// entry points etainv_op_* of the parity tests: ops_capi.cpp).
//
// The engine owns: (1) the SD1.x UNet weights, re-laid-out for the kernels (conv [O][tap][I], fused QKV / KV,
// GEGLU row-interleave, one concatenated time-embedding projection), (2) a preallocated NHWC activation
// workspace sized for `max_unet_batch` rows, (3) the attention-map store.  etainv_unet_forward walks the static
// SD1.x graph and only enqueues kernels on the caller's stream: no allocation, no host sync.
// It replaces `self.unet(latent_input, t, encoder_hidden_states=context)["sample"]`
// (reference modules/inversion/eta_inversion.py:321) including what the reference's monkey-patched attention
// forwards do (modules/utils/ptp_utils.py:205-260, modules/utils/masactrl_utils.py:84-127), driven by the
// declarative etainv_attn_ctrl.
#include <cmath>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"
#include "kernels.h"

namespace etainv {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

// ---- profiler
struct ProfRec { int cls; double work, bytes; hipEvent_t a, b; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_prof_pool;
static size_t g_prof_used = 0;
static bool g_prof_paused = false;
bool prof_enabled() { return g_prof_on && !g_prof_paused; }
void prof_pause(bool on) { g_prof_paused = on; }
void prof_begin(int cls, double work, hipStream_t s, double bytes) {
  if (g_prof_used == g_prof_pool.size()) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    g_prof_pool.emplace_back(a, b);
  }
  auto& ev = g_prof_pool[g_prof_used++];
  g_prof.push_back({cls, work, bytes, ev.first, ev.second});
  (void)hipEventRecord(ev.first, s);
}
void prof_end(hipStream_t s) { (void)hipEventRecord(g_prof.back().b, s); }

struct WeightSlot {
  std::string name;
  int64_t shape[4] = {0, 0, 0, 0};
  int ndim = 0;
  void* dst = nullptr;
  int pack = PK_PLAIN;
  int taps = 1;
  int dst_dtype = ETAINV_F32;  // F32 or the compute dtype (-1 placeholder replaced at build)
  float scale = 1.0f;          // constant folded into the values in fp32 before the rounding to the compute dtype
  void** dst4 = nullptr;       // upsampler convs: also packed as four 2x2 phase kernels (launch_pack_ups4) into *dst4
  float* stage = nullptr;      // fp32 copy kept instead of packing at once: the consumer of a folded LayerNorm is packed when gamma / beta are known
  bool set = false;
  int64_t numel() const {
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    return n;
  }
};

struct Norm { float* g = nullptr; float* b = nullptr; };
struct Lin { void* w = nullptr; float* b = nullptr; int n = 0, k = 0; void* w4 = nullptr; };   // w4: phase form [4][n][4][k] of an upsampler conv (launch_pack_ups4)

struct ResBlock {
  int cin = 0, cout = 0;
  Norm n1, n2;
  Lin conv1, conv2, shortcut;  // conv weights [cout][9][cin]
  int tproj_off = 0;           // column offset into the concatenated time-embedding projection
};
struct TBlock {
  int c = 0;
  Norm gn, ln1, ln2, ln3;
  Lin proj_in, qkv, out1, q, kv, out2, ff1, ff2, proj_out;
  // LayerNorm folded into its consumer (norm1 -> fused QKV, norm2 -> attn2.to_q, norm3 -> GEGLU projection): fp32 staging copies of the
  // consumer weights, the row sums s of the packed gamma-scaled operand and c = beta W^T + bias (kernels.h, launch_ln_fold)
  float *st_qkv = nullptr, *st_q = nullptr, *st_ff1 = nullptr;
  float *s_qkv = nullptr, *c_qkv = nullptr, *s_q = nullptr, *c_q = nullptr, *s_ff1 = nullptr, *c_ff1 = nullptr;
  float q_scale = 1.0f;
};

}  // namespace etainv

using namespace etainv;

struct etainv_engine {
  etainv_engine_config cfg{};
  int dt = ETAINV_F16;
  size_t esz = 2;   // bytes per activation / weight element: 2, or 4 in the fp32-operand mode (compute_dtype ETAINV_F32, f32path.hip)
  int L = 64, maxB = 4, max_img = 1;
  static constexpr int kHeads = 8, kCtx = 77, kCtxDim = 768, kGroups = 32, kTemb = 1280, kCh0 = 320;

  std::vector<WeightSlot> slots;
  std::unordered_map<std::string, int> slot_by_name;
  char* warena = nullptr;
  size_t wbytes = 0;
  char* wsarena = nullptr;
  size_t wsbytes = 0;

  // model
  void* conv_in_w = nullptr; float* conv_in_b = nullptr;
  void* conv_out_w = nullptr; float* conv_out_b = nullptr;
  Norm norm_out;
  Lin time1, time2, tproj;  // tproj: concatenated [sum_co][1280]
  int tproj_total = 0;
  std::vector<ResBlock> res;  // execution order: down (8), mid (2), up (12)
  std::vector<TBlock> tb;     // execution order: 16
  Lin down_conv[3], up_conv[3];

  // workspace (2-byte elements unless noted)
  void *skip[12] = {}, *tmp[3] = {}, *gnbuf = nullptr, *h1 = nullptr, *scbuf = nullptr;
  void *hsA = nullptr, *hsB = nullptr, *lnbuf = nullptr, *qkvbuf = nullptr, *attnbuf = nullptr, *qbuf = nullptr, *kvbuf = nullptr,
       *ffbuf = nullptr, *ctxT = nullptr, *tembuf = nullptr, *temb1 = nullptr, *temb2 = nullptr;
  float *tprojbuf = nullptr, *gn_scratch = nullptr, *maps_acc = nullptr, *lnstat = nullptr, *lnfinal = nullptr;
  size_t maps_bytes = 0;
  // which cross layers the store keeps (etainv_maps_configure): map_div 4 = the five (L/4)^2 layers (default; what LocalBlend and the default eta mask
  // read), 2 = the five (L/2)^2 layers (own lazily allocated buffer, 4x the size), 8 = the mid block's (L/8)^2 layer.  maps_cur = the buffer in use
  int map_div = 4, map_layers = 5;
  float *maps_alt = nullptr, *maps_cur = nullptr;
  size_t maps_alt_bytes = 0, maps_cur_bytes = 0;
  // norm1/2/3 of the transformer blocks folded into the GEMMs around them (no LayerNorm pass over HBM); ETAINV_LN_UNFUSED=1 keeps the
  // standalone LayerNorm kernel (A/B switch, read at engine creation)
  // GroupNorm statistics from the epilogue of the GEMM / conv that wrote the tensor (per-channel partials per wave-tile row block, one buffer per
  // activation buffer a GroupNorm can read: skip[0..11], tmp[0..2], h1) instead of a statistics pass over it; ETAINV_GN_UNFUSED=1 keeps the pass
  // cross-attention K / V of the text context per transformer block.  The context does not change over the 50 steps of a loop: with
  // etainv_engine_cache_context(e, 1) a call whose (context pointer, rows, dtype) equal the previous call's reuses them (16 small GEMMs and the
  // context cast per UNet call, 0.6 % of the benchmark step); the caller switches it off when the loop ends.
  void* kvcache[16] = {};
  bool ctx_cache_on = false;
  const void* ctx_cached = nullptr;
  int ctx_rows = 0, ctx_io = -1;
  void* gn_bufs[16] = {};
  float* gn_part[16] = {};
  float* gn_final = nullptr;
  bool gn_fused = true;
  bool ln_fused = true;
  bool ln_folded = false;   // the gamma-scaled consumer weights are packed (redone after any set_weight)
  std::vector<hipStream_t> upload_streams;   // streams weights were uploaded on since the last fold (the fold waits for each that is not the forward's)
  uint64_t ctx_gen = 0, ctx_gen_cached = 0;  // caller's generation of the context buffer (etainv_engine_context_generation)

  // read-only activation taps (etainv_engine_set_tap): one per block of the UNet graph, named by the oracle module whose output it is, in execution
  // order.  A set tap makes the forward copy the block's output to `dst` right after the block; `rows` = the rows that were live there in the last forward
  struct Tap { std::string name; int side = 1, channels = 0; void* dst = nullptr; int rows = 0; };
  std::vector<Tap> taps;
  int tap_index(const std::string& name) const {
    for (size_t i = 0; i < taps.size(); ++i)
      if (taps[i].name == name) return (int)i;
    return -1;
  }
  size_t tap_bytes(const Tap& t, int rows) const { return (size_t)rows * t.side * t.side * t.channels * esz; }

  long long qkv_hm_launches = 0;      // fused QKV projections that wrote the head-major layout since creation
  bool qkv_hm = true;                 // fused QKV projections write head-major planes where the GEMM and the attention kernel both can (ETAINV_QKV_HM)
};

namespace {

struct ArenaPlan {
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

// ---- model construction: registers every diffusers parameter name with its destination and packing
struct Builder {
  etainv_engine* e;
  ArenaPlan plan;
  std::vector<std::function<void(char*)>> fixups;  // resolve offsets -> pointers after allocation

  template <typename P>
  void want(P** field, size_t bytes) {
    size_t off = plan.take(bytes);
    fixups.push_back([field, off](char* base) { *field = reinterpret_cast<P*>(base + off); });
  }
  void add_slot(const std::string& name, std::vector<int64_t> shape, void** dst_field_holder, size_t dst_off_bytes, int pack, int taps,
                int dst_dtype) {
    WeightSlot s;
    s.name = name;
    s.ndim = (int)shape.size();
    for (int i = 0; i < s.ndim; ++i) s.shape[i] = shape[i];
    s.pack = pack;
    s.taps = taps;
    s.dst_dtype = dst_dtype;
    int idx = (int)e->slots.size();
    e->slots.push_back(s);
    e->slot_by_name[name] = idx;
    etainv_engine* eng = e;
    fixups.push_back([eng, idx, dst_field_holder, dst_off_bytes](char*) {
      eng->slots[idx].dst = reinterpret_cast<char*>(*dst_field_holder) + dst_off_bytes;
    });
  }
  // the slot keeps an fp32 copy at *holder + off (elements) instead of being packed by set_weight
  void stage_slot(const std::string& name, float** holder, size_t off) {
    const int idx = e->slot_by_name.at(name);
    etainv_engine* eng = e;
    fixups.push_back([eng, idx, holder, off](char*) { eng->slots[idx].stage = *holder + off; });
  }
  // fp32 vector parameter (bias / norm scale)
  void vec(const std::string& name, float** field, int n) {
    want(field, (size_t)n * 4);
    add_slot(name, {n}, reinterpret_cast<void**>(field), 0, PK_PLAIN, 1, ETAINV_F32);
  }
  void norm(const std::string& prefix, Norm& nm, int c) {
    vec(prefix + ".weight", &nm.g, c);
    vec(prefix + ".bias", &nm.b, c);
  }
  // linear [n][k] in compute dtype (+ optional fp32 bias)
  void linear(const std::string& prefix, Lin& l, int n, int k, bool bias, int pack = PK_PLAIN) {
    l.n = n;
    l.k = k;
    want(&l.w, (size_t)n * k * e->esz);
    add_slot(prefix + ".weight", {n, k}, &l.w, 0, pack, 1, e->dt);
    if (bias) {
      want(&l.b, (size_t)n * 4);
      add_slot(prefix + ".bias", {n}, reinterpret_cast<void**>(&l.b), 0, pack == PK_GEGLU ? PK_GEGLU : PK_PLAIN, 1, ETAINV_F32);
    }
  }
  void conv1x1(const std::string& prefix, Lin& l, int n, int k) {
    l.n = n;
    l.k = k;
    want(&l.w, (size_t)n * k * e->esz);
    add_slot(prefix + ".weight", {n, k, 1, 1}, &l.w, 0, PK_PLAIN, 1, e->dt);
    want(&l.b, (size_t)n * 4);
    add_slot(prefix + ".bias", {n}, reinterpret_cast<void**>(&l.b), 0, PK_PLAIN, 1, ETAINV_F32);
  }
  void conv3x3(const std::string& prefix, Lin& l, int n, int k) {
    l.n = n;
    l.k = k;
    want(&l.w, (size_t)n * k * 9 * e->esz);
    add_slot(prefix + ".weight", {n, k, 3, 3}, &l.w, 0, PK_CONV, 9, e->dt);
    want(&l.b, (size_t)n * 4);
    add_slot(prefix + ".bias", {n}, reinterpret_cast<void**>(&l.b), 0, PK_PLAIN, 1, ETAINV_F32);
  }
  void conv3x3_ups(const std::string& prefix, Lin& l, int n, int k) {   // conv behind a nearest-2x upsample: the 9-tap form + the four 2x2 phase kernels
    conv3x3(prefix, l, n, k);
    if (e->dt != ETAINV_F32) {
      want(&l.w4, (size_t)16 * n * k * e->esz);
      e->slots[e->slot_by_name.at(prefix + ".weight")].dst4 = &l.w4;
    }
  }
  void resblock(const std::string& prefix, int cin, int cout) {
    e->res.emplace_back();
    // NB: pointers into e->res are taken after all blocks exist (vector may grow) -> reserve() up front
    ResBlock& r = e->res.back();
    r.cin = cin;
    r.cout = cout;
    norm(prefix + ".norm1", r.n1, cin);
    conv3x3(prefix + ".conv1", r.conv1, cout, cin);
    r.tproj_off = e->tproj_total;
    // time_emb_proj rows live inside the concatenated projection matrix
    add_slot(prefix + ".time_emb_proj.weight", {cout, etainv_engine::kTemb}, &e->tproj.w,
             (size_t)r.tproj_off * etainv_engine::kTemb * e->esz, PK_PLAIN, 1, e->dt);
    add_slot(prefix + ".time_emb_proj.bias", {cout}, reinterpret_cast<void**>(&e->tproj.b), (size_t)r.tproj_off * 4, PK_PLAIN, 1,
             ETAINV_F32);
    e->tproj_total += cout;
    norm(prefix + ".norm2", r.n2, cout);
    conv3x3(prefix + ".conv2", r.conv2, cout, cout);
    if (cin != cout) conv1x1(prefix + ".conv_shortcut", r.shortcut, cout, cin);
  }
  void tblock(const std::string& prefix, int c) {
    e->tb.emplace_back();
    TBlock& t = e->tb.back();
    t.c = c;
    const std::string tp = prefix + ".transformer_blocks.0";
    norm(prefix + ".norm", t.gn, c);
    conv1x1(prefix + ".proj_in", t.proj_in, c, c);
    norm(tp + ".norm1", t.ln1, c);
    // fused QKV [3c][c]
    t.qkv.n = 3 * c;
    t.qkv.k = c;
    want(&t.qkv.w, (size_t)3 * c * c * e->esz);
    add_slot(tp + ".attn1.to_q.weight", {c, c}, &t.qkv.w, 0, PK_PLAIN, 1, e->dt);
    // head_dim 40 / 80 (the L^2- and (L/2)^2-token levels): softmax scale * log2(e) folded into to_q, so that the self-attention kernel's
    // score accumulator is directly the exponent argument of exp2 (attention.hip, self_attn40_kernel) -- one rounding of W_q * c instead of
    // W_q, none added
    if (self_attn_prescaled_hm_ok(c / etainv_engine::kHeads, e->dt))
      e->slots.back().scale = (1.0f / std::sqrt((float)(c / etainv_engine::kHeads))) * 1.4426950408889634f;
    t.q_scale = e->slots.back().scale;
    add_slot(tp + ".attn1.to_k.weight", {c, c}, &t.qkv.w, (size_t)c * c * e->esz, PK_PLAIN, 1, e->dt);
    add_slot(tp + ".attn1.to_v.weight", {c, c}, &t.qkv.w, (size_t)2 * c * c * e->esz, PK_PLAIN, 1, e->dt);
    linear(tp + ".attn1.to_out.0", t.out1, c, c, true);
    norm(tp + ".norm2", t.ln2, c);
    linear(tp + ".attn2.to_q", t.q, c, c, false);
    t.kv.n = 2 * c;
    t.kv.k = etainv_engine::kCtxDim;
    want(&t.kv.w, (size_t)2 * c * etainv_engine::kCtxDim * e->esz);
    add_slot(tp + ".attn2.to_k.weight", {c, etainv_engine::kCtxDim}, &t.kv.w, 0, PK_PLAIN, 1, e->dt);
    add_slot(tp + ".attn2.to_v.weight", {c, etainv_engine::kCtxDim}, &t.kv.w, (size_t)c * etainv_engine::kCtxDim * e->esz, PK_PLAIN, 1, e->dt);
    linear(tp + ".attn2.to_out.0", t.out2, c, c, true);
    norm(tp + ".norm3", t.ln3, c);
    linear(tp + ".ff.net.0.proj", t.ff1, 8 * c, c, true, PK_GEGLU);
    linear(tp + ".ff.net.2", t.ff2, c, 4 * c, true);
    conv1x1(prefix + ".proj_out", t.proj_out, c, c);
    if (e->ln_fused) {
      const size_t cc = (size_t)c * c;
      want(&t.st_qkv, 3 * cc * 4);
      want(&t.st_q, cc * 4);
      want(&t.st_ff1, 8 * cc * 4);
      stage_slot(tp + ".attn1.to_q.weight", &t.st_qkv, 0);
      stage_slot(tp + ".attn1.to_k.weight", &t.st_qkv, cc);
      stage_slot(tp + ".attn1.to_v.weight", &t.st_qkv, 2 * cc);
      stage_slot(tp + ".attn2.to_q.weight", &t.st_q, 0);
      stage_slot(tp + ".ff.net.0.proj.weight", &t.st_ff1, 0);
      want(&t.s_qkv, (size_t)3 * c * 4);
      want(&t.c_qkv, (size_t)3 * c * 4);
      want(&t.s_q, (size_t)c * 4);
      want(&t.c_q, (size_t)c * 4);
      want(&t.s_ff1, (size_t)8 * c * 4);
      want(&t.c_ff1, (size_t)8 * c * 4);
    }
  }
};

int build_model(etainv_engine* e) {
  Builder b{e};
  e->res.reserve(22);
  e->tb.reserve(16);
  const int ch[4] = {320, 640, 1280, 1280};
  // conv_in / conv_out keep fp32 weights in their own layouts
  b.want(&e->conv_in_w, (size_t)64 * ch[0] * e->esz);   // [320][64] compute dtype: conv_in runs as a K = 64 GEMM on an im2col buffer
  b.add_slot("conv_in.weight", {ch[0], 4, 3, 3}, &e->conv_in_w, 0, PK_CONV_IN_GEMM, 9, e->dt);
  b.vec("conv_in.bias", &e->conv_in_b, ch[0]);
  b.linear("time_embedding.linear_1", e->time1, etainv_engine::kTemb, ch[0], true);
  b.linear("time_embedding.linear_2", e->time2, etainv_engine::kTemb, etainv_engine::kTemb, true);
  // concatenated time-embedding projection: total = sum of cout over the 22 resblocks = 21120... computed below;
  // reserve the maximum up front (22 * 1280) and trim logically via tproj_total
  b.want(&e->tproj.w, (size_t)22 * 1280 * etainv_engine::kTemb * e->esz);
  b.want(&e->tproj.b, (size_t)22 * 1280 * 4);
  // down
  int cin = ch[0];
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) {
      b.resblock("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), j == 0 ? cin : ch[i], ch[i]);
      if (i < 3) b.tblock("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), ch[i]);
    }
    if (i < 3) b.conv3x3("down_blocks." + std::to_string(i) + ".downsamplers.0.conv", e->down_conv[i], ch[i], ch[i]);
    cin = ch[i];
  }
  // mid
  b.resblock("mid_block.resnets.0", 1280, 1280);
  b.tblock("mid_block.attentions.0", 1280);
  b.resblock("mid_block.resnets.1", 1280, 1280);
  // up: rev = (1280,1280,640,320)
  const int rev[4] = {1280, 1280, 640, 320};
  int prev = 1280;
  for (int i = 0; i < 4; ++i) {
    const int cout = rev[i];
    const int cin_skip = rev[std::min(i + 1, 3)];
    for (int j = 0; j < 3; ++j) {
      const int skipc = (j == 2) ? cin_skip : cout;
      const int rin = (j == 0) ? prev : cout;
      b.resblock("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j), rin + skipc, cout);
      if (i > 0) b.tblock("up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), cout);
    }
    if (i < 3) b.conv3x3_ups("up_blocks." + std::to_string(i) + ".upsamplers.0.conv", e->up_conv[i], cout, cout);
    prev = cout;
  }
  b.norm("conv_norm_out", e->norm_out, ch[0]);
  b.want(&e->conv_out_w, (size_t)9 * ch[0] * 4 * e->esz);   // [4][9][320] compute dtype: conv_out is an N = 4 implicit GEMM
  b.add_slot("conv_out.weight", {4, ch[0], 3, 3}, &e->conv_out_w, 0, PK_CONV, 9, e->dt);
  b.vec("conv_out.bias", &e->conv_out_b, 4);
  e->tproj.n = e->tproj_total;
  e->tproj.k = etainv_engine::kTemb;

  e->wbytes = b.plan.off;
  ETAINV_HIP(hipMalloc(reinterpret_cast<void**>(&e->warena), e->wbytes));
  ETAINV_HIP(hipMemset(e->warena, 0, e->wbytes));
  // two passes: first resolve `want` fields (pointers), then slot destinations that depend on them
  for (auto& f : b.fixups) f(e->warena);
  for (auto& f : b.fixups) f(e->warena);
  return 0;
}

// the tap points: every block of the graph build_model registered, under the oracle's module names (oracle/unet.py), in execution order
void build_taps(etainv_engine* e) {
  const int L = e->L;
  const int ch[4] = {320, 640, 1280, 1280};
  auto add = [&](const std::string& name, int side, int c) {
    etainv_engine::Tap t;
    t.name = name;
    t.side = side;
    t.channels = c;
    e->taps.push_back(t);
  };
  add("time_embedding", 1, etainv_engine::kTemb);   // [rows][1280]: the MLP output in front of the in-place SiLU
  add("conv_in", L, ch[0]);
  int side = L;
  for (int i = 0; i < 4; ++i) {
    const std::string b = "down_blocks." + std::to_string(i);
    for (int j = 0; j < 2; ++j) {
      add(b + ".resnets." + std::to_string(j), side, ch[i]);
      if (i < 3) add(b + ".attentions." + std::to_string(j), side, ch[i]);
    }
    if (i < 3) {
      side /= 2;
      add(b + ".downsamplers.0", side, ch[i]);
    }
  }
  add("mid_block.resnets.0", side, 1280);
  add("mid_block.attentions.0", side, 1280);
  add("mid_block.resnets.1", side, 1280);
  const int rev[4] = {1280, 1280, 640, 320};
  for (int i = 0; i < 4; ++i) {
    const std::string b = "up_blocks." + std::to_string(i);
    for (int j = 0; j < 3; ++j) {
      add(b + ".resnets." + std::to_string(j), side, rev[i]);
      if (i > 0) add(b + ".attentions." + std::to_string(j), side, rev[i]);
    }
    if (i < 3) {
      side *= 2;
      add(b + ".upsamplers.0", side, rev[i]);
    }
  }
  add("conv_norm_out", L, ch[0]);                    // GroupNorm + SiLU in gnbuf: what conv_out reads
}

int build_workspace(etainv_engine* e) {
  ArenaPlan plan;
  std::vector<std::function<void(char*)>> fix;
  auto want = [&](void** field, size_t bytes) {
    size_t off = plan.take(bytes);
    fix.push_back([field, off](char* base) { *field = base + off; });
  };
  const size_t B = (size_t)e->maxB, L = (size_t)e->L, esz = e->esz;
  const size_t hw[4] = {L * L, (L / 2) * (L / 2), (L / 4) * (L / 4), (L / 8) * (L / 8)};
  const size_t skip_el[12] = {hw[0] * 320, hw[0] * 320, hw[0] * 320, hw[1] * 320,  hw[1] * 640,  hw[1] * 640,
                              hw[2] * 640, hw[2] * 1280, hw[2] * 1280, hw[3] * 1280, hw[3] * 1280, hw[3] * 1280};
  for (int i = 0; i < 12; ++i) want(&e->skip[i], B * skip_el[i] * esz);
  // largest activation [HW x C] over the levels is L^2 x 320 (x2 after an upsample conv never exceeds it)
  const size_t hmax = hw[0] * 320;
  // block outputs: the up_blocks.2 upsample conv emits L^2 x 640
  for (int i = 0; i < 3; ++i) want(&e->tmp[i], B * hw[0] * 640 * esz);
  want(&e->gnbuf, B * hw[0] * 960 * esz);
  want(&e->h1, B * hmax * esz);
  want(&e->scbuf, B * hmax * esz);
  want(&e->hsA, B * hmax * esz);
  want(&e->hsB, B * hmax * esz);
  want(&e->lnbuf, B * hmax * esz);
  want(&e->qkvbuf, B * hmax * 3 * esz);
  want(&e->attnbuf, B * hmax * esz);
  want(&e->qbuf, B * hmax * esz);
  want(&e->kvbuf, B * 77 * 2 * 1280 * esz);
  for (size_t i = 0; i < e->tb.size() && i < 16; ++i) want(&e->kvcache[i], B * 77 * 2 * (size_t)e->tb[i].c * esz);
  want(&e->ffbuf, B * hmax * 4 * esz);
  want(&e->ctxT, B * 77 * 768 * esz);
  want(&e->tembuf, B * 320 * esz);
  want(&e->temb1, B * 1280 * esz);
  want(&e->temb2, B * 1280 * esz);
  want(reinterpret_cast<void**>(&e->tprojbuf), B * (size_t)e->tproj_total * 4);
  want(reinterpret_cast<void**>(&e->gn_scratch), B * (GN_MAX_CHUNKS + 1) * etainv_engine::kGroups * 2 * 4);
  // LayerNorm partials [M][P][2]: P = C / (wave tile columns) <= C / 32, M * C <= B * hmax on every level
  want(reinterpret_cast<void**>(&e->lnstat), B * hmax / 32 * 2 * 4);
  want(reinterpret_cast<void**>(&e->lnfinal), B * hw[0] * 2 * 4);   // (mean, rstd) per token row
  // GroupNorm partials: [rows / wm][2][C] floats with wm >= 32 rows per block -> elements / 16 floats per tensor
  for (int i = 0; i < 12; ++i) want(reinterpret_cast<void**>(&e->gn_part[i]), B * skip_el[i] / 16 * 4);
  for (int i = 0; i < 3; ++i) want(reinterpret_cast<void**>(&e->gn_part[12 + i]), B * hw[0] * 640 / 16 * 4);
  want(reinterpret_cast<void**>(&e->gn_part[15]), B * hmax / 16 * 4);
  want(reinterpret_cast<void**>(&e->gn_final), B * (etainv_engine::kGroups * 2 + 2 * 2560) * 4);   // (mean, rstd) + scale / shift planes
  const size_t res = L / 4;
  e->maps_bytes = (size_t)5 * e->max_img * 2 * etainv_engine::kHeads * res * res * 77 * 4;
  want(reinterpret_cast<void**>(&e->maps_acc), e->maps_bytes);
  e->wsbytes = plan.off;
  ETAINV_HIP(hipMalloc(reinterpret_cast<void**>(&e->wsarena), e->wsbytes));
  for (auto& f : fix) f(e->wsarena);
  for (int i = 0; i < 12; ++i) e->gn_bufs[i] = e->skip[i];
  for (int i = 0; i < 3; ++i) e->gn_bufs[12 + i] = e->tmp[i];
  e->gn_bufs[15] = e->h1;
  ETAINV_HIP(hipMemset(e->maps_acc, 0, e->maps_bytes));
  e->maps_cur = e->maps_acc;
  e->maps_cur_bytes = e->maps_bytes;
  return 0;
}

// ---- forward helpers
struct Fwd {
  etainv_engine* e;
  hipStream_t s;
  int rows;
  const etainv_attn_ctrl* ctrl;
  int tblock_idx = 0;
  int ctx_rows = 0;        // rows of the context tensor of this call (== n_rows; `rows` shrinks behind a src_exit_block)
  bool kv_reuse = false;   // the K / V projections of this context are already in e->kvcache (etainv_engine_cache_context)

  // rows per GroupNorm partial block of the tensor now in each tracked buffer (0: no partials -- the GroupNorm runs its statistics pass)
  int part_wm[16] = {};
  int part_of(const void* buf) const {
    for (int i = 0; i < 16; ++i)
      if (e->gn_bufs[i] == buf) return i;
    return -1;
  }
  // tap point `name`: `n` rows of `buf` are the block's output (a set tap copies them out; the row count is recorded either way)
  int tap(const std::string& name, const void* buf, int n) {
    const int i = e->tap_index(name);
    if (i < 0) {
      set_error("unknown tap point " + name);
      return 1;
    }
    etainv_engine::Tap& t = e->taps[i];
    t.rows = n;
    if (t.dst) ETAINV_HIP(hipMemcpyAsync(t.dst, buf, e->tap_bytes(t, n), hipMemcpyDeviceToDevice, s));
    return 0;
  }
  // launch + bookkeeping: gn_out asks the epilogue for the GroupNorm partials of p.out (when the launch shape can: launch_igemm reports the rows
  // per block, 0 otherwise)
  int run(IGemmParams p, bool gn_out = false) {
    const int idx = part_of(p.out);
    int wm = 0;
    if (gn_out && e->gn_fused && idx >= 0) {
      p.stat_out = e->gn_part[idx];
      p.stat_kind = 1;
      if (launch_igemm(p, e->dt, s, &wm)) return 1;
    } else if (launch_igemm(p, e->dt, s)) {
      return 1;
    }
    if (idx >= 0) part_wm[idx] = wm;
    return 0;
  }
  // Context-independent prefix (see etainv_unet_forward): a tensor computed for the first `half` batch rows is copied to rows half .. 2 half - 1, together
  // with the GroupNorm partials its producer left (row blocks are batch-row major: the first half is a prefix of the buffer)
  int dup_rows(void* buf, int have, int n, int hw, int c) {   // rows [0, n) -> rows [have, have + n); a batch row holds hw pixels of c channels
    const size_t elems_per_row = (size_t)hw * c;
    const size_t off = (size_t)have * elems_per_row * e->esz, bytes = (size_t)n * elems_per_row * e->esz;
    ETAINV_HIP(hipMemcpyAsync(reinterpret_cast<char*>(buf) + off, buf, bytes, hipMemcpyDeviceToDevice, s));
    const int idx = part_of(buf);
    if (idx >= 0 && part_wm[idx] > 0) {
      if (hw % part_wm[idx] == 0) {   // [rows * hw / wm][2][C]: a batch row owns hw / wm whole row blocks
        const size_t per_row = (size_t)(hw / part_wm[idx]) * 2 * c * sizeof(float);
        ETAINV_HIP(hipMemcpyAsync(reinterpret_cast<char*>(e->gn_part[idx]) + per_row * have, e->gn_part[idx], per_row * n, hipMemcpyDeviceToDevice, s));
      } else {
        part_wm[idx] = 0;             // row blocks straddle batch rows (small L): no per-row slice to copy -- the consumer runs the statistics pass
      }
    }
    return 0;
  }
  int groupnorm(const void* x1, const void* x2, int c1, int c2, const Norm& nm, int hw, float eps, int silu) {
    const int i1 = part_of(x1), i2 = x2 ? part_of(x2) : -1;
    const int w1 = i1 >= 0 ? part_wm[i1] : 0, w2 = i2 >= 0 ? part_wm[i2] : 0;
    if (w1 > 0 && hw % w1 == 0 && (!x2 || (w2 > 0 && hw % w2 == 0)))
      return launch_groupnorm_pre(x1, x2, c1, c2, e->gn_part[i1], w1, x2 ? e->gn_part[i2] : nullptr, w2, nm.g, nm.b, e->gnbuf, rows, hw,
                                  etainv_engine::kGroups, eps, silu, e->gn_final, e->dt, s);
    return launch_groupnorm(x1, x2, c1, c2, nm.g, nm.b, e->gnbuf, rows, hw, etainv_engine::kGroups, eps, silu, e->gn_scratch, e->dt, s);
  }
  // a Linear / 1x1 conv of the model on M rows; what is special to a launch is assigned by name on the result
  static IGemmParams linear(const void* a, const Lin& l, void* out, int M) { return igemm_linear(a, l.w, l.b, out, M, l.n, l.k); }
  // out = l(LayerNorm(x)), x [M][l.k]: the norm folded into the GEMM (s_vec / c_vec of launch_ln_fold, (mean, rstd) per row in e->lnfinal), or
  // the standalone pass through e->lnbuf in front of it
  int ln_consumer(IGemmParams& p, const void* x, const Norm& nm, const float* s_vec, const float* c_vec, const Lin& l, void* out, int M) {
    if (!e->ln_fused) {
      p = linear(e->lnbuf, l, out, M);
      return launch_layernorm(x, nm.g, nm.b, e->lnbuf, M, l.k, 1e-5f, e->dt, s);
    }
    p = linear(x, l, out, M);
    p.bias = c_vec;
    p.ln_stat = e->lnfinal;
    p.ln_s = s_vec;
    return 0;
  }
  // this GEMM writes the input of a LayerNorm: when the norm is folded into its consumer, leave (mean, rstd) of the output rows in e->lnfinal
  // (partials from the epilogue when the launch can, combined by a small pass; else a pass over the output)
  int run_ln_out(IGemmParams p) {
    if (!e->ln_fused) return run(p);
    p.stat_out = e->lnstat;
    int P = 0;
    if (launch_igemm(p, e->dt, s, &P)) return 1;
    if (P == 0) return launch_row_stats(p.out, e->lnfinal, p.M, p.N, 1e-5f, e->dt, s);
    return launch_ln_finalize(e->lnstat, P, p.N / P, 1e-5f, e->lnfinal, p.M, s);
  }
  // conv3x3 of the model over the current rows (side x side pixels each); the time row and the residual are assigned by name on the result
  IGemmParams conv3x3(const void* a, const Lin& l, void* out, int side, int stride, int ups) const {
    IGemmParams p = igemm_conv3x3(a, l.w, l.b, out, rows, side, side, l.k, l.n, stride, ups);
    p.rowvec_stride = e->tproj_total;
    return p;
  }
  int run_conv(const IGemmParams& p, const Lin& l) {
    if (p.ups && l.w4) {   // four 2 x 2 phase convs on the source image instead of nine taps on the upsampled one (4 / 9 of the FLOPs) where the ring can
      IGemmParams q = p;
      q.ups = 2;
      q.taps = 4;
      q.w = l.w4;
      if (igemm_ups4_ok(q, e->dt)) return run(q, true);
    }
    return run(p, true);
  }
  // x = cat[x1 (c1), x2 (c2)] -> out
  // pnp_site: this is up_blocks[1].resnets[1], the one block of the plug-and-play feature injection
  int resblock(const ResBlock& r, const void* x1, const void* x2, int c1, int c2, int side, void* out, bool pnp_site = false) {
    const int hw = side * side;
    if (groupnorm(x1, x2, c1, c2, r.n1, hw, 1e-5f, 1)) return 1;
    IGemmParams cv1 = conv3x3(e->gnbuf, r.conv1, e->h1, side, /*stride=*/1, /*ups=*/0);
    cv1.rowvec = e->tprojbuf + r.tproj_off;
    if (run_conv(cv1, r.conv1)) return 1;
    if (groupnorm(e->h1, nullptr, r.cout, 0, r.n2, hw, 1e-5f, 1)) return 1;
    // plug-and-play: conv2's output of the target rows is that of the u_s row of their image (pnp_utils.py conv_forward) -- conv2 is a function of its
    // input row alone, so the substitution happens on its input; the shortcut / residual term below stays each row's own
    if (pnp_site && ctrl && ctrl->mode == ETAINV_ATTN_PNP && ctrl->pnp_conv_active &&
        launch_rows_broadcast(e->gnbuf, rows, ctrl->n_img, (int64_t)hw * r.cout, e->dt, s)) return 1;
    IGemmParams cv2 = conv3x3(e->gnbuf, r.conv2, out, side, /*stride=*/1, /*ups=*/0);
    cv2.residual = x1;
    if (r.shortcut.w) {
      IGemmParams sc = linear(x1, r.shortcut, e->scbuf, rows * hw);
      if (x2) {
        sc.a2 = x2;
        sc.c1 = c1;
        sc.c2 = c2;
      }
      if (run(sc)) return 1;
      cv2.residual = e->scbuf;
    }
    return run_conv(cv2, r.conv2);
  }
  // self_rows (0 = all): the sublayers in front of the cross-attention (GroupNorm, proj_in, QKV, self-attention, to_out + residual) do not see
  // the text context; when batch rows r and r + self_rows carry the same latent and timestep (the uncond / cond halves of a CFG call) they are
  // computed for the first self_rows rows only and their result (the residual stream entering the cross-attention) is copied to the other half
  int transformer(const TBlock& t, const void* x, int side, void* out, int self_rows = 0) {
    const int hw = side * side, c = t.c, d = c / etainv_engine::kHeads;
    const int blk = tblock_idx++;
    const bool fold = e->ln_fused;
    int mode = 0, n_img = 1;
    if (ctrl) {
      n_img = ctrl->n_img;
      if (ctrl->mode == ETAINV_ATTN_PTP && ctrl->self_replace_active && hw <= ctrl->self_max_tokens) mode = 1;
      if (ctrl->mode == ETAINV_ATTN_MASA && ctrl->masa_active && blk >= ctrl->masa_first_block) mode = 2;
      if (ctrl->mode == ETAINV_ATTN_PNP && ctrl->pnp_qk_active && blk >= 8) mode = 3;   // up_blocks[1].attentions[1] onwards (pnp.py register_pnp)
    }
    const int all_rows = rows;
    if (self_rows <= 0 || self_rows >= all_rows || 2 * self_rows < all_rows || mode != 0) self_rows = all_rows;   // (a row remap couples the halves: no sharing)
    rows = self_rows;
    int M = rows * hw;
    if (groupnorm(x, nullptr, c, 0, t.gn, hw, 1e-6f, 0)) return 1;
    if (run_ln_out(linear(e->gnbuf, t.proj_in, e->hsA, M))) return 1;
    // self-attention
    int head_major = 0;   // the fused QKV projection writes head-major planes when both sides can (section 4.2: a 64-key tile becomes one contiguous block)
    IGemmParams qkv;
    if (ln_consumer(qkv, e->hsA, t.ln1, t.s_qkv, t.c_qkv, t.qkv, e->qkvbuf, M)) return 1;
    if (fold && e->qkv_hm && self_attn_prescaled_hm_ok(d, e->dt)) {
      IGemmParams hm = qkv;
      hm.hm_heads = etainv_engine::kHeads;
      hm.hm_dim = d;
      hm.hm_tokens = hw;
      if (igemm_hm_ok(hm, e->dt)) {
        head_major = 1;
        ++e->qkv_hm_launches;
        qkv = hm;
      }
    }
    if (run(qkv)) return 1;
    if (launch_self_attention_mode(e->qkvbuf, e->attnbuf, rows, hw, etainv_engine::kHeads, d, mode, n_img, e->dt, s, /*q_prescaled=*/self_attn_prescaled_hm_ok(d, e->dt),
                                   ctrl ? (ctrl->src_exit_block ? -1 : ctrl->first_row) : 0, head_major)) return 1;
    IGemmParams o1 = linear(e->attnbuf, t.out1, e->hsB, M);
    o1.residual = e->hsA;
    if (run_ln_out(o1)) return 1;
    if (self_rows != all_rows) {   // the other half of the batch enters the cross-attention with the same residual stream (and LayerNorm statistics)
      const size_t off = (size_t)M * c * e->esz, Mn = (size_t)(all_rows - self_rows) * hw;   // rows [0, all - self) -> rows [self, all)
      ETAINV_HIP(hipMemcpyAsync(reinterpret_cast<char*>(e->hsB) + off, e->hsB, Mn * c * e->esz, hipMemcpyDeviceToDevice, s));
      if (fold) ETAINV_HIP(hipMemcpyAsync(e->lnfinal + (size_t)M * 2, e->lnfinal, Mn * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
      rows = all_rows;
      M = rows * hw;
    }
    // cross-attention
    IGemmParams q;
    if (ln_consumer(q, e->hsB, t.ln2, t.s_q, t.c_q, t.q, e->qbuf, M) || run(q)) return 1;
    void* kvb = e->kvcache[blk];
    // (all rows of the call's context, also behind a src_exit_block: a later call that reuses the cache may exit later)
    if (!kv_reuse && run(linear(e->ctxT, t.kv, kvb, ctx_rows * etainv_engine::kCtx))) return 1;
    CrossParams cp;
    cp.N = hw;
    cp.heads = etainv_engine::kHeads;
    cp.n_ctx = etainv_engine::kCtx;
    cp.scale_log2 = (1.0f / std::sqrt((float)d)) * 1.4426950408889634f;
    cp.rows = rows;
    cp.n_img_cap = e->max_img;
    cp.maps_acc = e->maps_cur;
    cross_params_from_ctrl(cp, ctrl);
    if (cp.layout) {
      const int res = e->L / e->map_div;
      if (ctrl->store_maps && hw == res * res) {
        // the five (L/4)^2-token cross layers: transformer blocks 4,5 (down) and 7,8,9 (up); (L/2)^2: 2,3 and 10,11,12; (L/8)^2: the mid block 6
        static const int layer_of_block[3][16] = {{-1, -1, 0, 1, -1, -1, -1, -1, -1, -1, 2, 3, 4, -1, -1, -1},
                                                  {-1, -1, -1, -1, 0, 1, -1, 2, 3, 4, -1, -1, -1, -1, -1, -1},
                                                  {-1, -1, -1, -1, -1, -1, 0, -1, -1, -1, -1, -1, -1, -1, -1, -1}};
        cp.map_layer = layer_of_block[e->map_div == 2 ? 0 : e->map_div == 4 ? 1 : 2][blk];
      }
    }
    if (launch_cross_attention_p(e->qbuf, kvb, e->attnbuf, rows, d, cp, e->dt, s)) return 1;
    IGemmParams o2 = linear(e->attnbuf, t.out2, e->hsA, M);
    o2.residual = e->hsB;
    if (run_ln_out(o2)) return 1;
    // feed-forward (GEGLU)
    IGemmParams ff1;
    if (ln_consumer(ff1, e->hsA, t.ln3, t.s_ff1, t.c_ff1, t.ff1, e->ffbuf, M)) return 1;
    ff1.geglu = 1;
    if (run(ff1)) return 1;
    IGemmParams ff2 = linear(e->ffbuf, t.ff2, e->hsB, M);
    ff2.residual = e->hsA;
    if (run(ff2)) return 1;
    IGemmParams po = linear(e->hsB, t.proj_out, out, M);
    po.residual = x;
    return run(po, /*gn_out=*/true);
  }
};

void* pick_tmp(etainv_engine* e, const void* a, const void* b) {
  for (int i = 0; i < 3; ++i)
    if (e->tmp[i] != a && e->tmp[i] != b) return e->tmp[i];
  return nullptr;
}

}  // namespace

// =============================================================================================== C ABI
extern "C" int etainv_abi_version(void) { return ETAINV_ABI_VERSION; }
extern "C" const char* etainv_last_error(void) { return g_err.c_str(); }

extern "C" int etainv_engine_create(const etainv_engine_config* cfg, etainv_engine_t** out) {
  ETAINV_CHECK(cfg && out, "null argument");
  ETAINV_CHECK(cfg->compute_dtype == ETAINV_F16 || cfg->compute_dtype == ETAINV_BF16 || cfg->compute_dtype == ETAINV_F32, "compute_dtype must be f16, bf16 or f32");
  ETAINV_CHECK(cfg->latent_size >= 8 && cfg->latent_size % 8 == 0 && cfg->latent_size <= 128, "latent_size must be a multiple of 8 in [8,128]");
  ETAINV_CHECK(cfg->max_unet_batch >= 1 && cfg->max_img >= 1, "batch sizes must be positive");
  int ndev = 0;
  ETAINV_HIP(hipGetDeviceCount(&ndev));
  ETAINV_CHECK(ndev > 0, "no HIP device visible: the etainv engine has no CPU fallback");
  auto* e = new etainv_engine();
  e->cfg = *cfg;
  e->dt = cfg->compute_dtype;
  e->L = cfg->latent_size;
  e->maxB = cfg->max_unet_batch;
  e->max_img = cfg->max_img;
  e->esz = e->dt == ETAINV_F32 ? 4 : 2;
  // fp32-operand mode: the standalone norms (the folds are fusions of the 16-bit kernels' epilogues)
  e->ln_fused = !env_on("ETAINV_LN_UNFUSED") && e->dt != ETAINV_F32;
  e->gn_fused = !env_on("ETAINV_GN_UNFUSED") && e->dt != ETAINV_F32;
  e->qkv_hm = env_flag("ETAINV_QKV_HM", true);   // (default on: +0.8 % on the benchmark step, +1 % on config 5; "0" = row-major)
  build_taps(e);
  if (build_model(e) || build_workspace(e)) {
    etainv_engine_destroy(e);
    return 1;
  }
  *out = e;
  return 0;
}

extern "C" int etainv_engine_destroy(etainv_engine_t* e) {
  if (!e) return 0;
  if (e->warena) (void)hipFree(e->warena);
  if (e->maps_alt) (void)hipFree(e->maps_alt);
  if (e->wsarena) (void)hipFree(e->wsarena);
  delete e;
  return 0;
}

extern "C" int etainv_engine_num_weights(etainv_engine_t* e) { return e ? (int)e->slots.size() : 0; }

extern "C" int etainv_engine_weight_info(etainv_engine_t* e, int i, char* name, int name_cap, int64_t shape[4], int* ndim) {
  ETAINV_CHECK(e && i >= 0 && i < (int)e->slots.size() && name && shape && ndim, "bad arguments");
  const WeightSlot& s = e->slots[i];
  ETAINV_CHECK((int)s.name.size() + 1 <= name_cap, "name buffer too small");
  std::memcpy(name, s.name.c_str(), s.name.size() + 1);
  for (int k = 0; k < 4; ++k) shape[k] = s.shape[k];
  *ndim = s.ndim;
  return 0;
}

extern "C" int etainv_engine_set_weight(etainv_engine_t* e, const char* name, const float* data, int64_t numel, void* stream) {
  ETAINV_CHECK(e && name && data, "null argument");
  auto it = e->slot_by_name.find(name);
  ETAINV_CHECK(it != e->slot_by_name.end(), std::string("unknown parameter ") + name);
  WeightSlot& s = e->slots[it->second];
  ETAINV_CHECK(numel == s.numel(), std::string("size mismatch for ") + name);
  int64_t rows = s.shape[0], cols = s.numel() / s.shape[0];
  if (s.ndim == 1) { rows = s.shape[0]; cols = 1; }
  if (s.stage) {   // a staged slot is copied (fold_layernorms packs it), any other is packed
    ETAINV_HIP(hipMemcpyAsync(s.stage, data, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  } else if (launch_pack_weight(data, s.dst, rows, cols, s.pack, s.taps, s.dst_dtype, (hipStream_t)stream, s.scale)) {
    return 1;
  }
  if (s.dst4 && launch_pack_ups4(data, *s.dst4, (int)s.shape[0], (int)s.shape[1], s.dst_dtype, (hipStream_t)stream)) return 1;
  s.set = true;
  e->ln_folded = false;
  bool seen = false;
  for (hipStream_t u : e->upload_streams) seen = seen || u == (hipStream_t)stream;
  if (!seen) e->upload_streams.push_back((hipStream_t)stream);
  return 0;
}

// gamma / beta of norm1/2/3 folded into the staged consumer weights of every transformer block (launch_ln_fold); runs on the forward's stream
// before the first UNet call after the weights changed
static int fold_layernorms(etainv_engine* e, hipStream_t s) {
  for (hipStream_t u : e->upload_streams)
    if (u != s) ETAINV_HIP(hipStreamSynchronize(u));
  e->upload_streams.clear();
  for (const TBlock& t : e->tb) {
    const int64_t c = t.c, cc = c * c;
    for (int part = 0; part < 3; ++part)
      if (launch_ln_fold(t.st_qkv + part * cc, t.ln1.g, t.ln1.b, nullptr, c, c, PK_PLAIN, part == 0 ? t.q_scale : 1.0f,
                         reinterpret_cast<char*>(t.qkv.w) + (size_t)part * cc * 2, t.s_qkv + part * c, t.c_qkv + part * c, e->dt, s))
        return 1;
    if (launch_ln_fold(t.st_q, t.ln2.g, t.ln2.b, nullptr, c, c, PK_PLAIN, 1.0f, t.q.w, t.s_q, t.c_q, e->dt, s)) return 1;
    if (launch_ln_fold(t.st_ff1, t.ln3.g, t.ln3.b, t.ff1.b, 8 * c, c, PK_GEGLU, 1.0f, t.ff1.w, t.s_ff1, t.c_ff1, e->dt, s)) return 1;
  }
  e->ln_folded = true;
  return 0;
}

extern "C" int etainv_engine_weights_ready(etainv_engine_t* e) {
  if (!e) return 0;
  for (auto& s : e->slots)
    if (!s.set) return 0;
  return 1;
}

extern "C" int etainv_engine_cache_context(etainv_engine_t* e, int enable) {
  ETAINV_CHECK(e, "null engine");
  e->ctx_cache_on = enable != 0;
  e->ctx_cached = nullptr;   // (the first call after switching it on computes the projections)
  return 0;
}

extern "C" int etainv_engine_context_generation(etainv_engine_t* e, uint64_t generation) {
  ETAINV_CHECK(e, "null engine");
  e->ctx_gen = generation;
  return 0;
}

extern "C" int64_t etainv_engine_workspace_bytes(etainv_engine_t* e) { return e ? (int64_t)e->wsbytes : 0; }
extern "C" int64_t etainv_engine_weight_bytes(etainv_engine_t* e) { return e ? (int64_t)e->wbytes : 0; }

/* fused QKV projections that wrote the head-major planes since the engine was created (tests: the layout is really on the path) */
extern "C" int etainv_engine_qkv_head_major_count(etainv_engine_t* e, long long* launches) {
  ETAINV_CHECK(e && launches, "bad arguments");
  *launches = e->qkv_hm_launches;
  return 0;
}

extern "C" int etainv_engine_tap_count(etainv_engine_t* e) { return e ? (int)e->taps.size() : 0; }

extern "C" int etainv_engine_tap_info(etainv_engine_t* e, int point, char* name, int name_cap, int* side, int* channels) {
  ETAINV_CHECK(e && point >= 0 && point < (int)e->taps.size() && name && side && channels, "bad arguments");
  const etainv_engine::Tap& t = e->taps[point];
  ETAINV_CHECK((int)t.name.size() + 1 <= name_cap, "name buffer too small");
  std::memcpy(name, t.name.c_str(), t.name.size() + 1);
  *side = t.side;
  *channels = t.channels;
  return 0;
}

extern "C" int etainv_engine_set_tap(etainv_engine_t* e, int point, void* dst, int64_t capacity_bytes) {
  ETAINV_CHECK(e && point >= 0 && point < (int)e->taps.size(), "bad arguments");
  etainv_engine::Tap& t = e->taps[point];
  // (every forward of this engine fits: no call can find the buffer too small after it has enqueued work)
  ETAINV_CHECK(!dst || capacity_bytes >= (int64_t)e->tap_bytes(t, e->maxB), "tap buffer smaller than max_unet_batch rows of " + t.name);
  t.dst = dst;
  return 0;
}

extern "C" int etainv_engine_tap_rows(etainv_engine_t* e, int point) {
  if (!e || point < 0 || point >= (int)e->taps.size()) return -1;
  return e->taps[point].rows;
}

extern "C" int etainv_unet_forward(etainv_engine_t* e, const void* latent, int n_lat, const int64_t* t_host, const void* ctx, int n_rows,
                                   const etainv_attn_ctrl* ctrl, void* out, int io_dtype, void* stream) {
  ETAINV_CHECK(e && latent && t_host && ctx && out, "null argument");
  ETAINV_CHECK(n_rows >= 1 && n_rows <= e->maxB, "n_rows exceeds max_unet_batch");
  ETAINV_CHECK(n_lat >= 1 && n_lat <= n_rows, "1 <= n_lat <= n_rows (UNet row r reads latent r % n_lat)");
  ETAINV_CHECK(etainv_engine_weights_ready(e), "weights not fully set");
  if (ctrl) {
    ETAINV_CHECK(ctrl->n_img >= 1 && ctrl->n_img <= e->max_img, "ctrl.n_img exceeds max_img");
    ETAINV_CHECK(ctrl->first_row == 0 || (ctrl->mode == ETAINV_ATTN_PTP && ctrl->first_row == ctrl->n_img), "first_row: 0, or n_img with prompt-to-prompt");
    // (the self-replace reaches up to the (L/2)^2-token layers: transformer blocks <= 12 -- an exit in front of that would starve it)
    ETAINV_CHECK(ctrl->src_exit_block == 0 || (ctrl->mode == ETAINV_ATTN_PTP && ctrl->first_row == ctrl->n_img && !ctrl->mapper && !ctrl->replace_mat &&
                                               ctrl->src_exit_block >= (ctrl->self_replace_active ? 12 : 9) && ctrl->src_exit_block < 15),
                 "src_exit_block: prompt-to-prompt three-row call without cross edit; exit after block 9..14 (12..14 while the self-replace is active)");
    // the store may keep other layers than the (L/4)^2 ones (etainv_maps_configure): an exit in front of the last stored block would silently drop the
    // source rows' maps of the later layers (last stored block: res_div 2 -> 12, 4 -> 9, 8 -> 6)
    ETAINV_CHECK(!ctrl->src_exit_block || !ctrl->store_maps || (e->map_div == 2 ? 12 : e->map_div == 4 ? 9 : 6) <= ctrl->src_exit_block,
                 "src_exit_block lies in front of the last cross-attention layer the map store keeps (etainv_maps_configure): the source rows' maps would be lost");
    if (ctrl->mode == ETAINV_ATTN_PTP || ctrl->mode == ETAINV_ATTN_MASA)
      ETAINV_CHECK(n_rows == 4 * ctrl->n_img - ctrl->first_row, "ptp / masactrl need 4*n_img UNet rows [u_s,u_t,c_s,c_t] (ptp with first_row = n_img: 3*n_img rows [u_t,c_s,c_t])");
    if (ctrl->mode == ETAINV_ATTN_STORE)
      ETAINV_CHECK(n_rows == 2 * ctrl->n_img || n_rows == ctrl->n_img, "store mode needs n_img or 2*n_img rows");
    if (ctrl->mode == ETAINV_ATTN_PNP)
      ETAINV_CHECK(n_rows == 3 * ctrl->n_img && n_lat == n_rows && !ctrl->store_maps && !ctrl->mapper && !ctrl->alphas && !ctrl->replace_mat && !ctrl->equalizer &&
                       !ctrl->cross_alpha && ctrl->first_row == 0 && ctrl->src_exit_block == 0,
                   "plug-and-play needs 3*n_img UNet rows [u_s,u_t,c_t] over as many latents [src,tgt,tgt], no map store, no tables, first_row == src_exit_block == 0");
  }
  hipStream_t s = (hipStream_t)stream;
  const int L = e->L;
  if (e->ln_fused && !e->ln_folded && fold_layernorms(e, s)) return 1;
  Fwd f{e, s, n_rows, ctrl};
  f.ctx_rows = n_rows;
  for (auto& t : e->taps) t.rows = 0;

  // timesteps (by value in the kernel arguments: no host buffer outlives this call) -> embedding, MLP, all 22 projections in one GEMM
  if (launch_time_embedding(t_host, n_rows, etainv_engine::kCh0, e->tembuf, e->dt, s)) return 1;
  if (f.run(Fwd::linear(e->tembuf, e->time1, e->temb1, n_rows))) return 1;
  if (launch_silu(e->temb1, e->temb1, (int64_t)n_rows * etainv_engine::kTemb, e->dt, s)) return 1;
  if (f.run(Fwd::linear(e->temb1, e->time2, e->temb2, n_rows))) return 1;
  if (f.tap("time_embedding", e->temb2, n_rows)) return 1;
  if (launch_silu(e->temb2, e->temb2, (int64_t)n_rows * etainv_engine::kTemb, e->dt, s)) return 1;
  {
    IGemmParams p = Fwd::linear(e->temb2, e->tproj, e->tprojbuf, n_rows);
    p.out_f32 = 1;
    if (launch_igemm(p, e->dt, s)) return 1;
  }
  f.kv_reuse = e->ctx_cache_on && e->ctx_cached == ctx && e->ctx_rows == n_rows && e->ctx_io == io_dtype && e->ctx_gen_cached == e->ctx_gen;
  // the cache entry becomes valid only when this forward has enqueued every projection (set at the end of this function): an error half-way
  // leaves it invalid, so the next call projects again
  e->ctx_cached = nullptr;
  if (!f.kv_reuse && launch_cast_f32(ctx, io_dtype, e->ctxT, e->dt, (int64_t)n_rows * etainv_engine::kCtx * etainv_engine::kCtxDim, s)) return 1;

  // ---- down path
  // Context-independent prefix: with classifier-free guidance the call carries every latent twice (rows r and r + n_lat: uncond / cond context,
  // same latent, same timestep).  Nothing in front of the first cross-attention reads the context -- conv_in, the first residual block and the first
  // transformer block's GroupNorm / proj_in / QKV / self-attention (N = L^2: the most expensive launch of the call) / to_out -- so those run on
  // n_lat rows and their results are copied to the other half (3 device copies, ~0.3 ms, for 2.6 % of a 128-row call).  The reference evaluates
  // both halves (eta_inversion.py:320-321 `torch.cat([latent] * 2)`); the values are the same.  ETAINV_NO_PREFIX_SHARE=1: A/B switch.
  // (general form: n_lat < n_rows <= 2 n_lat -- rows r >= n_lat repeat latent r - n_lat; the 3 n_img-row backward calls of eta == 0 steps carry
  // latents [tgt, src] and rows [u_t, c_s, c_t]: the last n_img rows repeat the first n_img)
  bool share = !env_on("ETAINV_NO_PREFIX_SHARE") && n_rows > n_lat && n_rows <= 2 * n_lat;
  for (int r = n_lat; share && r < n_rows; ++r) share = t_host[r] == t_host[r - n_lat];
  const int dup_n = n_rows - n_lat;   // rows copied from the head of every shared tensor to its tail
  const int pre_rows = share ? n_lat : n_rows;
  f.rows = pre_rows;
  if (launch_im2col_in(latent, io_dtype, n_lat, pre_rows, L, e->gnbuf, e->dt, s)) return 1;
  if (f.run(igemm_linear(e->gnbuf, e->conv_in_w, e->conv_in_b, e->skip[0], pre_rows * L * L, etainv_engine::kCh0, 64), /*gn_out=*/true)) return 1;
  const int ch[4] = {320, 640, 1280, 1280};
  int ri = 0, ti = 0, si = 1, side = L;
  const void* h = e->skip[0];
  int hc = 320;
  for (int i = 0; i < 4; ++i) {
    const std::string blk = "down_blocks." + std::to_string(i);
    for (int j = 0; j < 2; ++j) {
      const std::string rname = blk + ".resnets." + std::to_string(j);
      if (i < 3) {
        void* r_out = pick_tmp(e, h, nullptr);
        if (f.resblock(e->res[ri++], h, nullptr, hc, 0, side, r_out)) return 1;
        const bool first = i == 0 && j == 0;
        if (first && share) {   // skip[0] (a skip connection of the up path) and the block input (proj_out's residual) are needed for all rows
          if (f.dup_rows(e->skip[0], pre_rows, dup_n, L * L, etainv_engine::kCh0) || f.dup_rows(r_out, pre_rows, dup_n, L * L, ch[0])) return 1;
        }
        f.rows = n_rows;
        // (behind dup_rows: the taps of a shared prefix hold all rows)
        if ((first && f.tap("conv_in", e->skip[0], n_rows)) || f.tap(rname, r_out, n_rows)) return 1;
        if (f.transformer(e->tb[ti++], r_out, side, e->skip[si], first && share ? pre_rows : 0)) return 1;
        if (f.tap(blk + ".attentions." + std::to_string(j), e->skip[si], f.rows)) return 1;
      } else {
        if (f.resblock(e->res[ri++], h, nullptr, hc, 0, side, e->skip[si])) return 1;
        if (f.tap(rname, e->skip[si], f.rows)) return 1;
      }
      h = e->skip[si++];
      hc = ch[i];
    }
    if (i < 3) {
      if (f.run_conv(f.conv3x3(h, e->down_conv[i], e->skip[si], side, /*stride=*/2, /*ups=*/0), e->down_conv[i])) return 1;
      h = e->skip[si++];
      side /= 2;
      if (f.tap(blk + ".downsamplers.0", h, f.rows)) return 1;
    }
  }
  // ---- mid
  {
    void* a = pick_tmp(e, h, nullptr);
    if (f.resblock(e->res[ri++], h, nullptr, 1280, 0, side, a) || f.tap("mid_block.resnets.0", a, f.rows)) return 1;
    void* b2 = pick_tmp(e, a, nullptr);
    if (f.transformer(e->tb[ti++], a, side, b2) || f.tap("mid_block.attentions.0", b2, f.rows)) return 1;
    void* c = pick_tmp(e, b2, nullptr);
    if (f.resblock(e->res[ri++], b2, nullptr, 1280, 0, side, c) || f.tap("mid_block.resnets.1", c, f.rows)) return 1;
    h = c;
    hc = 1280;
  }
  // ---- up path
  const int rev[4] = {1280, 1280, 640, 320};
  const int skip_c[12] = {320, 320, 320, 320, 640, 640, 640, 1280, 1280, 1280, 1280, 1280};
  int sp = 11;
  for (int i = 0; i < 4; ++i) {
    const int cout = rev[i];
    const std::string blk = "up_blocks." + std::to_string(i);
    for (int j = 0; j < 3; ++j) {
      const void* sk = e->skip[sp];
      const int skc = skip_c[sp];
      --sp;
      void* r_out = pick_tmp(e, h, nullptr);
      if (f.resblock(e->res[ri++], h, sk, hc, skc, side, r_out, /*pnp_site=*/i == 1 && j == 1)) return 1;
      if (f.tap(blk + ".resnets." + std::to_string(j), r_out, f.rows)) return 1;
      h = r_out;
      hc = cout;
      if (i > 0) {
        void* t_out = pick_tmp(e, h, nullptr);
        if (f.transformer(e->tb[ti++], h, side, t_out)) return 1;
        if (f.tap(blk + ".attentions." + std::to_string(j), t_out, f.rows)) return 1;   // (all rows: an exit takes effect behind this block)
        h = t_out;
        // the cond source rows (last n_img of [u_t, c_t, c_s]) have fed their last stored attention layer: everything after runs on the other rows
        if (ctrl && ctrl->src_exit_block && ti == ctrl->src_exit_block + 1) f.rows = 2 * ctrl->n_img;
      }
    }
    if (i < 3) {
      void* u = pick_tmp(e, h, nullptr);
      if (f.run_conv(f.conv3x3(h, e->up_conv[i], u, side, /*stride=*/1, /*ups=*/1), e->up_conv[i])) return 1;
      h = u;
      side *= 2;
      if (f.tap(blk + ".upsamplers.0", u, f.rows)) return 1;
    }
  }
  // ---- out
  if (f.groupnorm(h, nullptr, 320, 0, e->norm_out, L * L, 1e-5f, 1)) return 1;
  if (f.tap("conv_norm_out", e->gnbuf, f.rows)) return 1;
  IGemmParams p = igemm_conv3x3(e->gnbuf, e->conv_out_w, e->conv_out_b, out, f.rows, L, L, 320, 4, /*stride=*/1, /*ups=*/0);
  p.out_nchw = 4;
  p.out_io_dtype = io_dtype;
  if (launch_igemm(p, e->dt, s)) return 1;
  if (e->ctx_cache_on) {
    e->ctx_cached = ctx;
    e->ctx_rows = n_rows;
    e->ctx_io = io_dtype;
    e->ctx_gen_cached = e->ctx_gen;
  }
  return 0;
}

extern "C" int etainv_maps_reset(etainv_engine_t* e, void* stream) {
  ETAINV_CHECK(e, "null engine");
  ETAINV_HIP(hipMemsetAsync(e->maps_cur, 0, e->maps_cur_bytes, (hipStream_t)stream));
  return 0;
}

extern "C" int etainv_maps_configure(etainv_engine_t* e, int res_div, void* stream) {
  ETAINV_CHECK(e, "null engine");
  ETAINV_CHECK(res_div == 2 || res_div == 4 || res_div == 8, "res_div must be 2, 4 or 8 (the (L/2)^2, (L/4)^2 cross layers or the mid block's (L/8)^2 layer)");
  ETAINV_CHECK(e->L % res_div == 0, "latent size not divisible by res_div");
  const int layers = res_div == 8 ? 1 : 5;
  const size_t res = e->L / res_div;
  const size_t bytes = (size_t)layers * e->max_img * 2 * etainv_engine::kHeads * res * res * 77 * 4;
  if (bytes <= e->maps_bytes) {
    e->maps_cur = e->maps_acc;
  } else {
    if (bytes > e->maps_alt_bytes) {   // first use of the (L/2)^2 store: its own allocation (host work, outside any capture)
      ETAINV_HIP(hipStreamSynchronize((hipStream_t)stream));
      e->maps_cur = e->maps_acc;           // (a failure below leaves the engine on its default store, never on a freed one)
      e->maps_cur_bytes = e->maps_bytes;
      e->map_div = 4;
      e->map_layers = 5;
      float* old = e->maps_alt;
      e->maps_alt = nullptr;
      e->maps_alt_bytes = 0;
      if (old) ETAINV_HIP(hipFree(old));
      ETAINV_HIP(hipMalloc(reinterpret_cast<void**>(&e->maps_alt), bytes));
      e->maps_alt_bytes = bytes;
    }
    e->maps_cur = e->maps_alt;
  }
  e->maps_cur_bytes = bytes;
  e->map_div = res_div;
  e->map_layers = layers;
  ETAINV_HIP(hipMemsetAsync(e->maps_cur, 0, e->maps_cur_bytes, (hipStream_t)stream));
  return 0;
}

extern "C" int etainv_maps_word_maps_ex(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done, int row_sel, unsigned layer_mask,
                                        float* out, int accumulate, float scale, void* stream) {
  ETAINV_CHECK(e && n_img >= 1 && n_img <= e->max_img && (row_sel == 0 || row_sel == 1), "bad arguments");
  ETAINV_CHECK((layer_mask & ((1u << e->map_layers) - 1u)) != 0, "layer_mask selects none of the stored layers");
  return launch_word_maps(e->maps_cur, e->map_layers, e->max_img, 2, row_sel, etainv_engine::kHeads, e->L / e->map_div, e->L, n_img, tokens, n_tok,
                          steps_done, out, accumulate, scale, (hipStream_t)stream, layer_mask);
}

extern "C" int etainv_maps_word_maps(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done, float* out,
                                     int accumulate, float scale, void* stream) {
  ETAINV_CHECK(e && n_img >= 1 && n_img <= e->max_img, "bad arguments");
  return etainv_maps_word_maps_ex(e, n_img, tokens, n_tok, steps_done, /*row_sel=*/0, /*layer_mask=*/~0u, out, accumulate, scale, stream);
}

extern "C" int etainv_maps_word_maps_role(etainv_engine_t* e, int n_img, const int32_t* tokens, int n_tok, int steps_done, int row_sel,
                                          float* out, int accumulate, float scale, void* stream) {
  ETAINV_CHECK(e && n_img >= 1 && n_img <= e->max_img && (row_sel == 0 || row_sel == 1), "bad arguments");
  return etainv_maps_word_maps_ex(e, n_img, tokens, n_tok, steps_done, row_sel, /*layer_mask=*/~0u, out, accumulate, scale, stream);
}

extern "C" int etainv_local_blend(etainv_engine_t* e, float* x, int n_img, const float* blend_alpha, float thres, void* stream) {
  ETAINV_CHECK(e && n_img >= 1 && n_img <= e->max_img, "bad arguments");
  ETAINV_CHECK(e->map_div == 4, "LocalBlend reads the five (L/4)^2 cross layers (ptp.py:37-39): etainv_maps_configure(e, 4, ...) first");
  return launch_local_blend(e->maps_acc, 5, e->max_img, etainv_engine::kHeads, e->L / 4, e->L, x, n_img, blend_alpha, thres,
                            (hipStream_t)stream);
}

extern "C" int etainv_prof_enable(int on) {
  g_prof_on = on != 0;
  return 0;
}
extern "C" int etainv_prof_reset(void) {
  g_prof.clear();
  g_prof_used = 0;
  return 0;
}
// fn(record, event-timed ms) for every launch of one kernel class since the last reset, in launch order.  Synchronises the device (the readers below
// are diagnostic calls, never used inside the loops).
template <typename F>
static int prof_visit(int cls, F fn) {
  ETAINV_HIP(hipDeviceSynchronize());
  for (const ProfRec& r : g_prof)
    if (r.cls == cls) {
      float ms = 0.f;
      ETAINV_HIP(hipEventElapsedTime(&ms, r.a, r.b));
      fn(r, ms);
    }
  return 0;
}
/* Sum of the durations (ms), work (FLOPs or bytes) and launch count of one kernel class. */
extern "C" int etainv_prof_read(int cls, double* ms, double* work, int64_t* launches) {
  ETAINV_CHECK(cls >= 0 && cls < PROF_NCLASS && ms && work && launches, "bad arguments");
  *ms = *work = 0.0;
  *launches = 0;
  return prof_visit(cls, [&](const ProfRec& r, float t) {
    *ms += t;
    *work += r.work;
    ++*launches;
  });
}
// the first `cap` launches of one class, one entry each (bytes: optional); *launches = how many there were
static int prof_records(int cls, double* ms, double* work, double* bytes, int64_t cap, int64_t* launches) {
  *launches = 0;
  return prof_visit(cls, [&](const ProfRec& r, float t) {
    const int64_t n = (*launches)++;
    if (n >= cap) return;
    ms[n] = t;
    work[n] = r.work;
    if (bytes) bytes[n] = r.bytes;
  });
}
extern "C" int etainv_prof_records(int cls, double* ms, double* work, int64_t cap, int64_t* launches) {
  ETAINV_CHECK(cls >= 0 && cls < PROF_NCLASS && ms && work && launches && cap >= 0, "bad arguments");
  return prof_records(cls, ms, work, nullptr, cap, launches);
}
/* etainv_prof_records + the algorithmic HBM bytes of every launch (0 for classes that record none): joins a per-launch PMC traffic pass
 * (tools/pmc_per_launch.py) with what each launch had to move at minimum */
extern "C" int etainv_prof_records_ex(int cls, double* ms, double* work, double* bytes, int64_t cap, int64_t* launches) {
  ETAINV_CHECK(cls >= 0 && cls < PROF_NCLASS && ms && work && bytes && launches && cap >= 0, "bad arguments");
  return prof_records(cls, ms, work, bytes, cap, launches);
}
/* Roofline split of one class: launches whose arithmetic intensity work / bytes is at least `ridge` (FLOP per byte; MFMA peak / HBM peak) are
 * MFMA-bound, the rest HBM-bound.  out[0..2] = ms, FLOPs, bytes of the MFMA-bound launches; out[3..5] = the same of the HBM-bound ones. */
extern "C" int etainv_prof_split(int cls, double ridge, double* out6, int64_t* launches2) {
  ETAINV_CHECK(cls >= 0 && cls < PROF_NCLASS && out6 && launches2, "bad arguments");
  for (int k = 0; k < 6; ++k) out6[k] = 0.0;
  launches2[0] = launches2[1] = 0;
  return prof_visit(cls, [&](const ProfRec& r, float t) {
    if (r.bytes <= 0.0) return;
    const int o = (r.work / r.bytes >= ridge) ? 0 : 3;
    out6[o] += t;
    out6[o + 1] += r.work;
    out6[o + 2] += r.bytes;
    ++launches2[o / 3];
  });
}
