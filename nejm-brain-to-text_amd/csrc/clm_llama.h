// clm_llama.h — the Llama-family forward (causal_lm_llama.hip's header has the contract and the kernel sequence), written once
// for both element types and for every family that rides on it: the embed and RMSNorm kernels, llama_forward, the Llama family
// and the defaults of the families that derive it, and the statements the families' descriptor checks share.  The bodies of the
// entry points, the size rules and the family contract are clm_internal.h's, for every family.
//
// What a forward of this header asks of its policy P beside P::E:
//   P::gemm_rope, gemm_swiglu, gemm_resid, gemm_head (g, s)   the four GEMMs, each through the one tile rule launch_gemm
//   P::embed, P::rmsnorm                        the launches of the two kernels below
//   P::attn, P::attn_tree                       the flat and the tree attention launcher
//   P::qk_norm                                  whether the QKV GEMM's epilogue norms the q and k heads (Qwen3): llama_forward then
//                                               hands it the layer's weights from the b2t_clm_qknorm_t array and rms_eps
// The Llama policy is LlamaShared<E> (below; causal_lm_llama.hip defines its members for fp16 and holds the fp16 entry points,
// causal_lm_llama_bf16.hip the same for bf16, with every bf16 kernel instantiation) plus qk_norm = false; Qwen3's
// (causal_lm_qwen3.hip) is LlamaShared<E> plus a gemm_rope with the epilogue EP_QKNORM_ROPE, instantiated there.
#pragma once
#include <math.h>
#include <string>
#include <vector>

#include "clm_gemm.h"

namespace b2t {

// dimensions, head dim and weight pointers of a descriptor (0, or an error with the message set); causal_lm_llama.hip
int clm_llama_check_model(const b2t_clm_llama_t* m);
// the q / k norm weights of a checked model for the entry point `who`: a null array or entry and a q / k / v bias (Qwen3 has
// none, and EP_QKNORM_ROPE adds none) are refused; causal_lm_qwen3.hip
int clm_qknorm_check(const char* who, const b2t_clm_llama_t& m, const b2t_clm_qknorm_t* qkn);

// The statements every family's descriptor check makes, `pre` being the prefix of its messages (the family's name, or the entry
// point's for Phi-3); the head-dim set, the multiples-of-64 line and the extras stay with the family, in the family's order.
inline int clm_check_dims(const char* pre, const b2t_clm_llama_t* m) {
  B2T_REQUIRE(m, "%s: null model", pre);
  B2T_REQUIRE(m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->n_kv_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 &&
              m->max_pos > 0,
              "%s: bad dimensions (layers %d, d %d, heads %d, kv heads %d, ffn %d, vocab %d, max_pos %d)", pre, m->n_layers,
              m->d_model, m->n_heads, m->n_kv_heads, m->ffn_dim, m->vocab, m->max_pos);
  return 0;
}
inline int clm_check_gqa(const char* pre, const b2t_clm_llama_t& m) {
  B2T_REQUIRE(m.n_heads % m.n_kv_heads == 0, "%s: n_heads %d is not a multiple of n_kv_heads %d", pre, m.n_heads, m.n_kv_heads);
  return 0;
}
inline int clm_check_eps(const char* pre, const b2t_clm_llama_t& m) {
  B2T_REQUIRE(m.rms_eps >= 0.f && m.rms_eps < 1.f, "%s: rms_eps %g outside [0, 1)", pre, (double)m.rms_eps);
  return 0;
}
// the model's own pointers; `own`: whether the family's own per-layer array, where it has one, is there
inline int clm_check_pointers(const char* pre, const b2t_clm_llama_t& m, bool own = true) {
  B2T_REQUIRE(m.embed_tokens && m.lm_head && m.final_norm_w && m.rope_cos && m.rope_sin &&
              (m.n_layers == 0 || (m.layers_host && own)), "%s: null weight pointer", pre);
  return 0;
}
// layer l's six matrices and norms (qkv_b may be null: no q / k / v biases); `own`: the family's own pointers of the layer
inline int clm_check_layer(const char* pre, const b2t_clm_llama_layer_t& w, int l, bool own = true) {
  B2T_REQUIRE(w.norm1_w && w.norm2_w && w.qkv_w && w.o_w && w.gate_up_w && w.down_w && own, "%s: null weight pointer in layer %d",
              pre, l);
  return 0;
}
// dimensions a descriptor must have for the sizes of a layout to mean anything (the full check is the family's check)
inline bool llama_dims_ok(const b2t_clm_llama_t* m) {
  return m && m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->n_kv_heads > 0 && m->ffn_dim > 0 && m->vocab > 0;
}

// The launches of the Llama policy for element type E, which the other families' policies share (Qwen3's and OLMo-2's put a QKV
// GEMM of their own in front of gemm_rope, Mixtral's takes it as it is), so that their kernels are instantiated in one unit:
// the template has no definitions; the members are specialised in causal_lm_llama.hip for _Float16 and in
// causal_lm_llama_bf16.hip for __bf16, each with its launch.
template <class El>
struct LlamaShared {
  using E = El;
  static int gemm_rope(const ClmGemm& g, hipStream_t s);
  static int gemm_swiglu(const ClmGemm& g, hipStream_t s);
  static int gemm_resid(const ClmGemm& g, hipStream_t s);
  static int gemm_head(const ClmGemm& g, hipStream_t s);
  static int embed(const int* ids, const E* et, float* resid, int d, long long rows, hipStream_t s);
  static int rmsnorm(const float* x, const int* rowmap, long long n, const E* w, float eps, E* out, int d, hipStream_t s);
  static int attn(const E* qkv, E* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s);
  static int attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start, int n_seq, int Hq,
                       int Hkv, int hd, hipStream_t s);
};
// the Llama policy of the forward for element type El
template <class El>
struct LlamaPolicy : LlamaShared<El> {
  static constexpr bool qk_norm = false;
};

namespace {

// resid[t] = embed_tokens[id[t]] (fp32)
template <class E>
__global__ __launch_bounds__(256) void clm_llama_embed_kernel(const int* ids, const E* et, float* resid, int d) {
  const int t = blockIdx.x;
  const E* a = et + (long long)ids[t] * d;
  float* o = resid + (long long)t * d;
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (float)a[c];
}

// out[r] = E(RMSNorm(x[rowmap ? rowmap[r] : r])) for r < rows; zeros for rows <= r < gridDim.x (the operand's padding)
template <class E>
__global__ __launch_bounds__(256) void clm_llama_rmsnorm_kernel(const float* x, const int* rowmap, int rows, const E* w, float eps,
                                                                E* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  E* o = out + (long long)r * d;
  if (r >= rows) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)0.f;
    return;
  }
  const float* xr = x + (long long)(rowmap ? rowmap[r] : r) * d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) v += xr[c] * xr[c];
  const float rstd = 1.0f / sqrtf(block_sum256(v, red) / d + eps);
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)(xr[c] * rstd * (float)w[c]);
}

// Workspace of a forward over `rows` rows with `hrows` head rows and `ints` index entries (2-byte elements either way)
inline ClmLayout llama_layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * (m->d_model / m->n_heads);
  return clm_layout(m->d_model, qw, m->ffn_dim, m->vocab, rows, hrows, ints);
}

// The forward over r.rows rows up to the per-row log-probs logp[Mh]; attn(layer, qkv, out) enqueues one layer's attention,
// mlp(layer, x16, resid) one layer's MLP: resid += MLP(x16), x16 being E(RMSNorm(resid; norm2_w)) with its padding rows zero.
// qkn is the per-layer q / k norm weights of a policy with qk_norm (checked by clm_qknorm_check), unused otherwise.
// f8 (causal_lm_llama_fp8.hip, whose policy's GEMMs read B packed): the scales of the projections kept in FP8, the codes being
// where the dense matrices are; null for every other caller.
template <class P, class Attn, class Mlp>
int llama_forward_mlp(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                      const b2t_clm_qknorm_t* qkn, Mlp&& mlp, const b2t_clm_llama_fp8_t* f8 = nullptr) {
  using E = typename P::E;
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = d / Hq, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  E* x16 = reinterpret_cast<E*>(base + L.x16);
  E* qkv = reinterpret_cast<E*>(base + L.qkv);
  auto W = [](const void* p) { return static_cast<const E*>(p); };
  if (int rc = P::embed(r.d_ids, W(m.embed_tokens), resid, d, rows, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm1_w), m.rms_eps, x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = w.qkv_w; g.M = (int)rows; g.N = qw; g.K = d; g.bias = w.qkv_b; g.out16 = qkv; g.ldo = qw;
    g.qscale = 1.0f / sqrtf((float)hd); g.qcols = Hq * hd;
    g.pos = r.d_pos; g.rope_cos = m.rope_cos; g.rope_sin = m.rope_sin; g.rope_cols = (Hq + Hkv) * hd; g.hd = hd;
    if constexpr (P::qk_norm) { g.qnorm_w = qkn[l].q_norm_w; g.knorm_w = qkn[l].k_norm_w; g.rms_eps = m.rms_eps; }
    if (f8) { g.b_scale = f8->layers_host[l].qkv_s; g.b_block_k = f8->block_k; }
    if (int rc = P::gemm_rope(g, s)) return rc;
    if (int rc = attn(l, qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.o_w; g.M = (int)rows; g.N = d; g.K = d; g.resid = resid; g.ldo = d;
    if (f8) { g.b_scale = f8->layers_host[l].o_s; g.b_block_k = f8->block_k; }
    if (int rc = P::gemm_resid(g, s)) return rc;
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm2_w), m.rms_eps, x16, d, s)) return rc;
    if (int rc = mlp(l, x16, resid)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = P::rmsnorm(resid, r.d_src, r.Mh, W(m.final_norm_w), m.rms_eps, x16, d, s)) return rc;
  return clm_head(x16, m.lm_head, m.vocab, d, r, L, base, s, &P::gemm_head);
}

// The forward with the family's dense SwiGLU MLP: gate / up GEMM (EP_SWIGLU), down GEMM into the residual.
template <class P, class Attn>
int llama_forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                  const b2t_clm_qknorm_t* qkn = nullptr, const b2t_clm_llama_fp8_t* f8 = nullptr) {
  using E = typename P::E;
  const int d = m.d_model, F = m.ffn_dim;
  E* hb = reinterpret_cast<E*>(base + L.hbuf);
  auto mlp = [&](int l, const E* x16, float* resid) -> int {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    ClmGemm g{};
    g.A = x16; g.B = w.gate_up_w; g.M = (int)r.rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (f8) { g.b_scale = f8->layers_host[l].gate_up_s; g.b_block_k = f8->block_k; }
    if (int rc = P::gemm_swiglu(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.down_w; g.M = (int)r.rows; g.N = d; g.K = F; g.resid = resid; g.ldo = d;
    if (f8) { g.b_scale = f8->layers_host[l].down_s; g.b_block_k = f8->block_k; }
    return P::gemm_resid(g, s);
  };
  return llama_forward_mlp<P>(m, r, L, base, attn, s, qkn, mlp, f8);
}

// What a family whose descriptor obeys the Llama rule hd = d_model / n_heads hands the bodies and the size rules beside layout
// and forward (the contract in clm_internal.h): the model check alone as its check, and the two attention launches, which
// are told the layer (gpt-oss, clm_gptoss.h: a sink per head and a window per layer; nobody else looks at it).
struct LlamaFamilyBase {
  using Model = b2t_clm_llama_t;
  using Extra = b2t_clm_qknorm_t;
  static int kv_heads(const b2t_clm_llama_t& m) { return m.n_kv_heads; }
  template <class X>
  static int head_dim(const b2t_clm_llama_t& m, const X*) { return m.d_model / m.n_heads; }
  template <class X>
  static float attn_cap(const X*) { return 0.f; }
  template <class X>
  static bool dims_ok(const b2t_clm_llama_t* m, const X*) { return llama_dims_ok(m) && m->d_model % m->n_heads == 0; }
  template <class P, class X>
  static int check(const char*, const b2t_clm_llama_t* m, const X*) { return clm_llama_check_model(m); }
  template <class P, class X>
  static int attn(const b2t_clm_llama_t& m, const X*, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                  const int* seq_off, int n_seq, hipStream_t s) {
    return P::attn(qkv, out, seq_off, n_seq, m.n_heads, m.n_kv_heads, m.d_model / m.n_heads, s);
  }
  template <class P, class X>
  static int attn_tree(const b2t_clm_llama_t& m, const X*, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                       const int* seq_off, const int* tok_node, const int* own_start, int n_seq, hipStream_t s) {
    return P::attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, m.n_heads, m.n_kv_heads, m.d_model / m.n_heads, s);
  }
};

// The Llama family's (Qwen3 included: P::qk_norm): the Llama layout, the refusals that go with the q / k norm array behind the
// model check, and llama_forward.
struct LlamaFamily : LlamaFamilyBase {
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const void* /*extra*/ = nullptr) {
    return llama_layout(m, rows, hrows, ints);   // the q / k norm array changes no size
  }
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_qknorm_t* qkn) {
    if (int rc = clm_llama_check_model(m)) return rc;
    if constexpr (P::qk_norm) return clm_qknorm_check(who, *m, qkn);
    return 0;
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_qknorm_t* qkn) {
    return llama_forward<P>(m, r, L, base, attn, s, qkn);
  }
};

}  // namespace
}  // namespace b2t
