// clm_llama.h — the Llama-family forward (causal_lm_llama.hip's header has the contract and the kernel sequence), written once
// for both element types: the embed and RMSNorm kernels, llama_forward and the bodies of the flat and the tree entry point are
// templates, on the element type or on a policy P that names it and supplies the launches that differ with it:
//   P::E                                        _Float16 or __bf16 (ClmElem, clm_internal.h)
//   P::gemm_rope, gemm_swiglu, gemm_resid, gemm_head (g, s)   the four GEMMs, each through the one tile rule launch_gemm
//   P::embed, P::rmsnorm                        the two kernels below (LlamaOps<E>)
//   P::attn, P::attn_tree                       the flat and the tree attention launcher
//   P::qk_norm                                  whether the QKV GEMM's epilogue norms the q and k heads (Qwen3): llama_forward then
//                                               hands it the layer's weights from the b2t_clm_qknorm_t array and rms_eps
// causal_lm_llama.hip holds the fp16 policy and the fp16 entry points (the cached one included), causal_lm_llama_bf16.hip the
// bf16 policy, every bf16 kernel instantiation and the two bf16 entry points.  causal_lm_qwen3.hip holds the two Qwen3
// policies: gemm_rope with the epilogue EP_QKNORM_ROPE, instantiated there, and every other launch through LlamaShared<E>.
// The two entry-point bodies also serve a family with another layer (OLMo-2, clm_olmo2.h; Mixtral, clm_moe.h): their second
// template argument supplies the layout, the refusals that go with the family's extra argument and the forward (LlamaFamily
// below by default), and -- through LlamaFamilyBase, or on its own for Gemma-2 (clm_gemma2.h), whose head dim is not
// d_model / n_heads, and Phi-3 (clm_phi3.h), whose head dim may be 96 -- the model check and the attention launches.
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

// The launches of the Llama policy for element type E that another family's policy shares (P's list above; Qwen3's and OLMo-2's
// policies put a QKV GEMM of their own in front of gemm_rope, Mixtral's takes it as it is),
// so that their kernels are instantiated in one unit: the members are defined in causal_lm_llama.hip for _Float16 and in
// causal_lm_llama_bf16.hip for __bf16, each forwarding to its unit's policy.
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
// the specialisations the two units define, declared before any use
#define B2T_LLAMA_SHARED(EL)                                                                                                  \
  template <> int LlamaShared<EL>::gemm_rope(const ClmGemm&, hipStream_t);                                                    \
  template <> int LlamaShared<EL>::gemm_swiglu(const ClmGemm&, hipStream_t);                                                  \
  template <> int LlamaShared<EL>::gemm_resid(const ClmGemm&, hipStream_t);                                                   \
  template <> int LlamaShared<EL>::gemm_head(const ClmGemm&, hipStream_t);                                                    \
  template <> int LlamaShared<EL>::embed(const int*, const EL*, float*, int, long long, hipStream_t);                         \
  template <> int LlamaShared<EL>::rmsnorm(const float*, const int*, long long, const EL*, float, EL*, int, hipStream_t);     \
  template <> int LlamaShared<EL>::attn(const EL*, EL*, const int*, int, int, int, int, hipStream_t);                         \
  template <> int LlamaShared<EL>::attn_tree(const EL*, EL*, const int*, const int*, const int*, int, int, int, int, hipStream_t);
B2T_LLAMA_SHARED(_Float16)
B2T_LLAMA_SHARED(__bf16)
#undef B2T_LLAMA_SHARED

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

// the part of a policy that is the same text for both element types
template <class El>
struct LlamaOps {
  using E = El;
  static constexpr bool qk_norm = false;
  static int embed(const int* ids, const E* et, float* resid, int d, long long rows, hipStream_t s) {
    hipLaunchKernelGGL(clm_llama_embed_kernel<E>, dim3((unsigned)rows), dim3(256), 0, s, ids, et, resid, d);
    B2T_CHECK_LAUNCH("clm_llama_embed_kernel");
    return 0;
  }
  static int rmsnorm(const float* x, const int* rowmap, long long n, const E* w, float eps, E* out, int d, hipStream_t s) {
    hipLaunchKernelGGL(clm_llama_rmsnorm_kernel<E>, dim3((unsigned)rup(n, ROWPAD)), dim3(256), 0, s, x, rowmap, (int)n, w, eps, out, d);
    B2T_CHECK_LAUNCH("clm_llama_rmsnorm_kernel");
    return 0;
  }
};

// Workspace of a forward over `rows` rows with `hrows` head rows and `ints` index entries (2-byte elements either way)
inline ClmLayout llama_layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * (m->d_model / m->n_heads);
  return clm_layout(m->d_model, qw, m->ffn_dim, m->vocab, rows, hrows, ints);
}

// The forward over r.rows rows up to the per-row log-probs logp[Mh]; attn(layer, qkv, out) enqueues one layer's attention,
// mlp(layer, x16, resid) one layer's MLP: resid += MLP(x16), x16 being E(RMSNorm(resid; norm2_w)) with its padding rows zero.
// qkn is the per-layer q / k norm weights of a policy with qk_norm (checked by clm_qknorm_check), unused otherwise.
template <class P, class Attn, class Mlp>
int llama_forward_mlp(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                      const b2t_clm_qknorm_t* qkn, Mlp&& mlp) {
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
    if (int rc = P::gemm_rope(g, s)) return rc;
    if (int rc = attn(l, qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.o_w; g.M = (int)rows; g.N = d; g.K = d; g.resid = resid; g.ldo = d;
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
                  const b2t_clm_qknorm_t* qkn = nullptr) {
  using E = typename P::E;
  const int d = m.d_model, F = m.ffn_dim;
  E* hb = reinterpret_cast<E*>(base + L.hbuf);
  auto mlp = [&](int l, const E* x16, float* resid) -> int {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    ClmGemm g{};
    g.A = x16; g.B = w.gate_up_w; g.M = (int)r.rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (int rc = P::gemm_swiglu(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.down_w; g.M = (int)r.rows; g.N = d; g.K = F; g.resid = resid; g.ldo = d;
    return P::gemm_resid(g, s);
  };
  return llama_forward_mlp<P>(m, r, L, base, attn, s, qkn, mlp);
}

// What a family whose descriptor obeys the Llama rule hd = d_model / n_heads hands the entry-point bodies beside layout, check
// and forward: the model check, the head dim and the two attention launches, which are told the layer (gpt-oss, clm_gptoss.h:
// a sink per head and a window per layer; nobody else looks at it).  Gemma-2 (clm_gemma2.h), whose head dim is a
// field of its own descriptor and whose attention takes a soft cap, supplies its own.
struct LlamaFamilyBase {
  template <class X>
  static int check_model(const b2t_clm_llama_t* m, const X*) { return clm_llama_check_model(m); }
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

// What the two entry-point bodies below take from a family: the workspace layout, the refusals that go with the q / k norm
// array, and the forward.  This is the Llama family's (Qwen3 included: P::qk_norm); OLMo-2's is Olmo2Family (clm_olmo2.h).
struct LlamaFamily : LlamaFamilyBase {
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const void* /*extra*/ = nullptr) {
    return llama_layout(m, rows, hrows, ints);   // the q / k norm array changes no size
  }
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t& m, const b2t_clm_qknorm_t* qkn) {
    if constexpr (P::qk_norm) return clm_qknorm_check(who, m, qkn);
    return 0;
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_qknorm_t* qkn) {
    return llama_forward<P>(m, r, L, base, attn, s, qkn);
  }
};

// The flat entry point of a policy; `who` is its name.  `extra` is what the family's layout, check and forward take beside the
// model, of the family's own type X: the q / k norm array (Qwen3, OLMo-2) or a descriptor (Mixtral's b2t_clm_moe_t, clm_moe.h).
template <class P, class Fam = LlamaFamily, class X = b2t_clm_qknorm_t>
int llama_score(const char* who, const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream, const X* extra = nullptr) {
  using E = typename P::E;
  if (int rc = Fam::check_model(model, extra)) return rc;
  const b2t_clm_llama_t& m = *model;
  if (int rc = Fam::template check<P>(who, m, extra)) return rc;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  const ClmLayout L = Fam::layout(model, M, M - n_seq, flat_ints(M, n_seq), extra);
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmFlatIndex ix;
  if (int rc = clm_build_flat_index((std::string(who) + " upload").c_str(), ids_host, seq_off_host, n_seq,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int l, const E* qkv, E* out) { return Fam::template attn<P>(m, extra, l, qkv, out, ix.d_soff, n_seq, s); };
  if (int rc = Fam::template forward<P>(m, ix.run, L, base, attn, s, extra)) return rc;
  return clm_launch_seq_sum(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hoff, scores_out, tok_logp_out, n_seq, s);
}

// The tree entry point of a policy.
template <class P, class Fam = LlamaFamily, class X = b2t_clm_qknorm_t>
int llama_score_tree(const char* who, const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                     int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                     void* stream, const X* extra = nullptr) {
  using E = typename P::E;
  if (int rc = Fam::check_model(model, extra)) return rc;
  const b2t_clm_llama_t& m = *model;
  if (int rc = Fam::template check<P>(who, m, extra)) return rc;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  ClmTreePlan& plan = clm_plan_tree(ids_host, seq_off_host, n_seq);   // a node's rotary position is its depth, node_pos
  const long long Mn = plan.Mn;
  if (n_nodes_out) *n_nodes_out = Mn;
  const ClmLayout L = Fam::layout(model, Mn, Mn, tree_ints(Mn, M, n_seq), extra);
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmTreeIndex ix;
  if (int rc = clm_build_tree_index((std::string(who) + " upload").c_str(), ids_host, seq_off_host, n_seq, plan, 0,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int l, const E* qkv, E* out) {
    return Fam::template attn_tree<P>(m, extra, l, qkv, out, ix.d_soff, ix.d_node, ix.d_own, n_seq, s);
  };
  if (int rc = Fam::template forward<P>(m, ix.run, L, base, attn, s, extra)) return rc;
  return clm_launch_seq_sum_tree(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hrow, scores_out, tok_logp_out, n_seq, s);
}

}  // namespace
}  // namespace b2t
