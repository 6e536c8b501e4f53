// causal_lm_neox.hip — the scoring forward of causal_lm.hip for GPT-NeoX (HF GPTNeoXForCausalLM with head dim 64 or 128: of the Pythia
// suite 70M, 160M, 410M, 1.4B, 6.9B, 12B; pythia-2.8b, pythia-1b and GPT-NeoX-20B have head dims 80, 256 and 96 and are refused):
// b2t_clm_neox_score_f16 over packed sequences, b2t_clm_neox_score_tree_f16 over the shared-prefix token tree and
// b2t_clm_neox_score_tree_cached_f16 behind a context cache.  GPT-NeoX has OPT's pieces -- LayerNorm with eps 1e-5, biased
// projections, multi-head attention with q scaled by head_dim^-0.5 -- and three things of its own: rotary positions on only
// the first rotary_ndims dims of every q and k head, the erf GELU, and the parallel residual x + attn(ln1(x)) + mlp(ln2(x)).
//
// Numerics contract (what ref_logp_neox of tests/test_clm_neox_host.py rounds):
//   - weights are fp16; GEMM operands are fp16, accumulation fp32 (v_mfma_f32_32x32x16_f16);
//   - the residual stream (the fp16 embedding row widened), the LayerNorm statistics, the rotation, the activation, softmax /
//     log-softmax and the sums are fp32; cos / sin come from an fp32 table [max_pos][rotary_ndims / 2] the host builds in double;
//   - rounded to fp16, once each: both LayerNorm outputs; q, k and v; P per 32-key block; the attention output; gelu(fc1);
//   - the QKV GEMM's epilogue (EP_ROPE_PART, clm_gemm.h), on the fp32 accumulator, in this order: + bias; the rotation of the
//     rotary dims of every q and k head (rotate-half pairs (i, i + rotary_ndims / 2), i < rotary_ndims / 2); the other dims
//     pass through; q times head_dim^-0.5; the one rounding.  v gets the bias only;
//   - the fc1 GEMM's epilogue: + bias, then gelu(v) = 0.5 v (1 + erf(v / sqrt 2)) (EP_GELU_ERF; act 0) or the tanh form
//     gelu_new (EP_GELU, causal_lm_gpt2.hip's; act 1: "gelu_new" = "gelu_fast" = "gelu_pytorch_tanh") in fp32, one rounding.  A
//     saturated pre-activation gives v or -0.0 / 0, never NaN;
//   - the residual order: both LayerNorms of a layer read the layer's input x; the residual then receives the attention
//     branch (the dense GEMM's EP_RESID, += in fp32) first and the MLP branch (the fc2 GEMM's EP_RESID) second.
//   Every output element is computed by one thread in an order that depends on its own row alone: flat, tree and cached calls
//   are bit-identical, and so is a sequence alone or in a batch.
//
// Kernels per layer, in a buffer order that needs no workspace beyond the OPT layout's: ln1(resid) -> x16; QKV GEMM -> qkv;
// ln2(resid) -> x16 (free again); fc1 GEMM -> hbuf; attention qkv -> x16; dense GEMM += resid; fc2 GEMM += resid.  Then the final
// LayerNorm of the head rows and clm_head on embed_out.  The LayerNorm, attention, residual and head kernels are the OPT paths'
// through their launchers (attention with Hkv = Hq), the embedding is the Llama family's kernel (LlamaShared, clm_llama.h), the
// cached entry point's body is clm_score_tree_cached, and every GEMM goes through the one tile rule (launch_gemm of
// causal_lm.hip).  This unit instantiates its two epilogues in fp16 on both tiles and nothing else.
// The layout the rotation relies on is made at load time (llm_rescore.neox_device_layout): query_key_value de-interleaved to
// q | k | v rows, and every q and k head's rows stored so that a rotary pair is 32 columns apart inside one 64-column slice
// (neox_head_perm); q . k is invariant under one permutation of both, v and dense are stored as they are.  The cache holds K
// rows after bias and rotation, in that stored order.
#include "clm_llama.h"

namespace b2t {
namespace {

int neox_gemm_rope(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE_PART>); }
int neox_gemm_gelu_erf(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_GELU_ERF>); }

// dimensions a descriptor must have for the sizes of neox_layout to mean anything (the full check is neox_check_model)
bool neox_dims_ok(const b2t_clm_neox_t* m) {
  return m && m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 && m->d_model % m->n_heads == 0;
}

// dimensions, head dim, rotary dims, activation and weight pointers of a descriptor (0, or an error under the entry point's name)
int neox_check_model(const char* who, const b2t_clm_neox_t* m) {
  B2T_REQUIRE(m, "%s: null model", who);
  B2T_REQUIRE(m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 && m->max_pos > 0,
              "%s: bad dimensions (layers %d, d %d, heads %d, ffn %d, vocab %d, max_pos %d)", who, m->n_layers, m->d_model,
              m->n_heads, m->ffn_dim, m->vocab, m->max_pos);
  B2T_REQUIRE(m->d_model % m->n_heads == 0, "%s: d_model %d is not a multiple of n_heads %d", who, m->d_model, m->n_heads);
  const int hd = m->d_model / m->n_heads;
  B2T_REQUIRE(hd == 64 || hd == 128, "%s: unsupported head dim %d (64 or 128)", who, hd);
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0, "%s: d_model %d and ffn_dim %d must be multiples of 64", who, m->d_model,
              m->ffn_dim);
  B2T_REQUIRE(m->rotary_ndims == hd / 4 || m->rotary_ndims == hd / 2 || m->rotary_ndims == hd,
              "%s: unsupported rotary_ndims %d for head dim %d (%d, %d or %d)", who, m->rotary_ndims, hd, hd / 4, hd / 2, hd);
  B2T_REQUIRE(m->act == B2T_CLM_NEOX_ACT_GELU_ERF || m->act == B2T_CLM_NEOX_ACT_GELU_TANH, "%s: unknown act %d (0: erf GELU, 1: tanh GELU)",
              who, m->act);
  B2T_REQUIRE(m->rope_cos && m->rope_sin, "%s: null rotary table", who);
  B2T_REQUIRE(m->embed_in && m->embed_out && m->final_ln_w && m->final_ln_b && (m->n_layers == 0 || m->layers_host),
              "%s: null weight pointer", who);
  for (int l = 0; l < m->n_layers; ++l) {
    const b2t_clm_layer_t& w = m->layers_host[l];
    B2T_REQUIRE(w.ln1_w && w.ln1_b && w.qkv_w && w.qkv_b && w.out_w && w.out_b && w.ln2_w && w.ln2_b && w.fc1_w && w.fc1_b &&
                w.fc2_w && w.fc2_b, "%s: null weight pointer in layer %d", who, l);
  }
  return 0;
}

inline ClmLayout neox_layout(const b2t_clm_neox_t* m, long long rows, long long head_rows, size_t ints) {
  return clm_layout(m->d_model, 3LL * m->d_model, m->ffn_dim, m->vocab, rows, head_rows, ints);
}

// The forward over r.rows rows up to the per-row log-probs logp[r.Mh] (base + L.logp); attn(layer, qkv, out) enqueues one
// layer's attention from qkv ([rows][3d]) into out ([rows][d]).  The order of the kernels is the header's: both LayerNorms
// read the layer's input, and the residual receives the attention branch first, then the MLP branch.
template <class Attn>
int neox_forward(const b2t_clm_neox_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s) {
  const int d = m.d_model, hd = d / m.n_heads, F = m.ffn_dim, M = (int)r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  _Float16* x16 = reinterpret_cast<_Float16*>(base + L.x16);
  _Float16* qkv = reinterpret_cast<_Float16*>(base + L.qkv);
  _Float16* hb = reinterpret_cast<_Float16*>(base + L.hbuf);
  auto H16 = [](const void* p) { return static_cast<const _Float16*>(p); };
  const ClmGemmLaunch fc1 = m.act == B2T_CLM_NEOX_ACT_GELU_TANH ? &clm_gemm_gelu : &neox_gemm_gelu_erf;
  if (int rc = LlamaShared<_Float16>::embed(r.d_ids, H16(m.embed_in), resid, d, r.rows, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_layer_t& w = m.layers_host[l];
    if (int rc = clm_launch_layernorm(resid, nullptr, r.rows, H16(w.ln1_w), H16(w.ln1_b), x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = w.qkv_w; g.M = M; g.N = 3 * d; g.K = d; g.bias = w.qkv_b; g.out16 = qkv; g.ldo = 3 * d;
    g.qscale = 1.0f / sqrtf((float)hd); g.qcols = d;
    g.pos = r.d_pos; g.rope_cos = m.rope_cos; g.rope_sin = m.rope_sin; g.rope_cols = 2 * d; g.hd = hd; g.rope_half = m.rotary_ndims / 2;
    if (int rc = neox_gemm_rope(g, s)) return rc;
    if (int rc = clm_launch_layernorm(resid, nullptr, r.rows, H16(w.ln2_w), H16(w.ln2_b), x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.fc1_w; g.M = M; g.N = F; g.K = d; g.bias = w.fc1_b; g.out16 = hb; g.ldo = F;
    if (int rc = fc1(g, s)) return rc;
    if (int rc = attn(l, qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.out_w; g.M = M; g.N = d; g.K = d; g.bias = w.out_b; g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.fc2_w; g.M = M; g.N = d; g.K = F; g.bias = w.fc2_b; g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = clm_launch_layernorm(resid, r.d_src, r.Mh, H16(m.final_ln_w), H16(m.final_ln_b), x16, d, s)) return rc;
  return clm_head(x16, m.embed_out, m.vocab, d, r, L, base, s);
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_neox_ws_bytes(const b2t_clm_neox_t* model, long long n_tokens, int n_seq) {
  if (!neox_dims_ok(model) || n_tokens < 1 || n_seq < 1 || n_seq > n_tokens) return 0;
  return neox_layout(model, n_tokens, n_tokens - n_seq, flat_ints(n_tokens, n_seq)).total;
}

extern "C" int b2t_clm_neox_score_f16(const b2t_clm_neox_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                      float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "b2t_clm_neox_score_f16";
  if (int rc = neox_check_model(who, model)) return rc;
  const b2t_clm_neox_t& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  const ClmLayout L = neox_layout(model, M, M - n_seq, flat_ints(M, n_seq));
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmFlatIndex ix;
  if (int rc = clm_build_flat_index("b2t_clm_neox_score_f16 upload", ids_host, seq_off_host, n_seq,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int, const _Float16* qkv, _Float16* out) {
    return clm_launch_attn(qkv, out, ix.d_soff, n_seq, m.n_heads, m.n_heads, m.d_model / m.n_heads, s);
  };
  if (int rc = neox_forward(m, ix.run, L, base, attn, s)) return rc;
  return clm_launch_seq_sum(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hoff, scores_out, tok_logp_out, n_seq, s);
}

extern "C" size_t b2t_clm_neox_tree_ws_bytes(const b2t_clm_neox_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  if (!neox_dims_ok(model) || n_nodes < 1 || n_nodes > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  return neox_layout(model, n_nodes, n_nodes, tree_ints(n_nodes, n_tokens, n_seq)).total;
}

extern "C" int b2t_clm_neox_score_tree_f16(const b2t_clm_neox_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                           int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                           size_t ws_bytes, void* stream) {
  const char* who = "b2t_clm_neox_score_tree_f16";
  if (int rc = neox_check_model(who, model)) return rc;
  const b2t_clm_neox_t& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  ClmTreePlan& plan = clm_plan_tree(ids_host, seq_off_host, n_seq);   // a node's rotary position is its depth
  const long long Mn = plan.Mn;
  if (n_nodes_out) *n_nodes_out = Mn;
  const ClmLayout L = neox_layout(model, Mn, Mn, tree_ints(Mn, M, n_seq));
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmTreeIndex ix;
  if (int rc = clm_build_tree_index("b2t_clm_neox_score_tree_f16 upload", ids_host, seq_off_host, n_seq, plan, 0,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int, const _Float16* qkv, _Float16* out) {
    return clm_launch_attn_tree(qkv, out, ix.d_soff, ix.d_node, ix.d_own, n_seq, m.n_heads, m.n_heads, m.d_model / m.n_heads, s);
  };
  if (int rc = neox_forward(m, ix.run, L, base, attn, s)) return rc;
  return clm_launch_seq_sum_tree(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hrow, scores_out, tok_logp_out, n_seq, s);
}

extern "C" size_t b2t_clm_neox_cache_kv_bytes(const b2t_clm_neox_t* model, int cap) {
  if (!neox_dims_ok(model) || cap < 1 || cap > model->max_pos || model->n_layers < 1) return 0;
  return (size_t)model->n_layers * (size_t)cap * 2 * (size_t)model->d_model * sizeof(_Float16);
}

extern "C" size_t b2t_clm_neox_tree_cached_ws_bytes(const b2t_clm_neox_t* model, long long n_rows, long long n_tokens, int n_seq) {
  if (!neox_dims_ok(model) || n_rows < 1 || n_rows > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  const size_t tree = neox_layout(model, n_rows, n_rows, tree_ints(n_rows, n_tokens, n_seq)).total;
  return clm_cached_state(tree, n_rows, model->n_heads, model->d_model).total;
}

extern "C" int b2t_clm_neox_score_tree_cached_f16(const b2t_clm_neox_t* model, b2t_clm_cache_t* cache, int update,
                                                  const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                  float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                  int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = neox_check_model("b2t_clm_neox_score_tree_cached_f16", model)) return rc;
  const b2t_clm_neox_t& m = *model;
  const ClmCacheDims dims{m.vocab, m.max_pos, m.n_heads, m.n_heads, m.d_model / m.n_heads};
  return clm_score_tree_cached(
      "b2t_clm_neox_score_tree_cached_f16", "b2t_clm_neox_score_tree_f16", dims, cache, update, ids_host, seq_off_host, n_seq,
      scores_out, tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, as_stream(stream),
      [&](long long rows, size_t ints) { return neox_layout(model, rows, rows, ints); },
      [&](const ClmRun& r, const ClmLayout& L, char* base, auto&& attn, hipStream_t s) { return neox_forward(m, r, L, base, attn, s); });
}
