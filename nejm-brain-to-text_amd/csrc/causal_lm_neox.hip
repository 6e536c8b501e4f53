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
// entry points' bodies and the size rules are every family's (clm_internal.h) under NeoxFamily, and every GEMM goes through the
// one tile rule (launch_gemm of causal_lm.hip).  This unit instantiates its two epilogues in fp16 on both tiles and nothing else.
// The layout the rotation relies on is made at load time (llm_rescore.neox_device_layout): query_key_value de-interleaved to
// q | k | v rows, and every q and k head's rows stored so that a rotary pair is 32 columns apart inside one 64-column slice
// (neox_head_perm); q . k is invariant under one permutation of both, v and dense are stored as they are.  The cache holds K
// rows after bias and rotation, in that stored order.
#include "clm_llama.h"

namespace b2t {
namespace {

int neox_gemm_rope(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE_PART>); }
int neox_gemm_gelu_erf(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_GELU_ERF>); }

// dimensions, head dim, rotary dims, activation and weight pointers of a descriptor (0, or an error under the entry point's name)
int neox_check_model(const char* who, const b2t_clm_neox_t* m) {
  if (int rc = clm_check_mha_dims(who, m)) return rc;
  const int hd = m->d_model / m->n_heads;
  B2T_REQUIRE(hd == 64 || hd == 128, "%s: unsupported head dim %d (64 or 128)", who, hd);
  if (int rc = clm_check_mult64(who, m->d_model, m->ffn_dim)) return rc;
  B2T_REQUIRE(m->rotary_ndims == hd / 4 || m->rotary_ndims == hd / 2 || m->rotary_ndims == hd,
              "%s: unsupported rotary_ndims %d for head dim %d (%d, %d or %d)", who, m->rotary_ndims, hd, hd / 4, hd / 2, hd);
  B2T_REQUIRE(m->act == B2T_CLM_NEOX_ACT_GELU_ERF || m->act == B2T_CLM_NEOX_ACT_GELU_TANH, "%s: unknown act %d (0: erf GELU, 1: tanh GELU)",
              who, m->act);
  B2T_REQUIRE(m->rope_cos && m->rope_sin, "%s: null rotary table", who);
  B2T_REQUIRE(m->embed_in && m->embed_out && m->final_ln_w && m->final_ln_b && (m->n_layers == 0 || m->layers_host),
              "%s: null weight pointer", who);
  for (int l = 0; l < m->n_layers; ++l)
    if (int rc = clm_check_mha_layer(who, m->layers_host[l], l)) return rc;
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

// what the entry-point bodies and the size rules of clm_internal.h take from this family; the dims rule (clm_mha_dims_ok) and the
// attention with Hkv = Hq are ClmMhaFamily's
struct NeoxFamily : ClmMhaFamily {
  using Model = b2t_clm_neox_t;
  static ClmLayout layout(const b2t_clm_neox_t* m, long long rows, long long hrows, size_t ints, const void*) {
    return neox_layout(m, rows, hrows, ints);
  }
  template <class P>
  static int check(const char* who, const b2t_clm_neox_t* m, const void*) { return neox_check_model(who, m); }
  template <class P, class Attn>
  static int forward(const b2t_clm_neox_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s, const void*) {
    return neox_forward(m, r, L, base, attn, s);
  }
};
struct NeoxPolicy { using E = _Float16; };   // fp16 alone; neox_forward takes nothing else from a policy

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_neox_ws_bytes(const b2t_clm_neox_t* model, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<NeoxFamily>(model, n_tokens, n_seq);
}

extern "C" int b2t_clm_neox_score_f16(const b2t_clm_neox_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                      float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<NeoxPolicy, NeoxFamily>("b2t_clm_neox_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                  tok_logp_out, ws, ws_bytes, stream);
}

extern "C" size_t b2t_clm_neox_tree_ws_bytes(const b2t_clm_neox_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<NeoxFamily>(model, n_nodes, n_tokens, n_seq);
}

extern "C" int b2t_clm_neox_score_tree_f16(const b2t_clm_neox_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                           int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                           size_t ws_bytes, void* stream) {
  return clm_family_score_tree<NeoxPolicy, NeoxFamily>("b2t_clm_neox_score_tree_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                       tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" size_t b2t_clm_neox_cache_kv_bytes(const b2t_clm_neox_t* model, int cap) {
  return clm_family_cache_kv_bytes<NeoxFamily>(model, cap);
}

extern "C" size_t b2t_clm_neox_tree_cached_ws_bytes(const b2t_clm_neox_t* model, long long n_rows, long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<NeoxFamily>(model, n_rows, n_tokens, n_seq);
}

extern "C" int b2t_clm_neox_score_tree_cached_f16(const b2t_clm_neox_t* model, b2t_clm_cache_t* cache, int update,
                                                  const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                  float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                  int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<NeoxPolicy, NeoxFamily>("b2t_clm_neox_score_tree_cached_f16", "b2t_clm_neox_score_tree_f16", model,
                                                              cache, update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                              n_rows_out, n_reused_out, ws, ws_bytes, stream);
}
