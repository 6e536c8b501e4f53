// causal_lm_phi3.hip — the scoring forward of causal_lm_llama.hip for Phi-3 (HF Phi3ForCausalLM, model_type "phi3": Phi-3-mini,
// Phi-3.5-mini, Phi-3-medium, Phi-4, Phi-4-mini), in fp16 and bf16: b2t_clm_phi3_score_f16 / _bf16 over packed sequences,
// b2t_clm_phi3_score_tree_f16 / _bf16 over the shared-prefix token tree and b2t_clm_phi3_score_tree_cached_f16 behind a context
// cache.  Phi-3 is the Llama layer (pre-norm, grouped-query attention, SwiGLU, no bias anywhere) and differs from its forward in
// two places that reach the kernels:
//   - the head dim may be 96 (Phi-3-mini / 3.5-mini: 3072 / 32 heads).  The rotary epilogue of the QKV GEMM (EP_ROPE) needs a head
//     to tile into 64-column wave groups with its pairs 32 columns apart; 96 = 64 + 32 cannot be laid out that way with one
//     permutation for every q and k head;
//   - the rotation may be partial (Phi-4-mini: partial_rotary_factor 0.75): only the first rot = rotary_dims dims of a head are
//     rotated, pairs (c, c + rot / 2), the others pass through.
// So the rotation is a kernel of its own behind a QKV GEMM that keeps q | k in fp32, as OLMo-2's norms are.  LongRoPE (per-frequency
// short factors, an attention factor on cos and sin) is in the host's tables; the fused checkpoint tensors are the loader's.
// The head dim is a field of b2t_clm_phi3_t, as for Gemma-2: the QKV GEMM has N = (Hq + 2 Hkv) hd, the o_proj K = Hq hd.
//
// Numerics contract (what the fp64 restatement ref_logp_phi3 of tests/test_clm_phi3_host.py rounds), E = fp16 or bf16: the
// Llama family's with "rotation" read as above --
//   - weights, GEMM operands and attention operands are E; accumulation is fp32;
//   - the residual stream, the RMSNorm statistics, the rotation (cos / sin from the fp32 table, attention factor included),
//     softmax / log-softmax and the sums are fp32;
//   - rounded to E, once each: the RMSNorm outputs; q after rotation (or pass-through) and the factor head_dim^-0.5, which
//     multiplies every q dim; k after rotation (or pass-through); v; the attention's probabilities per 32-key block as the P.V
//     operand; the attention output; silu(gate) * up;
//   - the QKV GEMM's q | k columns are never rounded in front of the rotation: the GEMM stores its fp32 accumulator
//     (EP_QKV_F32) and the rotation reads it.
//   A rotated element is computed from its own pair alone, so a row's bits depend only on that row: flat, tree and cached calls
//   are byte-identical, a sequence scores the same alone or in a batch, and B2T_CLM_GEMM_256 / B2T_CLM_TRUNK_ATTN do not change
//   the bits.  K rows are cached after the rotation, in the Llama cache layout with the descriptor's head dim.
//
// Kernels per layer: clm_llama_rmsnorm_kernel -> QKV GEMM (EP_QKV_F32: q | k columns as fp32 accumulators into the fp32 region,
// v rounded into qkv) -> clm_phi3_rope_kernel (rotation, pass-through, q's scale, one rounding, into qkv in front of v) -> causal
// GQA attention (head dim 96: the templates of clm_attn.h instantiated here; 64 and 128: the launchers of the Llama forward)
// into the fp32 region, which the rotation has finished with -> o_proj GEMM (EP_RESID) -> RMSNorm -> gate / up GEMM (EP_SWIGLU)
// -> down GEMM (EP_RESID).  Embedding, final norm and head are the Llama forward's.  The rotation sits in a kernel that sees
// whole heads, so q / k rows stay in checkpoint order (no head_dim_perm); gate / up rows are interleaved as for Llama.
//
// This unit instantiates the EP_QKV_F32 epilogue (on both tiles), the rotation kernel and the flat and tree attention at head
// dim 96, in both element types, and the cached and trunk attention at 96 in fp16 (behind clm_launch_attn_cached of
// causal_lm_cache.hip, which hands head dim 96 to clm_launch_attn_cached_96 below); every other kernel is reached through
// LlamaShared<E>, the three entry-point bodies and the size rules are clm_internal.h's under Phi3Family.  No kernel
// here uses scratch (tests/test_clm_phi3_host.py checks it).  The workspace is phi3_layout (clm_phi3.h).
#include "clm_attn.h"
#include "clm_phi3.h"

namespace b2t {
namespace {

template <class El>
struct Phi3Policy : LlamaShared<El>, Phi3Ops<El> {
  using E = El;
  static int gemm_qkv(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_QKV_F32, El>); }
  static int attn(const E* qkv, E* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
    if (hd != 96) return LlamaShared<El>::attn(qkv, out, seq_off, n_seq, Hq, Hkv, hd, s);
    hipLaunchKernelGGL((clm_attn_kernel<96, E>), dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);
    B2T_CHECK_LAUNCH("clm_attn_kernel");
    return 0;
  }
  static int attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start, int n_seq, int Hq,
                       int Hkv, int hd, hipStream_t s) {
    if (hd != 96) return LlamaShared<El>::attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, Hq, Hkv, hd, s);
    hipLaunchKernelGGL((clm_attn_tree_kernel<96, E>), dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq,
                       Hkv);
    B2T_CHECK_LAUNCH("clm_attn_tree_kernel");
    return 0;
  }
};
using Phi3F16 = Phi3Policy<_Float16>;
using Phi3Bf16 = Phi3Policy<__bf16>;

}  // namespace

// launch_attn of causal_lm_cache.hip at head dim 96: stage B over the whole cached blocks, then the tree walk
int clm_launch_attn_cached_96(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s) {
  const int Rb = a.trunk ? a.R - a.R % 32 : 0;
  if (Rb > 0) {
    hipLaunchKernelGGL(clm_attn_trunk_kernel<96>, dim3((unsigned)((a.rows + 31) / 32), a.Hq), dim3(64), 0, s, qkv, slab, a.Hkv,
                       (int)a.rows, Rb / 32, a.st_ml, a.st_o);
    B2T_CHECK_LAUNCH("clm_attn_trunk_kernel");
  }
  hipLaunchKernelGGL(clm_attn_tree_cached_kernel<96>, dim3(a.n_seq, a.Hq), dim3(256), 0, s, qkv, slab, out, a.soff, a.node, a.own,
                     a.Hkv, a.R, Rb > 0 ? a.st_ml : nullptr, Rb > 0 ? a.st_o : nullptr, Rb / 32);
  B2T_CHECK_LAUNCH("clm_attn_tree_cached_kernel");
  return 0;
}

int clm_phi3_check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3) {
  B2T_REQUIRE(!m || p3, "%s: null phi3 descriptor", who);   // behind the null model, in front of the dimensions
  if (int rc = clm_check_dims(who, m)) return rc;
  const int hd = p3->head_dim, rot = p3->rotary_dims;
  B2T_REQUIRE(hd == 64 || hd == 96 || hd == 128, "%s: unsupported head dim %d (64, 96 or 128)", who, hd);
  B2T_REQUIRE(rot >= 2 && rot <= hd && rot % 2 == 0, "%s: rotary_dims %d is not an even number in [2, head_dim %d]", who, rot, hd);
  const long long qc = (long long)m->n_heads * hd, qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * hd;
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0 && qc % 64 == 0 && qw % 64 == 0,
              "%s: d_model %d, ffn_dim %d, n_heads * head_dim %lld and (n_heads + 2 n_kv_heads) * head_dim %lld must be multiples "
              "of 64", who, m->d_model, m->ffn_dim, qc, qw);
  if (int rc = clm_check_gqa(who, *m)) return rc;
  if (int rc = clm_check_eps(who, *m)) return rc;
  if (int rc = clm_check_pointers(who, *m)) return rc;
  for (int l = 0; l < m->n_layers; ++l) {
    if (int rc = clm_check_layer(who, m->layers_host[l], l)) return rc;
    B2T_REQUIRE(!m->layers_host[l].qkv_b, "%s: layer %d has q / k / v biases (qkv_b), which Phi-3 does not", who, l);
  }
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_phi3_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<Phi3Family>(model, n_tokens, n_seq, phi3);
}

extern "C" size_t b2t_clm_phi3_tree_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, long long n_nodes,
                                             long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<Phi3Family>(model, n_nodes, n_tokens, n_seq, phi3);
}

extern "C" size_t b2t_clm_phi3_cache_kv_bytes(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, int cap) {
  return clm_family_cache_kv_bytes<Phi3Family>(model, cap, phi3);
}

extern "C" size_t b2t_clm_phi3_tree_cached_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, long long n_rows,
                                                    long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<Phi3Family>(model, n_rows, n_tokens, n_seq, phi3);
}

extern "C" int b2t_clm_phi3_score_f16(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, const int32_t* ids_host,
                                      const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                      size_t ws_bytes, void* stream) {
  return clm_family_score<Phi3F16, Phi3Family>("b2t_clm_phi3_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                               tok_logp_out, ws, ws_bytes, stream, phi3);
}

extern "C" int b2t_clm_phi3_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, const int32_t* ids_host,
                                           const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                           long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<Phi3F16, Phi3Family>("b2t_clm_phi3_score_tree_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                    tok_logp_out, n_nodes_out, ws, ws_bytes, stream, phi3);
}

extern "C" int b2t_clm_phi3_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, b2t_clm_cache_t* cache,
                                                  int update, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                  float* scores_out, float* tok_logp_out, long long* n_rows_out, int* n_reused_out,
                                                  void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<Phi3F16, Phi3Family>("b2t_clm_phi3_score_tree_cached_f16", "b2t_clm_phi3_score_tree_f16",
                                                           model, cache, update, ids_host, seq_off_host, n_seq, scores_out,
                                                           tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, stream, phi3);
}

extern "C" int b2t_clm_phi3_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, const int32_t* ids_host,
                                       const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                       size_t ws_bytes, void* stream) {
  return clm_family_score<Phi3Bf16, Phi3Family>("b2t_clm_phi3_score_bf16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                tok_logp_out, ws, ws_bytes, stream, phi3);
}

extern "C" int b2t_clm_phi3_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_phi3_t* phi3, const int32_t* ids_host,
                                            const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                            long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<Phi3Bf16, Phi3Family>("b2t_clm_phi3_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                     scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, phi3);
}
