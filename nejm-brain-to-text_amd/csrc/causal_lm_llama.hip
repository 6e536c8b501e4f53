// causal_lm_llama.hip — the scoring forward of causal_lm.hip for the Llama family (HF LlamaForCausalLM, MistralForCausalLM,
// Qwen2ForCausalLM): RMSNorm, rotary positions, grouped-query attention, a SwiGLU MLP and an LM head of its own, over packed
// sequences (b2t_clm_llama_score_f16), over the shared-prefix token tree (b2t_clm_llama_score_tree_f16; the plan is
// causal_lm_tree.hip's, and a node's rotary position is its depth) and over that tree behind a context cache
// (b2t_clm_llama_score_tree_cached_f16; the rule, the kernels and the entry point's body are causal_lm_cache.hip's and
// clm_internal.h's: K rows are cached after the rotation, at their absolute positions).
//
// Numerics contract (what the fp64 restatement of tests/test_clm_llama_host.py rounds):
//   - weights are fp16; GEMM operands are fp16, accumulation fp32 (v_mfma_f32_32x32x16_f16);
//   - the residual stream (which starts as the fp16 embedding row widened), the RMSNorm statistics, the rotation, softmax /
//     log-softmax and the per-sequence sums are fp32; cos / sin come from an fp32 table the host builds in double;
//   - rounded to fp16, once each: the RMSNorm output x * rsqrt(mean(x^2) + eps) * w; q, k and v -- q and k after the bias, the
//     rotation and (q) the factor head_dim^-0.5, all applied to the fp32 accumulator; the attention output; silu(gate) * up,
//     formed from the two fp32 accumulators (gate and up are never rounded on their own); and the attention's
//     probabilities exp(s - m) per 32-key block as the P.V operand, exactly as in causal_lm.hip.
//   Every output element is computed by one thread in a fixed order that depends only on its own row, so a sequence's score
//   is bit-identical alone or in any batch, and the tree call is bit-identical to the flat call.
//
// Kernels per layer: RMSNorm -> QKV GEMM with the rotation in its epilogue (EP_ROPE, clm_gemm.h) -> causal GQA attention
// (causal_lm.hip's, causal_lm_tree.hip's and causal_lm_cache.hip's kernels through clm_launch_attn / clm_launch_attn_tree /
// clm_launch_attn_cached: query head h reads K / V head h / (Hq / Hkv); head dim 64 or 128) -> o_proj GEMM into the
// residual -> RMSNorm -> gate / up GEMM with SwiGLU in
// its epilogue (EP_SWIGLU; the [M][2F] intermediate never exists) -> down GEMM into the residual.  Then the final RMSNorm of
// every position but the last of each sequence and causal_lm.hip's fused head (clm_head with W = lm_head) and sums.  The
// list check, the plan, the index arrays and the workspace layout are the OPT paths' (clm_internal.h).
// The two weight layouts the epilogues rely on are made at load time (llm_rescore.py): gate / up rows interleaved in blocks
// of 32, and for head dim 128 the q / k rows of each head in the order [0..31, 64..95, 32..63, 96..127] (q . k is invariant
// under one permutation of both; V and o_proj are untouched).
//
// The forward (llama_forward) and the embed / RMSNorm kernels are templates in clm_llama.h, the bodies of the flat, the tree and
// the cached entry point and the size rules in clm_internal.h, on a per-element-type policy and a family; this unit holds the fp16 launches of
// the Llama policy (LlamaShared<_Float16>: the two GEMM launches of this family through the one tile rule, the OPT paths'
// residual / head GEMMs and attention launchers, embed and RMSNorm), which every other family's fp16 policy shares, and the
// model check.  The same forward in bf16 is causal_lm_llama_bf16.hip; Qwen3's, which norms the q and k heads in the QKV GEMM's
// epilogue, is causal_lm_qwen3.hip.
#include "clm_llama.h"

namespace b2t {

// LlamaShared<_Float16> (clm_llama.h); the attention kernels are causal_lm.hip's and causal_lm_tree.hip's
template <> int LlamaShared<_Float16>::gemm_rope(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE>);
}
template <> int LlamaShared<_Float16>::gemm_swiglu(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU>);
}
template <> int LlamaShared<_Float16>::gemm_resid(const ClmGemm& g, hipStream_t s) { return launch_gemm<EP_RESID>(g, s); }
template <> int LlamaShared<_Float16>::gemm_head(const ClmGemm& g, hipStream_t s) { return launch_gemm<EP_HEAD>(g, s); }
template <> int LlamaShared<_Float16>::embed(const int* ids, const E* et, float* resid, int d, long long rows, hipStream_t s) {
  hipLaunchKernelGGL(clm_llama_embed_kernel<E>, dim3((unsigned)rows), dim3(256), 0, s, ids, et, resid, d);
  B2T_CHECK_LAUNCH("clm_llama_embed_kernel");
  return 0;
}
template <> int LlamaShared<_Float16>::rmsnorm(const float* x, const int* rowmap, long long n, const E* w, float eps, E* out, int d,
                                                 hipStream_t s) {
  hipLaunchKernelGGL(clm_llama_rmsnorm_kernel<E>, dim3((unsigned)rup(n, ROWPAD)), dim3(256), 0, s, x, rowmap, (int)n, w, eps, out, d);
  B2T_CHECK_LAUNCH("clm_llama_rmsnorm_kernel");
  return 0;
}
template <> int LlamaShared<_Float16>::attn(const E* qkv, E* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  return clm_launch_attn(qkv, out, seq_off, n_seq, Hq, Hkv, hd, s);
}
template <> int LlamaShared<_Float16>::attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start,
                                                   int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  return clm_launch_attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, Hq, Hkv, hd, s);
}

int clm_llama_check_model(const b2t_clm_llama_t* m) {
  const char* pre = "b2t_clm_llama";
  if (int rc = clm_check_dims(pre, m)) return rc;
  B2T_REQUIRE(m->d_model % m->n_heads == 0, "b2t_clm_llama: d_model %d is not a multiple of n_heads %d", m->d_model, m->n_heads);
  const int hd = m->d_model / m->n_heads;
  B2T_REQUIRE(hd == 64 || hd == 128, "b2t_clm_llama: unsupported head dim %d (64 or 128)", hd);
  if (int rc = clm_check_gqa(pre, *m)) return rc;
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0, "b2t_clm_llama: d_model %d and ffn_dim %d must be multiples of 64",
              m->d_model, m->ffn_dim);
  if (int rc = clm_check_eps(pre, *m)) return rc;
  if (int rc = clm_check_pointers(pre, *m)) return rc;
  for (int l = 0; l < m->n_layers; ++l)
    if (int rc = clm_check_layer(pre, m->layers_host[l], l)) return rc;
  return 0;
}

}  // namespace b2t

using namespace b2t;
using LlamaF = LlamaPolicy<_Float16>;

extern "C" size_t b2t_clm_llama_ws_bytes(const b2t_clm_llama_t* model, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<LlamaFamily>(model, n_tokens, n_seq);
}

extern "C" int b2t_clm_llama_score_f16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                       int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes,
                                       void* stream) {
  return clm_family_score<LlamaF, LlamaFamily>("b2t_clm_llama_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                               tok_logp_out, ws, ws_bytes, stream);
}

extern "C" size_t b2t_clm_llama_tree_ws_bytes(const b2t_clm_llama_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<LlamaFamily>(model, n_nodes, n_tokens, n_seq);
}

extern "C" int b2t_clm_llama_score_tree_f16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                            int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                            size_t ws_bytes, void* stream) {
  return clm_family_score_tree<LlamaF, LlamaFamily>("b2t_clm_llama_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                    scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" size_t b2t_clm_llama_cache_kv_bytes(const b2t_clm_llama_t* model, int cap) {
  return clm_family_cache_kv_bytes<LlamaFamily>(model, cap);
}

extern "C" size_t b2t_clm_llama_tree_cached_ws_bytes(const b2t_clm_llama_t* model, long long n_rows, long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<LlamaFamily>(model, n_rows, n_tokens, n_seq);
}

extern "C" int b2t_clm_llama_score_tree_cached_f16(const b2t_clm_llama_t* model, b2t_clm_cache_t* cache, int update,
                                                   const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                   float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                   int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<LlamaF, LlamaFamily>("b2t_clm_llama_score_tree_cached_f16", "b2t_clm_llama_score_tree_f16",
                                                           model, cache, update, ids_host, seq_off_host, n_seq, scores_out,
                                                           tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, stream);
}
