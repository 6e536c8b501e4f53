// causal_lm_olmo2.hip — the scoring forward of causal_lm_llama.hip for OLMo-2 (HF Olmo2ForCausalLM; 1B, 7B, 13B, 32B), in fp16
// and bf16: b2t_clm_olmo2_score_f16 / _bf16 over packed sequences, b2t_clm_olmo2_score_tree_f16 / _bf16 over the shared-prefix
// token tree and b2t_clm_olmo2_score_tree_cached_f16 behind a context cache.  OLMo-2 has the Llama family's rotary positions,
// grouped-query attention, SwiGLU MLP and head, and differs from its forward in two places, neither of which a GEMM epilogue
// of clm_gemm.h can hold because each needs a whole output row:
//   - q and k are RMSNormed over the whole projection row, all heads together (one statistic for the Hq hd columns of q, one
//     for the Hkv hd columns of k; weights [Hq hd] and [Hkv hd]), between the projection and the rotation -- a q row spans every
//     column tile of the QKV GEMM;
//   - the layer is not pre-norm: there is no input norm, and the o_proj and the down output are RMSNormed over d
//     (post_attention_layernorm, post_feedforward_layernorm) before they are added to the residual:
//       x = x + RMSNorm(attn(x) Wo^T);  x = x + RMSNorm(mlp(x)).
// It has no q / k / v biases.  After the last layer: the final RMSNorm (model.norm), then the head.
//
// Numerics contract (what the fp64 restatement ref_logp_olmo2 of tests/test_clm_olmo2_host.py rounds), E = fp16 or bf16:
//   - weights, GEMM operands and attention operands are E; accumulation is fp32;
//   - the residual stream (which starts as the embedding row widened), all four RMSNorm statistics of a layer, the rotation
//     (cos / sin from the Llama family's fp32 table), softmax / log-softmax and the sums are fp32;
//   - rounded to E, once each: the residual as a GEMM's A operand (layer 0's is the embedding row itself, exact in E); q after
//     norm, rotation and the factor head_dim^-0.5; k after norm and rotation; v; the attention's probabilities per 32-key block
//     as the P.V operand; the attention output; silu(gate) * up; the final norm's output;
//   - the o_proj and down outputs are never rounded: the GEMM stores its fp32 accumulator, the post-norm reads it, and
//     resid += t * rsqrt(mean(t^2) + eps) * w happens in fp32.
//   Every statistic is a strided loop of 256 threads and block_sum256 over one row, so a row's bits depend only on that row:
//   flat, tree and cached calls are byte-identical, a sequence scores the same alone or in a batch, and B2T_CLM_GEMM_256 /
//   B2T_CLM_TRUNK_ATTN do not change the bits.  K rows are cached after norm and rotation, in the Llama cache layout.
//
// Kernels per layer: QKV GEMM (EP_QKV_F32: q | k columns as fp32 accumulators into the scratch region, v rounded into qkv) ->
// clm_olmo2_qknorm_rope_kernel (the two norms, the rotation, q's scale, one rounding, into qkv in front of v) -> causal GQA
// attention (the three launchers of the Llama forward) -> o_proj GEMM (EP_F32 into the scratch region) ->
// clm_olmo2_postnorm_add_kernel (residual += norm; next operand) -> gate / up GEMM (EP_SWIGLU) -> down GEMM (EP_F32) ->
// clm_olmo2_postnorm_add_kernel.  The rotation sits in a kernel that sees whole heads, so q / k rows and the norm weights stay
// in checkpoint order (no head_dim_perm); gate / up rows are interleaved as for Llama.
//
// This unit instantiates the two epilogues (on both tiles) and the two kernels, in both element types, and nothing else:
// every other kernel is reached through LlamaShared<E>, the three entry-point bodies and the size rules are clm_internal.h's under
// Olmo2Family.  The workspace is the Llama layout plus one fp32 region [padded rows][(Hq + Hkv) hd] behind it (olmo2_layout,
// clm_olmo2.h); the cache's size is the Llama family's.
#include "clm_olmo2.h"

namespace b2t {
namespace {

template <class El>
struct Olmo2Policy : LlamaShared<El>, Olmo2Ops<El> {
  static int gemm_qkv(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_QKV_F32, El>); }
  static int gemm_f32(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_F32, El>); }
};
using Olmo2F16 = Olmo2Policy<_Float16>;
using Olmo2Bf16 = Olmo2Policy<__bf16>;

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_olmo2_ws_bytes(const b2t_clm_llama_t* model, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<Olmo2Family>(model, n_tokens, n_seq);
}

extern "C" size_t b2t_clm_olmo2_tree_ws_bytes(const b2t_clm_llama_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<Olmo2Family>(model, n_nodes, n_tokens, n_seq);
}

extern "C" size_t b2t_clm_olmo2_cache_kv_bytes(const b2t_clm_llama_t* model, int cap) {
  return clm_family_cache_kv_bytes<Olmo2Family>(model, cap);
}

extern "C" size_t b2t_clm_olmo2_tree_cached_ws_bytes(const b2t_clm_llama_t* model, long long n_rows, long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<Olmo2Family>(model, n_rows, n_tokens, n_seq);
}

extern "C" int b2t_clm_olmo2_score_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                       const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                       float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<Olmo2F16, Olmo2Family>("b2t_clm_olmo2_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                 tok_logp_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_olmo2_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                            const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                            float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                            void* stream) {
  return clm_family_score_tree<Olmo2F16, Olmo2Family>("b2t_clm_olmo2_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                      scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_olmo2_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                                   b2t_clm_cache_t* cache, int update, const int32_t* ids_host,
                                                   const int32_t* seq_off_host, int n_seq, float* scores_out,
                                                   float* tok_logp_out, long long* n_rows_out, int* n_reused_out, void* ws,
                                                   size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<Olmo2F16, Olmo2Family>("b2t_clm_olmo2_score_tree_cached_f16", "b2t_clm_olmo2_score_tree_f16",
                                                             model, cache, update, ids_host, seq_off_host, n_seq, scores_out,
                                                             tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, stream,
                                                             qk_norm_host);
}

extern "C" int b2t_clm_olmo2_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                        const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                        float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<Olmo2Bf16, Olmo2Family>("b2t_clm_olmo2_score_bf16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                  tok_logp_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_olmo2_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                             const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                             float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                             void* stream) {
  return clm_family_score_tree<Olmo2Bf16, Olmo2Family>("b2t_clm_olmo2_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                       scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, qk_norm_host);
}
