// causal_lm_qwen3.hip — the Llama-family scoring forward of causal_lm_llama.hip for Qwen3 (HF Qwen3ForCausalLM), in fp16 and
// bf16: b2t_clm_qwen3_score_f16 / _bf16 over packed sequences, b2t_clm_qwen3_score_tree_f16 / _bf16 over the shared-prefix token
// tree and b2t_clm_qwen3_score_tree_cached_f16 behind a context cache.  Qwen3 differs from the Llama forward in one place: an
// RMSNorm over the head dimension of every q head and every k head (weights [hd] per layer, the model's rms_eps) between the
// projection and the rotation; it has no q / k / v biases.
//
// Numerics contract: causal_lm_llama.hip's (causal_lm_llama_bf16.hip's for bf16) with one insertion.  For each q head and each
// k head of a row, on the fp32 accumulator of the QKV GEMM: y[c] = x[c] * rsqrt(mean_c(x[c]^2) + rms_eps) * w[c], w widened
// from the element type, all in fp32; then the rotation, then (q only) head_dim^-0.5, then the one rounding to the element
// type.  v is untouched.  Nothing is rounded between the GEMM and that rounding, and there is no separate pass over qkv: the
// norm is the QKV GEMM's epilogue EP_QKNORM_ROPE (clm_gemm.h), whose per-row sum of squares is a butterfly inside the wave for
// head dim 64 and an exchange of two partial sums through LDS, added lower half first, for head dim 128 -- so the bits depend
// neither on the tile nor on the batch, and tree, cached and flat calls stay bit-identical.  K rows are cached after norm and
// rotation.
//
// This unit instantiates that one epilogue, on both tiles and for both element types, and nothing else: the forward is
// llama_forward (clm_llama.h) under a policy with qk_norm set, every other kernel is reached through LlamaShared<E>, the
// launches causal_lm_llama.hip and causal_lm_llama_bf16.hip define, the three entry-point bodies are clm_internal.h's under
// LlamaFamily, and the workspace and cache sizes are the Llama size functions'.  For head dim 128 the norm weights are
// stored in the order of the q / k rows they scale (llm_rescore.head_dim_perm); the mean of squares does not notice.
#include "clm_llama.h"

namespace b2t {
namespace {

// The Qwen3 policy of the forward for element type El: the Llama policy's launches, and the QKV GEMM with the norm in front
// of the rotation, through the one tile rule.
template <class El>
struct Qwen3Policy : LlamaShared<El> {
  static constexpr bool qk_norm = true;
  static int gemm_rope(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_QKNORM_ROPE, El>); }
};
using Qwen3F16 = Qwen3Policy<_Float16>;
using Qwen3Bf16 = Qwen3Policy<__bf16>;

}  // namespace

int clm_qknorm_check(const char* who, const b2t_clm_llama_t& m, const b2t_clm_qknorm_t* qkn) {
  B2T_REQUIRE(m.n_layers == 0 || qkn, "%s: null qk_norm_host", who);
  for (int l = 0; l < m.n_layers; ++l) {
    B2T_REQUIRE(qkn[l].q_norm_w && qkn[l].k_norm_w, "%s: null q / k norm weight in layer %d", who, l);
    B2T_REQUIRE(!m.layers_host[l].qkv_b, "%s: layer %d has q / k / v biases (qkv_b), which Qwen3 does not", who, l);
  }
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_qwen3_score_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                       const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                       float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<Qwen3F16, LlamaFamily>("b2t_clm_qwen3_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                 tok_logp_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_qwen3_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                            const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                            float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                            void* stream) {
  return clm_family_score_tree<Qwen3F16, LlamaFamily>("b2t_clm_qwen3_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                      scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_qwen3_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                                   b2t_clm_cache_t* cache, int update, const int32_t* ids_host,
                                                   const int32_t* seq_off_host, int n_seq, float* scores_out,
                                                   float* tok_logp_out, long long* n_rows_out, int* n_reused_out, void* ws,
                                                   size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<Qwen3F16, LlamaFamily>("b2t_clm_qwen3_score_tree_cached_f16", "b2t_clm_qwen3_score_tree_f16",
                                                             model, cache, update, ids_host, seq_off_host, n_seq, scores_out,
                                                             tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, stream,
                                                             qk_norm_host);
}

extern "C" int b2t_clm_qwen3_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                        const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                        float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<Qwen3Bf16, LlamaFamily>("b2t_clm_qwen3_score_bf16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                  tok_logp_out, ws, ws_bytes, stream, qk_norm_host);
}

extern "C" int b2t_clm_qwen3_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                             const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                             float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                             void* stream) {
  return clm_family_score_tree<Qwen3Bf16, LlamaFamily>("b2t_clm_qwen3_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                       scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, qk_norm_host);
}
