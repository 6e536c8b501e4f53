// causal_lm_gpt2.hip — the scoring forward of causal_lm.hip for GPT-2 (HF GPT2LMHeadModel: distilgpt2, gpt2, -medium, -large,
// -xl): b2t_clm_gpt2_score_f16 over packed sequences, b2t_clm_gpt2_score_tree_f16 over the shared-prefix token tree and
// b2t_clm_gpt2_score_tree_cached_f16 behind a context cache.  Behind the loader (Conv1D weights transposed, c_attn split into
// q | k | v rows, wpe behind two zero rows: llm_rescore.gpt2_device_layout) GPT-2 is the pre-LN OPT forward -- LayerNorm with
// eps 1e-5, learned positions, biased projections, q scaled by head_dim^-0.5, a tied head -- with one difference in
// arithmetic: the MLP activation is gelu_new where OPT has ReLU.
//
// Numerics contract: causal_lm.hip's with "ReLU" replaced by
//   gelu_new(v) = 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))),  v = the fc1 GEMM's fp32 accumulator + bias,
// all in fp32, then the one rounding to fp16.  Rounded to fp16 once each: the LayerNorm outputs, q (after bias and
// head_dim^-0.5), k, v, P per 32-key block, the attention output and gelu_new(fc1).  The tanh is 1 - 2 / (exp(2u) + 1), which
// saturates to +-1 without inf / inf: a pre-activation far on the positive side gives v, far on the negative side -0.0 or 0.
// The activation is the fc1 GEMM's epilogue EP_GELU (clm_gemm.h), elementwise on a thread's own accumulators, so a row's
// result depends on that row alone and on neither the tile nor the batch: flat, tree and cached calls are bit-identical.
//
// This unit instantiates that one epilogue in fp16, on both tiles, and nothing else: the forward is clm_forward and the entry
// points' bodies are every family's (clm_internal.h) under OptFamily and a policy with this unit's fc1 launcher, which goes
// through the one tile rule (launch_gemm of causal_lm.hip).  The model is b2t_clm_t, the cache b2t_clm_cache_t, and the sizes
// are the OPT size functions'.
#include "clm_gemm.h"

namespace b2t {
namespace {

int gpt2_fc1(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_GELU>); }

// the policy of OptFamily (clm_internal.h) with gelu_new in the fc1 GEMM's epilogue
struct Gpt2Policy {
  using E = _Float16;
  static constexpr ClmGemmLaunch fc1 = &gpt2_fc1;
};

}  // namespace

int clm_gemm_gelu(const ClmGemm& g, hipStream_t s) { return gpt2_fc1(g, s); }   // GPT-NeoX's gelu_fast / gelu_new is this one

}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_gpt2_score_f16(const b2t_clm_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                      float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<Gpt2Policy, OptFamily>("b2t_clm_gpt2_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                 tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_gpt2_score_tree_f16(const b2t_clm_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                           float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                           size_t ws_bytes, void* stream) {
  return clm_family_score_tree<Gpt2Policy, OptFamily>("b2t_clm_gpt2_score_tree_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                      tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_gpt2_score_tree_cached_f16(const b2t_clm_t* model, b2t_clm_cache_t* cache, int update,
                                                  const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                  float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                  int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<Gpt2Policy, OptFamily>("b2t_clm_gpt2_score_tree_cached_f16", "b2t_clm_gpt2_score_tree_f16", model,
                                                             cache, update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                             n_rows_out, n_reused_out, ws, ws_bytes, stream);
}
