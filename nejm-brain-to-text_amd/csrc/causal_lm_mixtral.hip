// causal_lm_mixtral.hip — the scoring forward of causal_lm_llama.hip for Mixtral (HF MixtralForCausalLM; 8x7B, 8x22B), in fp16
// and bf16: b2t_clm_mixtral_score_f16 / _bf16 over packed sequences, b2t_clm_mixtral_score_tree_f16 / _bf16 over the
// shared-prefix token tree and b2t_clm_mixtral_score_tree_cached_f16 behind a context cache.  A Mixtral layer is the Llama
// layer -- RMSNorm, rotary positions, grouped-query attention, no biases -- with the dense MLP replaced by n_experts SwiGLU
// MLPs, of which every row runs top_k, chosen and weighted by a router.
//
// The contract (include/b2t.h; what the fp64 restatement ref_logp_mixtral_fmt of tests/test_clm_mixtral_host.py rounds), E = fp16
// or bf16, x = E(RMSNorm(resid; norm2_w)) the row already rounded once, operand of the router and of the experts alike:
//   - router: l[e] = sum_c x[c] Wg[e][c] for e < n_experts, the 16-bit operands widened and accumulated in fp32 by the strided
//     loop and block_sum256 of the norm kernels, so the order depends on the row alone; the logits are never rounded to E;
//   - choice: top_k experts by repeated argmax with a strict `>`, ties to the lower index; the ids are in [0, n_experts)
//     whatever the logits hold, NaN and Inf included: a NaN then shows in the score, never in an address;
//   - weights: w[j] = exp(l[e_j] - l[e_0]) / sum_{i < top_k} exp(l[e_i] - l[e_0]) in fp32, j in order of choice (HF's
//     softmax-then-renormalise with the full sum cancelled); not rounded to E;
//   - experts: h_e = E(silu(x . gate_e) * (x . up_e)), exactly EP_SWIGLU: both fp32 accumulators, one rounding;
//     y_e = h_e . down_e with the fp32 accumulator unrounded (EP_F32);
//   - combine: resid[r] += ((w[0] y_{e_0} + w[1] y_{e_1}) + ...) in fp32, in order of choice, one thread per element, no atomics;
//   - everything else is causal_lm_llama.hip's contract.  Every output element is computed in an order that depends only on its
//     own row: a sequence scores the same alone or in any batch, flat, tree and cached calls are bit-identical, and
//     B2T_CLM_GEMM_256 does not change a bit.
// Limits: 1 <= n_experts <= 64, 1 <= top_k <= min(8, n_experts), ffn_dim % 64 == 0, head dim 64 or 128.
//
// Kernels of a layer's MLP (clm_moe.h), behind the Llama layer's attention half and its second RMSNorm: clm_moe_route_kernel
// (one workgroup per row: logits, choice, weights) -> clm_moe_plan_kernel (one workgroup: rows per expert, segment starts as a
// prefix sum of round_up(count, 256), the slot of every (row, choice) in row order inside its expert; no atomics) ->
// clm_moe_gather_kernel (the sorted operand, zeros in the padding) -> the grouped gate / up GEMM (EP_SWIGLU) -> the grouped down
// GEMM (EP_F32) -> clm_moe_combine_kernel.  The grouped GEMM is the tile of clm_gemm.h with GROUPED set (clm_gemm_grouped_kernel):
// a tile takes its expert's matrix from blk_expert[m0 / 128] and returns where no expert owns the block.  The host knows every
// size before the first launch -- S = round_up(rows * top_k, 256) + 256 * n_experts sorted rows always suffice -- and never
// reads the routing back; both tiles are served through the one tile rule launch_gemm, on a grid sized for S rows.
//
// This unit instantiates the two grouped GEMMs (on both tiles) and the kernels of clm_moe.h, in both element types, and nothing
// else: every other kernel is reached through LlamaShared<E>, the three entry-point bodies and the size rules are clm_internal.h's
// under MixtralFamily.  The workspace is the Llama layout with an empty hbuf plus one region behind it (mixtral_layout,
// clm_moe.h); the cache's size is the Llama family's, which is why this unit exports no cache_kv_bytes.
#include "clm_moe.h"

namespace b2t {
namespace {

template <class El>
struct MixtralPolicy : LlamaShared<El>, MoeOps<El> {
  static constexpr bool qk_norm = false;
  static int gemm_experts_swiglu(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU, El, true>); }
  static int gemm_experts_f32(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_F32, El, true>); }
};
using MixtralF16 = MixtralPolicy<_Float16>;
using MixtralBf16 = MixtralPolicy<__bf16>;

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_mixtral_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<MixtralFamily>(model, n_tokens, n_seq, moe);
}

extern "C" size_t b2t_clm_mixtral_tree_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, long long n_nodes,
                                                long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<MixtralFamily>(model, n_nodes, n_tokens, n_seq, moe);
}

extern "C" size_t b2t_clm_mixtral_tree_cached_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, long long n_rows,
                                                       long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<MixtralFamily>(model, n_rows, n_tokens, n_seq, moe);
}

extern "C" int b2t_clm_mixtral_score_f16(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, const int32_t* ids_host,
                                         const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                         size_t ws_bytes, void* stream) {
  return clm_family_score<MixtralF16, MixtralFamily>("b2t_clm_mixtral_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                     tok_logp_out, ws, ws_bytes, stream, moe);
}

extern "C" int b2t_clm_mixtral_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, const int32_t* ids_host,
                                              const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                              long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<MixtralF16, MixtralFamily>("b2t_clm_mixtral_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                          scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, moe);
}

extern "C" int b2t_clm_mixtral_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, b2t_clm_cache_t* cache,
                                                     int update, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                     float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                     int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<MixtralF16, MixtralFamily>("b2t_clm_mixtral_score_tree_cached_f16",
                                                                 "b2t_clm_mixtral_score_tree_f16", model, cache, update, ids_host,
                                                                 seq_off_host, n_seq, scores_out, tok_logp_out, n_rows_out,
                                                                 n_reused_out, ws, ws_bytes, stream, moe);
}

extern "C" int b2t_clm_mixtral_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, const int32_t* ids_host,
                                          const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                          size_t ws_bytes, void* stream) {
  return clm_family_score<MixtralBf16, MixtralFamily>("b2t_clm_mixtral_score_bf16", model, ids_host, seq_off_host, n_seq,
                                                      scores_out, tok_logp_out, ws, ws_bytes, stream, moe);
}

extern "C" int b2t_clm_mixtral_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_moe_t* moe, const int32_t* ids_host,
                                               const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                               long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<MixtralBf16, MixtralFamily>("b2t_clm_mixtral_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                           scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, moe);
}
