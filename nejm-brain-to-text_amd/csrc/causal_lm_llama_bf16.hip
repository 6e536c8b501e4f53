// causal_lm_llama_bf16.hip — the Llama-family scoring forward of causal_lm_llama.hip in bfloat16, the format Llama-3, Mistral
// and Qwen2 are trained and published in: b2t_clm_llama_score_bf16 over packed sequences and b2t_clm_llama_score_tree_bf16
// over the shared-prefix token tree.  The forward, the entry points' bodies and every kernel are the fp16 path's templates
// (clm_llama.h, clm_gemm.h, clm_attn.h) instantiated for __bf16; this unit holds the bf16 launches of the Llama policy
// (LlamaShared<__bf16>) and with them all bf16 instantiations:
// the GEMM with the epilogues EP_ROPE, EP_SWIGLU, EP_RESID and EP_HEAD on both tiles, the flat and the tree attention kernel
// for head dims 64 and 128, embed and RMSNorm.  No fp16 unit instantiates a bf16 kernel.
//
// Numerics contract: causal_lm_llama.hip's with "fp16" read as "bf16".  Weights are bf16; GEMM and attention operands are bf16,
// accumulation fp32 (v_mfma_f32_32x32x16_bf16, the shape, lane layout and rate of the f16 instruction); the residual stream
// (the bf16 embedding row widened), the RMSNorm statistics, the rotation (the same fp32 cos / sin table), softmax /
// log-softmax and the sums are fp32; rounded to bf16, once each and to nearest even: the RMSNorm output, q (after bias,
// rotation and head_dim^-0.5), k (after bias and rotation), v, the probabilities per 32-key block as the P.V operand, the
// attention output and silu(gate) * up.  A row's arithmetic order depends only on that row: a sequence scores the same alone
// or in a batch, and the tree call is bit-identical to the flat call.  What bf16 buys is range: 8 exponent bits, so no weight
// or activation of a bf16 checkpoint overflows or goes subnormal on the way in; what it costs is 3 bits of mantissa.
//
// Elements are 2 bytes either way, so the workspace sizes are b2t_clm_llama_ws_bytes / b2t_clm_llama_tree_ws_bytes, the weight
// layout is the fp16 one (llm_rescore.llama_device_layout with dtype=torch.bfloat16) and the tile rule is launch_gemm's
// (causal_lm.hip), applied to bf16 as to fp16.  The context cache behind bf16 is not built yet.
#include "clm_attn.h"
#include "clm_llama.h"

namespace b2t {

// LlamaShared<__bf16> (clm_llama.h): the launches every family's bf16 policy shares
template <> int LlamaShared<__bf16>::gemm_rope(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE, __bf16>);
}
template <> int LlamaShared<__bf16>::gemm_swiglu(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU, __bf16>);
}
template <> int LlamaShared<__bf16>::gemm_resid(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_RESID, __bf16>);
}
template <> int LlamaShared<__bf16>::gemm_head(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP_HEAD, __bf16>);
}
template <> int LlamaShared<__bf16>::embed(const int* ids, const E* et, float* resid, int d, long long rows, hipStream_t s) {
  hipLaunchKernelGGL(clm_llama_embed_kernel<E>, dim3((unsigned)rows), dim3(256), 0, s, ids, et, resid, d);
  B2T_CHECK_LAUNCH("clm_llama_embed_kernel");
  return 0;
}
template <> int LlamaShared<__bf16>::rmsnorm(const float* x, const int* rowmap, long long n, const E* w, float eps, E* out, int d,
                                               hipStream_t s) {
  hipLaunchKernelGGL(clm_llama_rmsnorm_kernel<E>, dim3((unsigned)rup(n, ROWPAD)), dim3(256), 0, s, x, rowmap, (int)n, w, eps, out, d);
  B2T_CHECK_LAUNCH("clm_llama_rmsnorm_kernel");
  return 0;
}
template <> int LlamaShared<__bf16>::attn(const E* qkv, E* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  const dim3 grid(n_seq, Hq);
  if (hd == 64) hipLaunchKernelGGL((clm_attn_kernel<64, E>), grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);
  else hipLaunchKernelGGL((clm_attn_kernel<128, E>), grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);   // 64 or 128: clm_llama_check_model
  B2T_CHECK_LAUNCH("clm_attn_kernel");
  return 0;
}
template <> int LlamaShared<__bf16>::attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start,
                                                 int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  const dim3 grid(n_seq, Hq);
  if (hd == 64) hipLaunchKernelGGL((clm_attn_tree_kernel<64, E>), grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv);
  else hipLaunchKernelGGL((clm_attn_tree_kernel<128, E>), grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv);
  B2T_CHECK_LAUNCH("clm_attn_tree_kernel");
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_llama_score_bf16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                        int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes,
                                        void* stream) {
  return clm_family_score<LlamaPolicy<__bf16>, LlamaFamily>("b2t_clm_llama_score_bf16", model, ids_host, seq_off_host, n_seq,
                                                            scores_out, tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_llama_score_tree_bf16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                             int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                             size_t ws_bytes, void* stream) {
  return clm_family_score_tree<LlamaPolicy<__bf16>, LlamaFamily>("b2t_clm_llama_score_tree_bf16", model, ids_host, seq_off_host,
                                                                 n_seq, scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes,
                                                                 stream);
}
