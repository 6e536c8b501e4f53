// causal_lm_gptoss.hip — the scoring forward of causal_lm_llama.hip for gpt-oss (HF GptOssForCausalLM; gpt-oss-20b, 120b), in fp16
// and bf16: b2t_clm_gptoss_score_f16 / _bf16 over packed sequences and b2t_clm_gptoss_score_tree_f16 / _bf16 over the shared-prefix
// token tree.  gpt-oss has the Llama family's pre-norm RMSNorm layer, grouped-query attention, rotary positions over the whole
// head, embedding and untied head, and differs from its forward in this:
//   - the head dim is a number of its own (64 heads of 64 dims against d = 2880), as in Gemma-2: the QKV GEMM has N = (Hq + 2 Hkv)
//     hd, the o_proj K = Hq hd, and the attention output is Hq hd wide;
//   - q, k, v and o_proj have biases; the rotary table carries YaRN's attention factor (the loader multiplies it in, as for Phi-3);
//   - every head has a learned sink, one more logit in the softmax's denominator;
//   - every other layer attends over a sliding window of 128 keys, which binds (a context plus a candidate is longer), so the
//     window lives in the attention kernel and does not lower max_pos;
//   - the MLP is n_experts routed experts with a router bias, per-expert gate / up / down biases and the clamped activation
//     (up + 1) * gate * sigmoid(1.702 gate).
//
// The contract (include/b2t.h; what the fp64 restatement ref_logp_gptoss of tests/test_clm_gptoss_host.py rounds), E = fp16 or
// bf16: causal_lm_llama.hip's, with
//   - attention: the state of a query at head h starts at (m, l, o) = (sinks[h], 1, 0), the sink in fp32 and compared with the
//     scores of the already-scaled q; with a window W > 0 key j is visible to query i iff i - W < j <= i; the key loop starts at
//     the first 32-key block that holds a visible key of the query block's lowest query and the invisible keys of the blocks
//     that remain are -inf; P is rounded to E per 32-key block as everywhere;
//   - x += E(attn) Wo^T + o_b in fp32 (EP_RESID with a bias, OPT's epilogue);
//   - router: l[e] = b[e] + sum_c h2[c] Wr[e][c], 16-bit operands widened, fp32 sums in an order fixed by the row (below), never
//     rounded; choice by repeated argmax, larger first, lower index among equals, ids always distinct and in range; weights
//     w[j] = exp(l[e_j] - l[e_0]) / sum_i exp(l[e_i] - l[e_0]) in fp32;
//   - experts: g = min(acc_g + b_g, limit), u = clamp(acc_u + b_u, -limit, limit), hs = E((u + 1) g / (1 + exp(-1.702 g))) with one
//     rounding (EP_OSS_GLU); y_e = hs Wd_e^T + b_d unrounded (EP_F32_BIAS); combine in order of choice, no atomics.
//   Every output element is computed in an order that depends only on its own row: tree and flat calls are byte-identical, a
//   sequence scores the same alone or in a batch, and B2T_CLM_GEMM_256 does not change a bit.
// Limits: head dim 64, 1 <= n_experts <= 128, 1 <= top_k <= min(8, n_experts), d_model % 64 == 0, ffn_dim % 64 == 0.
//
// Kernels per layer: RMSNorm -> QKV GEMM (EP_ROPE with the bias, the Llama family's) -> clm_attn_sink_kernel /
// clm_attn_tree_sink_kernel (clm_attn.h with SINK and WIN set) -> o_proj GEMM (EP_RESID with the bias) -> RMSNorm ->
// clm_gptoss_route_kernel (one workgroup per row; a wave per expert in turn, one barrier) -> clm_moe_plan_kernel ->
// clm_moe_gather_kernel -> the grouped gate / up GEMM (EP_OSS_GLU) -> the grouped down GEMM (EP_F32_BIAS) ->
// clm_moe_combine_kernel.  Plan, gather, combine, the region and S = round_up(rows * top_k, 256) + 256 * n_experts are clm_moe.h's.
//
// This unit instantiates the two grouped GEMMs (on both tiles), the router kernel, the plan, gather and combine kernels and the
// two attention kernels (through GptOssOps<E>, clm_gptoss.h), in both element types where they depend on it, and nothing else:
// every other kernel is reached through LlamaShared<E>, the flat and the tree entry-point body and the two size rules are
// clm_internal.h's under GptOssFamily.  There is no cached call: the cached and trunk
// attention kernels have neither sink nor window.
#include "clm_attn.h"
#include "clm_gptoss.h"

namespace b2t {
namespace {

template <class El>
struct GptOssPolicy : LlamaShared<El>, MoeOps<El>, GptOssOps<El> {
  static int gemm_experts_glu(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_OSS_GLU, El, true>); }
  static int gemm_experts_f32b(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_F32_BIAS, El, true>); }
};
using GptOssF16 = GptOssPolicy<_Float16>;
using GptOssBf16 = GptOssPolicy<__bf16>;

}  // namespace

int clm_gptoss_check_model(const b2t_clm_llama_t* m, const b2t_clm_gptoss_t* g) {
  const char* pre = "b2t_clm_gptoss";
  B2T_REQUIRE(!m || g, "b2t_clm_gptoss: null gptoss descriptor");   // behind the null model, in front of the dimensions
  if (int rc = clm_check_dims(pre, m)) return rc;
  B2T_REQUIRE(g->head_dim == OSS_HEAD_DIM, "b2t_clm_gptoss: unsupported head dim %d (%d)", g->head_dim, OSS_HEAD_DIM);
  if (int rc = clm_check_gqa(pre, *m)) return rc;
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0, "b2t_clm_gptoss: d_model %d and ffn_dim %d must be multiples of 64",
              m->d_model, m->ffn_dim);
  if (int rc = clm_check_eps(pre, *m)) return rc;
  B2T_REQUIRE(g->n_experts >= 1 && g->n_experts <= OSS_MAX_EXPERTS, "b2t_clm_gptoss: n_experts %d outside [1, %d]", g->n_experts,
              OSS_MAX_EXPERTS);
  B2T_REQUIRE(g->top_k >= 1 && g->top_k <= MOE_MAX_TOPK && g->top_k <= g->n_experts,
              "b2t_clm_gptoss: top_k %d outside [1, min(%d, n_experts %d)]", g->top_k, MOE_MAX_TOPK, g->n_experts);
  B2T_REQUIRE(g->gate_up_stride >= rup(2LL * m->ffn_dim, ROWPAD) && g->down_stride >= rup(m->d_model, ROWPAD),
              "b2t_clm_gptoss: expert strides %lld / %lld rows below round_up(2 ffn_dim, 256) = %lld / round_up(d_model, 256) = %lld",
              g->gate_up_stride, g->down_stride, rup(2LL * m->ffn_dim, ROWPAD), rup(m->d_model, ROWPAD));
  B2T_REQUIRE(g->swiglu_limit > 0.f, "b2t_clm_gptoss: swiglu_limit %g must be > 0", (double)g->swiglu_limit);
  if (int rc = clm_check_pointers(pre, *m, g->layers_host != nullptr)) return rc;
  for (int l = 0; l < m->n_layers; ++l) {
    const b2t_clm_gptoss_layer_t& w2 = g->layers_host[l];
    if (int rc = clm_check_layer(pre, m->layers_host[l], l,
                                 w2.sinks && w2.o_b && w2.router_w && w2.router_b && w2.gate_up_b && w2.down_b))
      return rc;
    B2T_REQUIRE(m->layers_host[l].qkv_b, "b2t_clm_gptoss: layer %d has no q / k / v biases (qkv_b), which gpt-oss has", l);
    B2T_REQUIRE(w2.window >= 0, "b2t_clm_gptoss: layer %d has window %d < 0 (0: full attention)", l, w2.window);
  }
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_gptoss_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<GptOssFamily>(model, n_tokens, n_seq, oss);
}

extern "C" size_t b2t_clm_gptoss_tree_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, long long n_nodes,
                                               long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<GptOssFamily>(model, n_nodes, n_tokens, n_seq, oss);
}

extern "C" int b2t_clm_gptoss_score_f16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const int32_t* ids_host,
                                        const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                        size_t ws_bytes, void* stream) {
  return clm_family_score<GptOssF16, GptOssFamily>("b2t_clm_gptoss_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                   tok_logp_out, ws, ws_bytes, stream, oss);
}

extern "C" int b2t_clm_gptoss_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const int32_t* ids_host,
                                             const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                             long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<GptOssF16, GptOssFamily>("b2t_clm_gptoss_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                        scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, oss);
}

extern "C" int b2t_clm_gptoss_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const int32_t* ids_host,
                                         const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                         size_t ws_bytes, void* stream) {
  return clm_family_score<GptOssBf16, GptOssFamily>("b2t_clm_gptoss_score_bf16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                    tok_logp_out, ws, ws_bytes, stream, oss);
}

extern "C" int b2t_clm_gptoss_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const int32_t* ids_host,
                                              const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                              long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<GptOssBf16, GptOssFamily>("b2t_clm_gptoss_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                         scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, oss);
}
