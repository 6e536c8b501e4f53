// causal_lm_gemma2.hip — the scoring forward of causal_lm_llama.hip for Gemma-2 (HF Gemma2ForCausalLM; 2b, 9b, 27b), in fp16 and
// bf16: b2t_clm_gemma2_score_f16 / _bf16 over packed sequences, b2t_clm_gemma2_score_tree_f16 / _bf16 over the shared-prefix token
// tree and b2t_clm_gemma2_score_tree_cached_f16 behind a context cache.  Gemma-2 has the Llama family's rotary positions (default
// rope over the whole head) and grouped-query attention, and differs from its forward in this:
//   - the head dim is a number of its own (256 in the 2b and 9b models, 128 in the 27b): Hq hd != d in all three, so the QKV
//     GEMM has N = (Hq + 2 Hkv) hd, the o_proj K = Hq hd, and the attention output is Hq hd wide;
//   - q is scaled by query_pre_attn_scalar^-0.5, and the scores are soft-capped inside the attention, s = c_a tanh(s / c_a), before
//     the mask and the softmax; the logits are soft-capped, c_f tanh(logit / c_f), in front of the log-softmax;
//   - a layer has four RMSNorms, pre and post on both branches, each multiplying by (1 + w):
//       x += RMSNorm1p(attn(RMSNorm1p(x; input_layernorm)) Wo^T; post_attention_layernorm)
//       x += RMSNorm1p(mlp(RMSNorm1p(x; pre_feedforward_layernorm)); post_feedforward_layernorm)
//     with RMSNorm1p(t; w) = t * rsqrt(mean(t^2) + eps) * (1 + w);
//   - the MLP is GeGLU: (gelu_tanh(h Wg^T) * (h Wu^T)) Wd^T;
//   - the embedding row is multiplied by sqrt(d), and the head is tied to the embedding.
// Sliding-window layers are full causal attention within the window; the loader caps max_pos at the window.  No biases.
//
// Numerics contract (what the fp64 restatement ref_logp_gemma2 of tests/test_clm_gemma2_host.py rounds), E = fp16 or bf16:
//   - weights, GEMM operands and attention operands are E; accumulation is fp32;
//   - the residual stream, every norm statistic, the 1 + w (formed in fp32 from the E weight, never stored rounded), the rotation
//     (cos / sin from the Llama family's fp32 table), both tanh caps, softmax / log-softmax and the sums are fp32;
//   - the embedding's factor is sqrt(d) rounded to E once on the host (what HF does in dtype E) and widened; the product is
//     fp32 and the residual is not rounded;
//   - rounded to E, once each: the two pre-norm outputs and the final norm's output; q after rotation and scale; k after
//     rotation; v; the attention's probabilities per 32-key block as the P.V operand; the attention output; gelu_tanh(gate) * up,
//     formed from the two fp32 accumulators;
//   - the o_proj and down outputs are never rounded: the GEMM stores its fp32 accumulator (EP_F32), the post-norm reads it, and
//     resid += t * rsqrt(mean(t^2) + eps) * (1 + w) happens in fp32;
//   - tanh(u) is written 1 - 2 / (exp(2u) + 1), like gelu_new's: a saturated argument yields +-1, never inf / inf;
//   - a cap of 0 in the descriptor means off: that tanh is not applied.
//   Every statistic is a strided loop of 256 threads and block_sum256 over one row and the cap is per element, so a row's bits
//   depend only on that row: flat, tree and cached calls are byte-identical, a sequence scores the same alone or in a batch, and
//   B2T_CLM_GEMM_256 / B2T_CLM_TRUNK_ATTN do not change the bits.  K rows are cached after the rotation, in the Llama cache layout
//   with the real head dim.
//
// Kernels per layer: QKV GEMM (EP_ROPE, the Llama family's, with hd = 128 or 256 and q's scale) -> causal GQA attention with the
// cap (clm_attn_cap_kernel / clm_attn_tree_cap_kernel of clm_attn.h; the cached call's clm_attn_tree_cached_cap_kernel /
// clm_attn_trunk_cap_kernel behind clm_launch_attn_cached of causal_lm_cache.hip, which hands head dim 256 and every capped call
// to clm_launch_attn_cached_cap below; all instantiated here) -> o_proj GEMM (EP_F32 into the fp32 region) -> clm_gemma2_postnorm_add_kernel
// (residual += post-norm; then the pre-feed-forward norm into the next operand) -> gate / up GEMM (EP_GEGLU) -> down GEMM (EP_F32)
// -> clm_gemma2_postnorm_add_kernel (residual += post-norm; then the next layer's input norm).  In front of layer 0:
// clm_gemma2_embed_kernel and clm_gemma2_rmsnorm_kernel; after the last: clm_gemma2_rmsnorm_kernel on the head rows and the fused
// head with the cap (EP_HEAD_CAP; EP_HEAD where the cap is off).  The rotation is in the QKV GEMM's epilogue, so the loader stores
// each q / k head with stored 32-row block 2j = dims [32j, 32j + 32) and block 2j + 1 = dims [hd / 2 + 32j, hd / 2 + 32j + 32)
// (the Llama order at 128); gate / up rows are interleaved as for Llama.
//
// The flat kernel at head dim 256 stages V through LDS as the tree kernel does (SLAB of clm_attn_flat): with the cap's code the
// global gather of the other head dims would leave no register to spare.  Every attention kernel here compiles without scratch
// (tests/test_clm_gemma2_host.py checks it).
//
// This unit instantiates the three GEMM epilogues (on both tiles), the three kernels of clm_gemma2.h and the capped flat and tree
// attention, in both element types, and the capped cached and trunk attention in fp16; the QKV and the uncapped head GEMM are
// reached through LlamaShared<E>, the three entry-point bodies and the size rules are clm_internal.h's under Gemma2Family.  The
// workspace is gemma2_layout (clm_gemma2.h).
#include "clm_attn.h"
#include "clm_gemma2.h"

namespace b2t {
namespace {

template <class El>
struct Gemma2Policy : LlamaShared<El>, Gemma2Ops<El> {
  using E = El;
  static int gemm_geglu(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_GEGLU, El>); }
  static int gemm_f32(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_F32, El>); }
  static int gemm_head_cap(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_HEAD_CAP, El>); }
  static int attn(const E* qkv, E* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, float cap, hipStream_t s) {
    const dim3 grid(n_seq, Hq);
    if (hd == 256) hipLaunchKernelGGL((clm_attn_cap_kernel<256, E, true>), grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv, cap);
    else hipLaunchKernelGGL((clm_attn_cap_kernel<128, E, false>), grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv, cap);
    B2T_CHECK_LAUNCH("clm_attn_cap_kernel");
    return 0;
  }
  static int attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start, int n_seq, int Hq,
                       int Hkv, int hd, float cap, hipStream_t s) {
    const dim3 grid(n_seq, Hq);
    if (hd == 256)
      hipLaunchKernelGGL((clm_attn_tree_cap_kernel<256, E>), grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv,
                         cap);
    else
      hipLaunchKernelGGL((clm_attn_tree_cap_kernel<128, E>), grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv,
                         cap);
    B2T_CHECK_LAUNCH("clm_attn_tree_cap_kernel");
    return 0;
  }
};
using Gemma2F16 = Gemma2Policy<_Float16>;
using Gemma2Bf16 = Gemma2Policy<__bf16>;

// launch_attn of causal_lm_cache.hip with the `_cap_` kernels: stage B over the whole cached blocks, then the tree walk
template <int D>
int launch_attn_cap(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s) {
  const int Rb = a.trunk ? a.R - a.R % 32 : 0;
  if (Rb > 0) {
    hipLaunchKernelGGL(clm_attn_trunk_cap_kernel<D>, dim3((unsigned)((a.rows + 31) / 32), a.Hq), dim3(64), 0, s, qkv, slab, a.Hkv,
                       (int)a.rows, Rb / 32, a.st_ml, a.st_o, a.cap);
    B2T_CHECK_LAUNCH("clm_attn_trunk_cap_kernel");
  }
  hipLaunchKernelGGL(clm_attn_tree_cached_cap_kernel<D>, dim3(a.n_seq, a.Hq), dim3(256), 0, s, qkv, slab, out, a.soff, a.node,
                     a.own, a.Hkv, a.R, Rb > 0 ? a.st_ml : nullptr, Rb > 0 ? a.st_o : nullptr, Rb / 32, a.cap);
  B2T_CHECK_LAUNCH("clm_attn_tree_cached_cap_kernel");
  return 0;
}

}  // namespace

int clm_launch_attn_cached_cap(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s) {
  B2T_REQUIRE(a.hd == 128 || a.hd == 256, "b2t_clm_gemma2: unsupported head dim %d (128 or 256)", a.hd);
  return a.hd == 256 ? launch_attn_cap<256>(a, qkv, slab, out, s) : launch_attn_cap<128>(a, qkv, slab, out, s);
}

int clm_gemma2_check_model(const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2) {
  const char* pre = "b2t_clm_gemma2";
  B2T_REQUIRE(!m || g2, "b2t_clm_gemma2: null gemma2 descriptor");   // behind the null model, in front of the dimensions
  if (int rc = clm_check_dims(pre, m)) return rc;
  const int hd = g2->head_dim;
  B2T_REQUIRE(hd == 128 || hd == 256, "b2t_clm_gemma2: unsupported head dim %d (128 or 256)", hd);
  if (int rc = clm_check_gqa(pre, *m)) return rc;
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0 && ((long long)m->n_heads * hd) % 64 == 0,
              "b2t_clm_gemma2: d_model %d, ffn_dim %d and n_heads * head_dim %lld must be multiples of 64", m->d_model, m->ffn_dim,
              (long long)m->n_heads * hd);
  if (int rc = clm_check_eps(pre, *m)) return rc;
  B2T_REQUIRE(g2->attn_cap >= 0.f && g2->final_cap >= 0.f, "b2t_clm_gemma2: caps %g and %g must be >= 0 (0: off)",
              (double)g2->attn_cap, (double)g2->final_cap);
  B2T_REQUIRE(g2->q_scale > 0.f && g2->embed_scale > 0.f, "b2t_clm_gemma2: q_scale %g and embed_scale %g must be > 0",
              (double)g2->q_scale, (double)g2->embed_scale);
  if (int rc = clm_check_pointers(pre, *m, g2->layers_host != nullptr)) return rc;
  for (int l = 0; l < m->n_layers; ++l) {
    const b2t_clm_gemma2_layer_t& w2 = g2->layers_host[l];
    if (int rc = clm_check_layer(pre, m->layers_host[l], l, w2.pre_ffn_norm_w && w2.post_ffn_norm_w)) return rc;
    B2T_REQUIRE(!m->layers_host[l].qkv_b, "b2t_clm_gemma2: layer %d has q / k / v biases (qkv_b), which Gemma-2 does not", l);
  }
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_gemma2_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<Gemma2Family>(model, n_tokens, n_seq, g2);
}

extern "C" size_t b2t_clm_gemma2_tree_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, long long n_nodes,
                                               long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<Gemma2Family>(model, n_nodes, n_tokens, n_seq, g2);
}

extern "C" size_t b2t_clm_gemma2_cache_kv_bytes(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, int cap) {
  return clm_family_cache_kv_bytes<Gemma2Family>(model, cap, g2);
}

extern "C" size_t b2t_clm_gemma2_tree_cached_ws_bytes(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, long long n_rows,
                                                      long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<Gemma2Family>(model, n_rows, n_tokens, n_seq, g2);
}

extern "C" int b2t_clm_gemma2_score_f16(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, const int32_t* ids_host,
                                        const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                        size_t ws_bytes, void* stream) {
  return clm_family_score<Gemma2F16, Gemma2Family>("b2t_clm_gemma2_score_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                   tok_logp_out, ws, ws_bytes, stream, g2);
}

extern "C" int b2t_clm_gemma2_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, const int32_t* ids_host,
                                             const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                             long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<Gemma2F16, Gemma2Family>("b2t_clm_gemma2_score_tree_f16", model, ids_host, seq_off_host, n_seq,
                                                        scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, g2);
}

extern "C" int b2t_clm_gemma2_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, b2t_clm_cache_t* cache,
                                                    int update, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                    float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                    int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<Gemma2F16, Gemma2Family>("b2t_clm_gemma2_score_tree_cached_f16",
                                                               "b2t_clm_gemma2_score_tree_f16", model, cache, update, ids_host,
                                                               seq_off_host, n_seq, scores_out, tok_logp_out, n_rows_out,
                                                               n_reused_out, ws, ws_bytes, stream, g2);
}

extern "C" int b2t_clm_gemma2_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, const int32_t* ids_host,
                                         const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
                                         size_t ws_bytes, void* stream) {
  return clm_family_score<Gemma2Bf16, Gemma2Family>("b2t_clm_gemma2_score_bf16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                    tok_logp_out, ws, ws_bytes, stream, g2);
}

extern "C" int b2t_clm_gemma2_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_gemma2_t* g2, const int32_t* ids_host,
                                              const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                              long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree<Gemma2Bf16, Gemma2Family>("b2t_clm_gemma2_score_tree_bf16", model, ids_host, seq_off_host, n_seq,
                                                         scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream, g2);
}
