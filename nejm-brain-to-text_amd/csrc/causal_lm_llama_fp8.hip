// causal_lm_llama_fp8.hip — the Llama-family forward of causal_lm_llama.hip / causal_lm_qwen3.hip with the four projections of
// every layer kept in block-scaled FP8 in device memory, in fp16 and bf16: b2t_clm_llama_fp8_score_f16 / _bf16 over packed
// sequences, b2t_clm_llama_fp8_score_tree_f16 / _bf16 over the shared-prefix token tree, b2t_clm_llama_fp8_score_tree_cached_f16
// behind a context cache, and b2t_clm_fp8_unpack_f16 / _bf16, which expand packed rows to a dense matrix.
//
// The contract (include/b2t.h) is the dense units', to the byte: the QKV, o, gate | up and down GEMMs read one e4m3fn code a
// weight and one fp32 scale per 32 stored rows and block_k columns where the dense ones read 16-bit weights, expand them in
// registers (fp8_unpack8, clm_gemm.h: exactly the value the loader's dequantise-then-cast stores -- an exact widening, one fp32
// multiplication and one conversion, both rounded to nearest even with subnormals kept) and write the dense tile's uint4s into
// the dense tile's LDS layout; the k loop, its order and the epilogues (EP_ROPE with or without the q / k / v bias,
// EP_QKNORM_ROPE, EP_SWIGLU, EP_RESID) are the dense kernel's code.  Activations are never quantised: this is not an FP8 matrix
// multiplication.  Embedding, norms, attention and the head (dense, 16-bit) are reached through LlamaShared<E>, the forward is
// clm_llama.h's llama_forward and the workspace llama_layout's; both tiles go through launch_gemm's one rule.
//
// A model with its fp8 descriptor is checked by the dense units' clm_llama_check_model (and clm_qknorm_check) on a copy of
// the layer records whose qkv_w / o_w / gate_up_w / down_w point at the codes, after this unit's own refusals: a null
// descriptor, a null pointer inside it, a block_k the tile cannot follow, and a model that also holds dense projections.  The
// forward runs on that copy, so it needs the scales alone.  A null qk_norm_host is Llama / Mistral / Qwen2, an array Qwen3.
//
// This unit instantiates the packed plain GEMM with the four epilogues (on both tiles, in both element types) and the unpack
// kernel in both element types, and nothing else.
#include <vector>

#include "clm_llama.h"

namespace b2t {
namespace {

// The policy of the forward for element type El, QKN: with Qwen3's q / k norm in the QKV epilogue.  The head, the embedding, the
// norm and the attention are LlamaShared<El>'s.
template <class El, bool QKN>
struct LlamaFp8Policy : LlamaShared<El> {
  static constexpr bool qk_norm = QKN;
  static int gemm_rope(const ClmGemm& g, hipStream_t s) {
    return launch_gemm(g, s, &clm_gemm_tiles<QKN ? EP_QKNORM_ROPE : EP_ROPE, El, false, PK_FP8>);
  }
  static int gemm_swiglu(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU, El, false, PK_FP8>); }
  static int gemm_resid(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_RESID, El, false, PK_FP8>); }
};

// what the entry-point bodies of clm_internal.h carry beside the model: the q / k norm array (null: none) and the scales
struct LlamaFp8Arg {
  const b2t_clm_qknorm_t* qkn;
  const b2t_clm_llama_fp8_t* f8;
};

// LlamaFamily on that pair: layout, sizes and the attention are its own; check and forward read the pair
struct LlamaFp8Family : LlamaFamily {
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t* m, const LlamaFp8Arg* x) {
    return LlamaFamily::check<P>(who, m, x->qkn);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const LlamaFp8Arg* x) {
    return llama_forward<P>(m, r, L, base, attn, s, x->qkn, x->f8);
  }
};

// This unit's refusals, and the model the forward runs on: `model` with a copy of its layer records (`layers`, which the caller
// keeps alive) whose four matrices are the codes.  A model the dense check will refuse for its dimensions or for a null layer
// array passes through unchanged, and is refused there.
int fp8_model(const char* who, const b2t_clm_llama_t* model, const b2t_clm_llama_fp8_t* f8, std::vector<b2t_clm_llama_layer_t>& layers,
              b2t_clm_llama_t* out) {
  B2T_REQUIRE(model, "b2t_clm_llama: null model");
  B2T_REQUIRE(f8, "%s: null fp8 descriptor (the projections kept in FP8)", who);
  *out = *model;
  if (model->d_model > 0 && model->ffn_dim > 0 && model->d_model % 64 == 0 && model->ffn_dim % 64 == 0)   // else: the dense check's
    B2T_REQUIRE(f8->block_k > 0 && f8->block_k % 64 == 0 && model->d_model % f8->block_k == 0 && model->ffn_dim % f8->block_k == 0,
                "%s: block_k %d must be a multiple of 64 that divides d_model %d and ffn_dim %d", who, f8->block_k, model->d_model,
                model->ffn_dim);
  if (model->n_layers <= 0 || !model->layers_host) return 0;
  B2T_REQUIRE(f8->layers_host, "%s: null layers_host in the fp8 descriptor", who);
  layers.assign(model->layers_host, model->layers_host + model->n_layers);
  for (int l = 0; l < model->n_layers; ++l) {
    const b2t_clm_llama_fp8_layer_t& p = f8->layers_host[l];
    B2T_REQUIRE(!layers[l].qkv_w && !layers[l].o_w && !layers[l].gate_up_w && !layers[l].down_w,
                "%s: layer %d of the model has qkv_w / o_w / gate_up_w / down_w beside the packed projections; a caller holds one "
                "form, not both", who, l);
    B2T_REQUIRE(p.qkv_q && p.qkv_s && p.o_q && p.o_s && p.gate_up_q && p.gate_up_s && p.down_q && p.down_s,
                "%s: null pointer in layer %d of the fp8 descriptor", who, l);
    layers[l].qkv_w = p.qkv_q;
    layers[l].o_w = p.o_q;
    layers[l].gate_up_w = p.gate_up_q;
    layers[l].down_w = p.down_q;
  }
  out->layers_host = layers.data();
  return 0;
}

template <class El, bool QKN>
int fp8_score_as(const char* who, const b2t_clm_llama_t& m, const LlamaFp8Arg& x, const int32_t* ids_host, const int32_t* seq_off_host,
                 int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<LlamaFp8Policy<El, QKN>, LlamaFp8Family>(who, &m, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                                   ws, ws_bytes, stream, &x);
}
template <class El>
int fp8_score(const char* who, const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qkn, const b2t_clm_llama_fp8_t* f8,
              const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
              size_t ws_bytes, void* stream) {
  std::vector<b2t_clm_llama_layer_t> layers;
  b2t_clm_llama_t m;
  if (int rc = fp8_model(who, model, f8, layers, &m)) return rc;
  const LlamaFp8Arg x{qkn, f8};
  return (qkn ? fp8_score_as<El, true> : fp8_score_as<El, false>)(who, m, x, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                                 ws, ws_bytes, stream);
}

template <class El, bool QKN>
int fp8_score_tree_as(const char* who, const b2t_clm_llama_t& m, const LlamaFp8Arg& x, const int32_t* ids_host,
                      const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                      size_t ws_bytes, void* stream) {
  return clm_family_score_tree<LlamaFp8Policy<El, QKN>, LlamaFp8Family>(who, &m, ids_host, seq_off_host, n_seq, scores_out,
                                                                        tok_logp_out, n_nodes_out, ws, ws_bytes, stream, &x);
}
template <class El>
int fp8_score_tree(const char* who, const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qkn, const b2t_clm_llama_fp8_t* f8,
                   const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                   long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  std::vector<b2t_clm_llama_layer_t> layers;
  b2t_clm_llama_t m;
  if (int rc = fp8_model(who, model, f8, layers, &m)) return rc;
  const LlamaFp8Arg x{qkn, f8};
  return (qkn ? fp8_score_tree_as<El, true> : fp8_score_tree_as<El, false>)(who, m, x, ids_host, seq_off_host, n_seq, scores_out,
                                                                           tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

template <bool QKN>
int fp8_score_tree_cached_as(const char* who, const b2t_clm_llama_t& m, const LlamaFp8Arg& x, b2t_clm_cache_t* cache, int update,
                             const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                             long long* n_rows_out, int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<LlamaFp8Policy<_Float16, QKN>, LlamaFp8Family>(
      who, "b2t_clm_llama_fp8_score_tree_f16", &m, cache, update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out, n_rows_out,
      n_reused_out, ws, ws_bytes, stream, &x);
}

// packed rows to dense ones: a thread expands one piece of eight elements, the GEMM's unit, with the GEMM's function
template <class E>
__global__ __launch_bounds__(256) void clm_fp8_unpack_kernel(const uint2* q, const float* sc, long long pieces, int kp, int bp, int nkb,
                                                             uint4* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // piece i: row i / kp, elements 8 (i % kp) ..; bp pieces a block
  if (i < pieces) out[i] = fp8_unpack8<E>(q[i], sc[((i / kp) >> 5) * nkb + (int)(i % kp) / bp]);
}

template <class E>
int fp8_unpack(const char* who, const void* q, const void* s, long long rows, int K, int block_k, void* out, void* stream) {
  B2T_REQUIRE(rows >= 0 && K > 0 && block_k > 0 && block_k % 64 == 0 && K % block_k == 0,
              "%s: rows %lld, K %d, block_k %d (block_k must be a positive multiple of 64 that divides K)", who, rows, K, block_k);
  if (rows == 0) return 0;
  B2T_REQUIRE(q && s && out, "%s: null argument", who);
  const long long blocks = (rows * (K / 8) + 255) / 256;
  B2T_REQUIRE(rows <= (1LL << 40) / K && blocks <= INT_MAX, "%s: %lld rows of %d elements are too many for one launch", who, rows, K);
  hipLaunchKernelGGL(clm_fp8_unpack_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), static_cast<const uint2*>(q),
                     static_cast<const float*>(s), rows * (K / 8), K / 8, block_k / 8, K / block_k, static_cast<uint4*>(out));
  B2T_CHECK_LAUNCH("clm_fp8_unpack_kernel");
  return 0;
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_llama_fp8_score_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                           const b2t_clm_llama_fp8_t* fp8, const int32_t* ids_host, const int32_t* seq_off_host,
                                           int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return fp8_score<_Float16>("b2t_clm_llama_fp8_score_f16", model, qk_norm_host, fp8, ids_host, seq_off_host, n_seq, scores_out,
                             tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_llama_fp8_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                                const b2t_clm_llama_fp8_t* fp8, const int32_t* ids_host, const int32_t* seq_off_host,
                                                int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                                size_t ws_bytes, void* stream) {
  return fp8_score_tree<_Float16>("b2t_clm_llama_fp8_score_tree_f16", model, qk_norm_host, fp8, ids_host, seq_off_host, n_seq,
                                  scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_llama_fp8_score_tree_cached_f16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                                       const b2t_clm_llama_fp8_t* fp8, b2t_clm_cache_t* cache, int update,
                                                       const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                                       float* scores_out, float* tok_logp_out, long long* n_rows_out,
                                                       int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "b2t_clm_llama_fp8_score_tree_cached_f16";
  std::vector<b2t_clm_llama_layer_t> layers;
  b2t_clm_llama_t m;
  if (int rc = fp8_model(who, model, fp8, layers, &m)) return rc;
  const LlamaFp8Arg x{qk_norm_host, fp8};
  return (qk_norm_host ? fp8_score_tree_cached_as<true> : fp8_score_tree_cached_as<false>)(
      who, m, x, cache, update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out, n_rows_out, n_reused_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_llama_fp8_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                            const b2t_clm_llama_fp8_t* fp8, const int32_t* ids_host, const int32_t* seq_off_host,
                                            int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return fp8_score<__bf16>("b2t_clm_llama_fp8_score_bf16", model, qk_norm_host, fp8, ids_host, seq_off_host, n_seq, scores_out,
                           tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_llama_fp8_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_qknorm_t* qk_norm_host,
                                                 const b2t_clm_llama_fp8_t* fp8, const int32_t* ids_host, const int32_t* seq_off_host,
                                                 int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                                 size_t ws_bytes, void* stream) {
  return fp8_score_tree<__bf16>("b2t_clm_llama_fp8_score_tree_bf16", model, qk_norm_host, fp8, ids_host, seq_off_host, n_seq,
                                scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_fp8_unpack_f16(const void* q, const void* s, long long rows, int K, int block_k, void* out, void* stream) {
  return fp8_unpack<_Float16>("b2t_clm_fp8_unpack_f16", q, s, rows, K, block_k, out, stream);
}

extern "C" int b2t_clm_fp8_unpack_bf16(const void* q, const void* s, long long rows, int K, int block_k, void* out, void* stream) {
  return fp8_unpack<__bf16>("b2t_clm_fp8_unpack_bf16", q, s, rows, K, block_k, out, stream);
}
