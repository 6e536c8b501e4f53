// causal_lm_gptoss_mx.hip — causal_lm_gptoss.hip's forward with the experts kept in MXFP4 in device memory, in fp16 and bf16:
// b2t_clm_gptoss_mx_score_f16 / _bf16 over packed sequences, b2t_clm_gptoss_mx_score_tree_f16 / _bf16 over the shared-prefix token
// tree, and b2t_clm_mxfp4_unpack_f16 / _bf16, which expand packed rows to a dense matrix.
//
// The contract (include/b2t.h) is causal_lm_gptoss.hip's, to the byte: the two grouped GEMMs read the nibbles and the scale bytes
// where the dense ones read 16-bit weights, expand them in registers (mxfp4_unpack8, clm_gemm.h: exactly the value the loader's
// dequantise-then-cast stores, rounded to nearest even) and write the dense tile's uint4s into the dense tile's LDS layout;
// the k loop, its order and both epilogues (EP_OSS_GLU, EP_F32_BIAS with the per-expert biases) are the dense kernel's code.
// Attention, router, plan, gather and combine are the kernels of causal_lm_gptoss.hip, the forward is clm_gptoss.h's
// gptoss_forward and the workspace gptoss_layout's; both tiles go through launch_gemm's one rule.
//
// A descriptor pair with mx is checked by the dense unit's clm_gptoss_check_model on a copy of the layer records whose
// gate_up_w / down_w point at the nibbles, after this unit's own refusals: a null mx, a null pointer inside it, and a model
// that also holds dense experts.  The forward runs on that copy, so gptoss_mlp needs the scale bytes alone.
//
// This unit instantiates the packed grouped GEMM with the two epilogues (on both tiles), the router, the gather and the two
// attention kernels, in both element types, the plan and combine kernels, and the unpack kernel in both element types.
#include <vector>

#include "clm_attn.h"
#include "clm_gptoss.h"

namespace b2t {
namespace {

template <class El>
struct GptOssMxPolicy : LlamaShared<El>, MoeOps<El>, GptOssOps<El> {
  static int gemm_experts_glu(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_OSS_GLU, El, true, true>); }
  static int gemm_experts_f32b(const ClmGemm& g, hipStream_t s) { return launch_gemm(g, s, &clm_gemm_tiles<EP_F32_BIAS, El, true, true>); }
};

// what the entry-point bodies of clm_internal.h carry beside the model: the gpt-oss descriptor and the packed experts
struct GptOssMxArg {
  const b2t_clm_gptoss_t* g;
  const b2t_clm_gptoss_mx_t* mx;
};

// GptOssFamily on that pair: check, layout and the attention are its own on x->g (gptoss_of); the forward gets the scale bytes
struct GptOssMxFamily : GptOssFamily {
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const GptOssMxArg* x) {
    return gptoss_forward<P>(m, *x->g, r, L, base, attn, s, x->mx);
  }
};

// This unit's refusals, and the model the forward runs on: `model` with a copy of its layer records (`layers`, which the caller
// keeps alive) whose gate_up_w / down_w are the nibbles.  A model the dense check will refuse for its dimensions or for null
// layer arrays passes through unchanged, and is refused there.
int mx_model(const char* who, const b2t_clm_llama_t* model, const b2t_clm_gptoss_mx_t* mx, std::vector<b2t_clm_llama_layer_t>& layers,
             b2t_clm_llama_t* out) {
  B2T_REQUIRE(model, "b2t_clm_gptoss: null model");
  B2T_REQUIRE(mx, "%s: null mx descriptor (the experts kept in MXFP4)", who);
  *out = *model;
  if (model->n_layers <= 0 || !model->layers_host) return 0;
  layers.assign(model->layers_host, model->layers_host + model->n_layers);
  for (int l = 0; l < model->n_layers; ++l) {
    B2T_REQUIRE(!layers[l].gate_up_w && !layers[l].down_w,
                "%s: layer %d of the model has gate_up_w / down_w beside the packed experts; a caller holds one form, not both", who, l);
    B2T_REQUIRE(mx[l].gate_up_q && mx[l].gate_up_s && mx[l].down_q && mx[l].down_s, "%s: null pointer in layer %d of mx", who, l);
    layers[l].gate_up_w = mx[l].gate_up_q;
    layers[l].down_w = mx[l].down_q;
  }
  out->layers_host = layers.data();
  return 0;
}

template <class P>
int mx_score(const char* who, const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const b2t_clm_gptoss_mx_t* mx,
             const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out, void* ws,
             size_t ws_bytes, void* stream) {
  std::vector<b2t_clm_llama_layer_t> layers;
  b2t_clm_llama_t m;
  if (int rc = mx_model(who, model, mx, layers, &m)) return rc;
  const GptOssMxArg x{oss, mx};
  return clm_family_score<P, GptOssMxFamily>(who, &m, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out, ws, ws_bytes, stream,
                                             &x);
}

template <class P>
int mx_score_tree(const char* who, const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const b2t_clm_gptoss_mx_t* mx,
                  const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                  long long* n_nodes_out, void* ws, size_t ws_bytes, void* stream) {
  std::vector<b2t_clm_llama_layer_t> layers;
  b2t_clm_llama_t m;
  if (int rc = mx_model(who, model, mx, layers, &m)) return rc;
  const GptOssMxArg x{oss, mx};
  return clm_family_score_tree<P, GptOssMxFamily>(who, &m, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out, n_nodes_out, ws,
                                                  ws_bytes, stream, &x);
}

// packed rows to dense ones: a thread expands one piece of eight elements, the GEMM's unit, with the GEMM's function
template <class E>
__global__ __launch_bounds__(256) void clm_mxfp4_unpack_kernel(const unsigned* q, const unsigned char* sc, long long pieces, uint4* out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < pieces) out[i] = mxfp4_unpack8<E>(q[i], sc[i >> 2]);
}

template <class E>
int mx_unpack(const char* who, const void* q, const void* s, long long rows, int K, void* out, void* stream) {
  B2T_REQUIRE(rows >= 0 && K > 0 && K % 32 == 0, "%s: rows %lld, K %d (K must be a positive multiple of 32)", who, rows, K);
  if (rows == 0) return 0;
  B2T_REQUIRE(q && s && out, "%s: null argument", who);
  const long long blocks = (rows * (K / 8) + 255) / 256;
  B2T_REQUIRE(rows <= (1LL << 40) / K && blocks <= INT_MAX, "%s: %lld rows of %d elements are too many for one launch", who, rows, K);
  hipLaunchKernelGGL(clm_mxfp4_unpack_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     static_cast<const unsigned*>(q), static_cast<const unsigned char*>(s), rows * (K / 8), static_cast<uint4*>(out));
  B2T_CHECK_LAUNCH("clm_mxfp4_unpack_kernel");
  return 0;
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_gptoss_mx_score_f16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const b2t_clm_gptoss_mx_t* mx,
                                           const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                           float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return mx_score<GptOssMxPolicy<_Float16>>("b2t_clm_gptoss_mx_score_f16", model, oss, mx, ids_host, seq_off_host, n_seq, scores_out,
                                            tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_gptoss_mx_score_tree_f16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss,
                                                const b2t_clm_gptoss_mx_t* mx, const int32_t* ids_host, const int32_t* seq_off_host,
                                                int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                                size_t ws_bytes, void* stream) {
  return mx_score_tree<GptOssMxPolicy<_Float16>>("b2t_clm_gptoss_mx_score_tree_f16", model, oss, mx, ids_host, seq_off_host, n_seq,
                                                 scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_gptoss_mx_score_bf16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss, const b2t_clm_gptoss_mx_t* mx,
                                            const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                            float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return mx_score<GptOssMxPolicy<__bf16>>("b2t_clm_gptoss_mx_score_bf16", model, oss, mx, ids_host, seq_off_host, n_seq, scores_out,
                                          tok_logp_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_gptoss_mx_score_tree_bf16(const b2t_clm_llama_t* model, const b2t_clm_gptoss_t* oss,
                                                 const b2t_clm_gptoss_mx_t* mx, const int32_t* ids_host, const int32_t* seq_off_host,
                                                 int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                                 size_t ws_bytes, void* stream) {
  return mx_score_tree<GptOssMxPolicy<__bf16>>("b2t_clm_gptoss_mx_score_tree_bf16", model, oss, mx, ids_host, seq_off_host, n_seq,
                                               scores_out, tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}

extern "C" int b2t_clm_mxfp4_unpack_f16(const void* q, const void* s, long long rows, int K, void* out, void* stream) {
  return mx_unpack<_Float16>("b2t_clm_mxfp4_unpack_f16", q, s, rows, K, out, stream);
}

extern "C" int b2t_clm_mxfp4_unpack_bf16(const void* q, const void* s, long long rows, int K, void* out, void* stream) {
  return mx_unpack<__bf16>("b2t_clm_mxfp4_unpack_bf16", q, s, rows, K, out, stream);
}
