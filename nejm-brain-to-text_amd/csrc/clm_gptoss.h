// clm_gptoss.h — the gpt-oss forward (causal_lm_gptoss.hip's header has the contract and the kernel sequence), written once for
// both element types like clm_gemma2.h: the router kernel gpt-oss adds, its workspace layout, one layer's routed MLP
// (gptoss_mlp: plan, gather and combine are clm_moe.h's kernels and region, unchanged), gptoss_forward and GptOssFamily, which
// hands them to the entry-point bodies and the size rules of clm_internal.h.  A policy P of this forward is LlamaShared<E> (the QKV
// GEMM with bias and rotation, the o_proj GEMM with bias into the residual, the head, embed, RMSNorm), MoeOps<E> (gather) and
// GptOssOps<E> (below: the router's launch route_oss, and attn_sink / attn_tree_sink (..., sinks, window, s), the flat and the
// tree attention with a sink and a window, instantiated by the unit that names the policy) plus
//   P::gemm_experts_glu, P::gemm_experts_f32b (g, s)   the two grouped GEMMs with EP_OSS_GLU and EP_F32_BIAS
#pragma once
#include "clm_attn.h"
#include "clm_moe.h"

namespace b2t {

// dimensions, head dim, expert counts, strides and weight pointers of a gpt-oss descriptor pair (0, or an error with the message
// set); causal_lm_gptoss.hip
int clm_gptoss_check_model(const b2t_clm_llama_t* m, const b2t_clm_gptoss_t* g);

namespace {

constexpr int OSS_MAX_EXPERTS = 128, OSS_HEAD_DIM = 64;

// One row: the router's logits l[e] = b[e] + sum_c x[c] Wr[e][c] for up to 128 experts, the choice and the weights.  Wave w takes
// the experts w, w + 4, ...: a lane widens the 16-byte pieces lane, lane + 64, ... of the two rows and sums their products in
// fp32 in piece order, element order inside a piece, and a fixed butterfly over the 64 lanes adds the lanes' sums, so a logit
// depends on its row alone, and the kernel has one barrier where a block reduction per expert would have two per expert.  The
// logits are never rounded.  Wave 0 then chooses k experts by repeated argmax (a lane holds experts lane and lane + 64; the
// larger value wins, the lower index among equals) and forms w[j] = exp(l[e_j] - l[e_0]) / sum_i exp(l[e_i] - l[e_0]) in fp32, the
// sum in order of choice.  A comparison with a NaN is false, and a lane offers only experts not yet taken, so whatever the
// logits hold the ids are k distinct values in [0, ne): a NaN shows in the score, never in an address.
// route_e / route_w: [rows][k]; route_out (optional): the ids once more, for the caller.  d % 8 == 0, ne <= 128, k <= min(8, ne).
template <class E>
__global__ __launch_bounds__(256) void clm_gptoss_route_kernel(const E* x, const E* wr, const E* br, int d, int ne, int k,
                                                               int* route_e, float* route_w, int* route_out) {
  using vec8 = typename ClmElem<E>::v8;
  __shared__ float lg[OSS_MAX_EXPERTS];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const E* xr = x + (long long)r * d;
  for (int e = wave; e < ne; e += 4) {
    const E* w = wr + (long long)e * d;
    float v = 0.f;
    for (int c = lane * 8; c < d; c += 512) {
      const vec8 a = *reinterpret_cast<const vec8*>(xr + c), b = *reinterpret_cast<const vec8*>(w + c);
#pragma unroll
      for (int j = 0; j < 8; ++j) v += (float)a[j] * (float)b[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) lg[e] = (float)br[e] + v;
  }
  __syncthreads();
  if (wave != 0) return;
  bool a0 = lane < ne, a1 = lane + 64 < ne;   // the lane's two experts are still to be had
  const float v0 = a0 ? lg[lane] : 0.f, v1 = a1 ? lg[lane + 64] : 0.f;
  float l0 = 0.f, sum = 0.f, mine = 0.f;
  int my_id = 0;
  for (int j = 0; j < k; ++j) {
    int bi = -1;
    float bv = 0.f;
    if (a0) { bi = lane; bv = v0; }
    if (a1 && (bi < 0 || v1 > bv)) { bi = lane + 64; bv = v1; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi >= 0 && (bi < 0 || ov > bv || (!(bv > ov) && oi < bi))) { bv = ov; bi = oi; }
    }
    bi = __shfl(bi, 0);   // k <= ne: an expert is left, and lane 0 holds one
    bv = __shfl(bv, 0);
    if (bi == lane) a0 = false;
    if (bi == lane + 64) a1 = false;
    if (j == 0) l0 = bv;
    const float ex = expf(bv - l0);
    sum += ex;
    if (lane == j) { mine = ex; my_id = bi; }
  }
  if (lane < k) {
    const long long at = (long long)r * k + lane;
    route_e[at] = my_id;
    route_w[at] = mine / sum;
    if (route_out) route_out[at] = my_id;
  }
}

template <class El>
struct GptOssOps {
  static int route_oss(const El* x, const El* wr, const El* br, int d, int ne, int k, int* route_e, float* route_w, int* route_out,
                       long long rows, hipStream_t s) {
    hipLaunchKernelGGL(clm_gptoss_route_kernel<El>, dim3((unsigned)rows), dim3(256), 0, s, x, wr, br, d, ne, k, route_e, route_w,
                       route_out);
    B2T_CHECK_LAUNCH("clm_gptoss_route_kernel");
    return 0;
  }
  static int attn_sink(const El* qkv, El* out, const int* seq_off, int n_seq, int Hq, int Hkv, const float* sinks, int window,
                       hipStream_t s) {
    hipLaunchKernelGGL((clm_attn_sink_kernel<OSS_HEAD_DIM, El>), dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv, sinks,
                       window);
    B2T_CHECK_LAUNCH("clm_attn_sink_kernel");
    return 0;
  }
  static int attn_tree_sink(const El* qkv, El* out, const int* seq_off, const int* tok_node, const int* own_start, int n_seq, int Hq,
                            int Hkv, const float* sinks, int window, hipStream_t s) {
    hipLaunchKernelGGL((clm_attn_tree_sink_kernel<OSS_HEAD_DIM, El>), dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, seq_off, tok_node,
                       own_start, Hq, Hkv, sinks, window);
    B2T_CHECK_LAUNCH("clm_attn_tree_sink_kernel");
    return 0;
  }
};

// the fields of the descriptor that size and drive clm_moe.h's region and plan (router_w_host is per layer here, and unused there)
inline b2t_clm_moe_t gptoss_moe(const b2t_clm_gptoss_t* g) {
  b2t_clm_moe_t moe{};
  moe.n_experts = g->n_experts; moe.top_k = g->top_k;
  moe.gate_up_stride = g->gate_up_stride; moe.down_stride = g->down_stride; moe.route_out = g->route_out;
  return moe;
}

// The layout of clm_layout with the real QKV width (Hq + 2 Hkv) hd and no dense hidden rows plus, behind its total, the attention
// output [padded rows][Hq hd] (wider than d, so it does not share x16) and then clm_moe.h's region for `rows` rows.
inline size_t gptoss_ao_bytes(const b2t_clm_llama_t* m, const b2t_clm_gptoss_t* g, long long Mp) {
  return al256(2 * (size_t)(Mp * m->n_heads * g->head_dim));
}
inline ClmLayout gptoss_layout(const b2t_clm_llama_t* m, const b2t_clm_gptoss_t* g, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * g->head_dim;
  ClmLayout L = clm_layout(m->d_model, qw, 0, m->vocab, rows, hrows, ints);
  const b2t_clm_moe_t moe = gptoss_moe(g);
  L.total += gptoss_ao_bytes(m, g, L.Mp) + moe_region(m, &moe, rows).bytes;
  return L;
}

// One layer's MLP over `rows` rows, x16 = E(RMSNorm(resid; norm2_w)) the operand of the router and of the experts alike:
// resid += sum_j w[j] (glu_{e_j}(x16) down_{e_j}^T + b_down_{e_j}), in order of choice.  moe_mlp of clm_moe.h with this family's
// router, the per-expert biases and EP_OSS_GLU; the plan, the gather, S and the combine are that file's.  With mx (the experts
// kept in MXFP4, causal_lm_gptoss_mx.hip) gate_up_w / down_w of the layer are the packed nibbles and mx[l] has their scale bytes;
// P's two grouped GEMMs are then the packed ones.
template <class P>
int gptoss_mlp(const b2t_clm_llama_t& m, const b2t_clm_gptoss_t& g, int l, long long rows, const ClmLayout& L, char* base,
               const typename P::E* x16, float* resid, hipStream_t s, const b2t_clm_gptoss_mx_t* mx = nullptr) {
  using E = typename P::E;
  const int d = m.d_model, F = m.ffn_dim, ne = g.n_experts, k = g.top_k;
  const b2t_clm_moe_t moe = gptoss_moe(&g);
  const MoeRegion R = moe_region(&m, &moe, rows);
  B2T_REQUIRE(R.S <= INT_MAX, "b2t_clm_gptoss: %lld sorted rows do not fit an int", R.S);
  char* reg = base + L.total - R.bytes;
  int* route_e = reinterpret_cast<int*>(reg + R.route_e);
  float* route_w = reinterpret_cast<float*>(reg + R.route_w);
  int* slot_of = reinterpret_cast<int*>(reg + R.slot_of);
  int* perm = reinterpret_cast<int*>(reg + R.perm);
  int* blk_expert = reinterpret_cast<int*>(reg + R.blk_expert);
  E* xs = reinterpret_cast<E*>(reg + R.xs);
  E* hs = reinterpret_cast<E*>(reg + R.hs);
  float* ys = reinterpret_cast<float*>(reg + R.ys);
  const b2t_clm_llama_layer_t& w = m.layers_host[l];
  const b2t_clm_gptoss_layer_t& w2 = g.layers_host[l];
  int* route_out = g.route_out ? g.route_out + (long long)l * rows * k : nullptr;
  if (int rc = P::route_oss(x16, static_cast<const E*>(w2.router_w), static_cast<const E*>(w2.router_b), d, ne, k, route_e, route_w,
                            route_out, rows, s))
    return rc;
  hipLaunchKernelGGL(clm_moe_plan_kernel, dim3(1), dim3(256), 0, s, route_e, (int)(rows * k), k, ne, (int)R.S, perm, slot_of,
                     blk_expert);
  B2T_CHECK_LAUNCH("clm_moe_plan_kernel");
  if (int rc = P::gather(x16, perm, xs, d, R.S, s)) return rc;
  ClmGemm gm{};
  gm.A = xs; gm.B = w.gate_up_w; gm.M = (int)R.S; gm.N = 2 * F; gm.K = d; gm.out16 = hs; gm.ldo = F;
  gm.blk_expert = blk_expert; gm.b_stride = g.gate_up_stride * d;
  gm.bias = w2.gate_up_b; gm.bias_stride = g.gate_up_stride; gm.glu_limit = g.swiglu_limit;
  gm.b_scale = mx ? mx[l].gate_up_s : nullptr;
  if (int rc = P::gemm_experts_glu(gm, s)) return rc;
  gm = ClmGemm{};
  gm.A = hs; gm.B = w.down_w; gm.M = (int)R.S; gm.N = d; gm.K = F; gm.resid = ys; gm.ldo = d;
  gm.blk_expert = blk_expert; gm.b_stride = g.down_stride * F;
  gm.bias = w2.down_b; gm.bias_stride = g.down_stride;
  gm.b_scale = mx ? mx[l].down_s : nullptr;
  if (int rc = P::gemm_experts_f32b(gm, s)) return rc;
  const long long elems = rows * d;
  hipLaunchKernelGGL(clm_moe_combine_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, ys, slot_of, route_w, k, resid,
                     d, elems);
  B2T_CHECK_LAUNCH("clm_moe_combine_kernel");
  return 0;
}

// The forward over r.rows rows up to the per-row log-probs; attn(layer, qkv, out) enqueues one layer's attention, out being
// [rows][Hq hd].  mx: gptoss_mlp's.
template <class P, class Attn>
int gptoss_forward(const b2t_clm_llama_t& m, const b2t_clm_gptoss_t& g, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn,
                   hipStream_t s, const b2t_clm_gptoss_mx_t* mx = nullptr) {
  using E = typename P::E;
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = g.head_dim, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  const b2t_clm_moe_t moe = gptoss_moe(&g);
  float* resid = reinterpret_cast<float*>(base + L.resid);
  E* x16 = reinterpret_cast<E*>(base + L.x16);
  E* qkv = reinterpret_cast<E*>(base + L.qkv);
  E* ao = reinterpret_cast<E*>(base + L.total - moe_region(&m, &moe, rows).bytes - gptoss_ao_bytes(&m, &g, L.Mp));
  auto W = [](const void* p) { return static_cast<const E*>(p); };
  if (int rc = P::embed(r.d_ids, W(m.embed_tokens), resid, d, rows, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm1_w), m.rms_eps, x16, d, s)) return rc;
    ClmGemm gm{};
    gm.A = x16; gm.B = w.qkv_w; gm.M = (int)rows; gm.N = qw; gm.K = d; gm.bias = w.qkv_b; gm.out16 = qkv; gm.ldo = qw;
    gm.qscale = 1.0f / sqrtf((float)hd); gm.qcols = Hq * hd;
    gm.pos = r.d_pos; gm.rope_cos = m.rope_cos; gm.rope_sin = m.rope_sin; gm.rope_cols = (Hq + Hkv) * hd; gm.hd = hd;
    if (int rc = P::gemm_rope(gm, s)) return rc;
    if (int rc = attn(l, qkv, ao)) return rc;
    gm = ClmGemm{};
    gm.A = ao; gm.B = w.o_w; gm.M = (int)rows; gm.N = d; gm.K = Hq * hd; gm.bias = g.layers_host[l].o_b; gm.resid = resid; gm.ldo = d;
    if (int rc = P::gemm_resid(gm, s)) return rc;
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm2_w), m.rms_eps, x16, d, s)) return rc;
    if (int rc = gptoss_mlp<P>(m, g, l, rows, L, base, x16, resid, s, mx)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = P::rmsnorm(resid, r.d_src, r.Mh, W(m.final_norm_w), m.rms_eps, x16, d, s)) return rc;
  return clm_head(x16, m.lm_head, m.vocab, d, r, L, base, s, &P::gemm_head);
}

// the gpt-oss descriptor in a family's extra argument: the argument itself, or the member g of a record that carries more
inline const b2t_clm_gptoss_t* gptoss_of(const b2t_clm_gptoss_t* g) { return g; }
template <class X>
const b2t_clm_gptoss_t* gptoss_of(const X* x) { return x->g; }

// what the entry-point bodies and the size rules of clm_internal.h take from this family; the extra argument is the
// b2t_clm_gptoss_t, or a record gptoss_of finds it in (causal_lm_gptoss_mx.hip's, whose family takes all but forward from here)
struct GptOssFamily : LlamaFamilyBase {
  template <class X>
  static int head_dim(const b2t_clm_llama_t&, const X* x) { return gptoss_of(x)->head_dim; }
  template <class X>
  static bool dims_ok(const b2t_clm_llama_t* m, const X* x) {
    const b2t_clm_gptoss_t* g = gptoss_of(x);
    return llama_dims_ok(m) && g && g->head_dim == OSS_HEAD_DIM && g->n_experts >= 1 && g->n_experts <= OSS_MAX_EXPERTS &&
           g->top_k >= 1 && g->top_k <= MOE_MAX_TOPK && g->top_k <= g->n_experts;
  }
  template <class X>
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const X* x) {
    return gptoss_layout(m, gptoss_of(x), rows, hrows, ints);
  }
  template <class P, class X>
  static int check(const char*, const b2t_clm_llama_t* m, const X* x) { return clm_gptoss_check_model(m, gptoss_of(x)); }
  template <class P, class X>
  static int attn(const b2t_clm_llama_t& m, const X* x, int l, const typename P::E* qkv, typename P::E* out, const int* seq_off,
                  int n_seq, hipStream_t s) {
    const b2t_clm_gptoss_layer_t& w2 = gptoss_of(x)->layers_host[l];
    return P::attn_sink(qkv, out, seq_off, n_seq, m.n_heads, m.n_kv_heads, w2.sinks, w2.window, s);
  }
  template <class P, class X>
  static int attn_tree(const b2t_clm_llama_t& m, const X* x, int l, const typename P::E* qkv, typename P::E* out, const int* seq_off,
                       const int* tok_node, const int* own_start, int n_seq, hipStream_t s) {
    const b2t_clm_gptoss_layer_t& w2 = gptoss_of(x)->layers_host[l];
    return P::attn_tree_sink(qkv, out, seq_off, tok_node, own_start, n_seq, m.n_heads, m.n_kv_heads, w2.sinks, w2.window, s);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_gptoss_t* g) {
    return gptoss_forward<P>(m, *g, r, L, base, attn, s);
  }
};

}  // namespace
}  // namespace b2t
