// clm_gemma2.h — the Gemma-2 forward (causal_lm_gemma2.hip's header has the contract and the kernel sequence), written once for
// both element types like clm_olmo2.h: the three kernels Gemma-2 adds, its workspace layout, gemma2_forward and Gemma2Family,
// which hands them to the entry-point bodies and the size rules of clm_internal.h.  A policy P of this forward is LlamaShared<E>
// (the QKV GEMM with EP_ROPE and the uncapped head GEMM) plus
//   P::gemm_geglu, P::gemm_f32, P::gemm_head_cap (g, s)   the gate / up GEMM with EP_GEGLU, the o_proj / down GEMM with EP_F32
//                                                         and the head GEMM with EP_HEAD_CAP
//   P::embed_scaled, P::rmsnorm1p, P::postnorm1p_add      the launches of the three kernels below
//   P::attn, P::attn_tree (..., hd, cap, s)               the flat and the tree attention with the soft cap
#pragma once
#include "clm_llama.h"

namespace b2t {

// dimensions, head dim, caps and weight pointers of a Gemma-2 descriptor pair (0, or an error with the message set);
// causal_lm_gemma2.hip
int clm_gemma2_check_model(const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2);

namespace {

// resid[t] = embed_tokens[id[t]] * scale in fp32 (scale = E(sqrt(d)) widened, from the host)
template <class E>
__global__ __launch_bounds__(256) void clm_gemma2_embed_kernel(const int* ids, const E* et, float scale, float* resid, int d) {
  const int t = blockIdx.x;
  const E* a = et + (long long)ids[t] * d;
  float* o = resid + (long long)t * d;
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (float)a[c] * scale;
}

// clm_llama_rmsnorm_kernel with the weight 1 + w, formed in fp32: out[r] = E(x * rsqrt(mean(x^2) + eps) * (1 + w)) of row
// rowmap ? rowmap[r] : r for r < rows; zeros for rows <= r < gridDim.x (the operand's padding)
template <class E>
__global__ __launch_bounds__(256) void clm_gemma2_rmsnorm_kernel(const float* x, const int* rowmap, int rows, const E* w, float eps,
                                                                 E* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  E* o = out + (long long)r * d;
  if (r >= rows) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)0.f;
    return;
  }
  const float* xr = x + (long long)(rowmap ? rowmap[r] : r) * d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) v += xr[c] * xr[c];
  const float rstd = 1.0f / sqrtf(block_sum256(v, red) / d + eps);
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)(xr[c] * rstd * (1.0f + (float)w[c]));
}

// clm_olmo2_postnorm_add_kernel with the weight 1 + w, and the next pre-norm behind it: resid[r] += t[r] * rsqrt(mean(t[r]^2) +
// eps) * (1 + w) in fp32, then, with wn set, out[r] = E(RMSNorm1p(resid[r]; wn)), the next GEMM's A operand (zeros for rows <= r
// < gridDim.x).  A thread reads back only the elements of resid it wrote itself.  Both sums are the strided loop and
// block_sum256 of the RMSNorm kernel over the row's d elements.
template <class E>
__global__ __launch_bounds__(256) void clm_gemma2_postnorm_add_kernel(const float* t, int rows, const E* w, float eps, float* resid,
                                                                      const E* wn, E* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  if (r >= rows) {
    if (wn)
      for (int c = threadIdx.x; c < d; c += 256) out[(long long)r * d + c] = (E)0.f;
    return;
  }
  float* xr = resid + (long long)r * d;
  const float* tr = t + (long long)r * d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) v += tr[c] * tr[c];
  const float rstd = 1.0f / sqrtf(block_sum256(v, red) / d + eps);
  float v2 = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) {
    const float x = xr[c] + tr[c] * rstd * (1.0f + (float)w[c]);
    xr[c] = x;
    v2 += x * x;
  }
  if (!wn) return;   // uniform
  const float rstd2 = 1.0f / sqrtf(block_sum256(v2, red) / d + eps);
  E* o = out + (long long)r * d;
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)(xr[c] * rstd2 * (1.0f + (float)wn[c]));
}

// the launches of the three kernels for element type El
template <class El>
struct Gemma2Ops {
  static int embed_scaled(const int* ids, const El* et, float scale, float* resid, int d, long long rows, hipStream_t s) {
    hipLaunchKernelGGL(clm_gemma2_embed_kernel<El>, dim3((unsigned)rows), dim3(256), 0, s, ids, et, scale, resid, d);
    B2T_CHECK_LAUNCH("clm_gemma2_embed_kernel");
    return 0;
  }
  static int rmsnorm1p(const float* x, const int* rowmap, long long n, const El* w, float eps, El* out, int d, hipStream_t s) {
    hipLaunchKernelGGL(clm_gemma2_rmsnorm_kernel<El>, dim3((unsigned)rup(n, ROWPAD)), dim3(256), 0, s, x, rowmap, (int)n, w, eps,
                       out, d);
    B2T_CHECK_LAUNCH("clm_gemma2_rmsnorm_kernel");
    return 0;
  }
  static int postnorm1p_add(const float* t, long long rows, const El* w, float eps, float* resid, const El* wn, El* out, int d,
                            hipStream_t s) {
    hipLaunchKernelGGL(clm_gemma2_postnorm_add_kernel<El>, dim3((unsigned)(wn ? rup(rows, ROWPAD) : rows)), dim3(256), 0, s, t,
                       (int)rows, w, eps, resid, wn, out, d);
    B2T_CHECK_LAUNCH("clm_gemma2_postnorm_add_kernel");
    return 0;
  }
};

// The layout of clm_layout with the real QKV width (Hq + 2 Hkv) hd plus, behind its total, an fp32 region [padded rows][d] (the
// o_proj and the down output in front of their post-norms) and the attention output [padded rows][Hq hd], which may be wider
// than d and so does not share x16.  A cached call's state goes behind the new total.
inline size_t gemma2_t32_bytes(const b2t_clm_llama_t* m, long long Mp) { return al256(sizeof(float) * (size_t)(Mp * m->d_model)); }
inline size_t gemma2_ao_bytes(const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2, long long Mp) {
  return al256(2 * (size_t)(Mp * m->n_heads * g2->head_dim));
}
inline ClmLayout gemma2_layout(const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * g2->head_dim;
  ClmLayout L = clm_layout(m->d_model, qw, m->ffn_dim, m->vocab, rows, hrows, ints);
  L.total += gemma2_t32_bytes(m, L.Mp) + gemma2_ao_bytes(m, g2, L.Mp);
  return L;
}

// The forward over r.rows rows up to the per-row log-probs; attn(layer, qkv, out) enqueues one layer's attention, out being
// [rows][Hq hd].  x16 holds E(RMSNorm1p(resid; the next pre-norm)) on entry to every GEMM that reads it.  norm1_w / norm2_w of
// a layer are input_layernorm and post_attention_layernorm, g2's per-layer pair the two feed-forward norms.
template <class P, class Attn>
int gemma2_forward(const b2t_clm_llama_t& m, const b2t_clm_gemma2_t& g2, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn,
                   hipStream_t s) {
  using E = typename P::E;
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = g2.head_dim, F = m.ffn_dim, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  char* behind = base + L.total - gemma2_t32_bytes(&m, L.Mp) - gemma2_ao_bytes(&m, &g2, L.Mp);
  float* t32 = reinterpret_cast<float*>(behind);
  E* ao = reinterpret_cast<E*>(behind + gemma2_t32_bytes(&m, L.Mp));
  E* x16 = reinterpret_cast<E*>(base + L.x16);
  E* qkv = reinterpret_cast<E*>(base + L.qkv);
  E* hb = reinterpret_cast<E*>(base + L.hbuf);
  auto W = [](const void* p) { return static_cast<const E*>(p); };
  if (int rc = P::embed_scaled(r.d_ids, W(m.embed_tokens), g2.embed_scale, resid, d, rows, s)) return rc;
  if (m.n_layers > 0)
    if (int rc = P::rmsnorm1p(resid, nullptr, rows, W(m.layers_host[0].norm1_w), m.rms_eps, x16, d, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    const b2t_clm_gemma2_layer_t& w2 = g2.layers_host[l];
    ClmGemm g{};
    g.A = x16; g.B = w.qkv_w; g.M = (int)rows; g.N = qw; g.K = d; g.out16 = qkv; g.ldo = qw;
    g.qscale = g2.q_scale; g.qcols = Hq * hd;
    g.pos = r.d_pos; g.rope_cos = m.rope_cos; g.rope_sin = m.rope_sin; g.rope_cols = (Hq + Hkv) * hd; g.hd = hd;
    if (int rc = P::gemm_rope(g, s)) return rc;
    if (int rc = attn(l, qkv, ao)) return rc;
    g = ClmGemm{};
    g.A = ao; g.B = w.o_w; g.M = (int)rows; g.N = d; g.K = Hq * hd; g.resid = t32; g.ldo = d;
    if (int rc = P::gemm_f32(g, s)) return rc;
    if (int rc = P::postnorm1p_add(t32, rows, W(w.norm2_w), m.rms_eps, resid, W(w2.pre_ffn_norm_w), x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.gate_up_w; g.M = (int)rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (int rc = P::gemm_geglu(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.down_w; g.M = (int)rows; g.N = d; g.K = F; g.resid = t32; g.ldo = d;
    if (int rc = P::gemm_f32(g, s)) return rc;
    const void* next = l + 1 < m.n_layers ? m.layers_host[l + 1].norm1_w : nullptr;   // the last layer: the head's norm is below
    if (int rc = P::postnorm1p_add(t32, rows, W(w2.post_ffn_norm_w), m.rms_eps, resid, W(next), x16, d, s)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = P::rmsnorm1p(resid, r.d_src, r.Mh, W(m.final_norm_w), m.rms_eps, x16, d, s)) return rc;
  if (g2.final_cap <= 0.f) return clm_head(x16, m.lm_head, m.vocab, d, r, L, base, s, &P::gemm_head);
  // clm_head with the cap in the GEMM's arguments
  ClmGemm g{};
  g.A = x16; g.B = m.lm_head; g.M = (int)r.Mh; g.N = m.vocab; g.K = d; g.cap = g2.final_cap;
  g.pmax = reinterpret_cast<float*>(base + L.pmax); g.psum = reinterpret_cast<float*>(base + L.psum);
  g.tlogit = reinterpret_cast<float*>(base + L.tlogit); g.tgt = r.d_tgt; g.ncg = (int)L.ncg;
  if (int rc = P::gemm_head_cap(g, s)) return rc;
  return clm_launch_head_combine(g.pmax, g.psum, g.tlogit, g.ncg, reinterpret_cast<float*>(base + L.logp), r.Mh, s);
}

// what the entry-point bodies and the size rules of clm_internal.h take from this family; the extra argument is the b2t_clm_gemma2_t
struct Gemma2Family {
  using Model = b2t_clm_llama_t;
  using Extra = b2t_clm_gemma2_t;
  static int kv_heads(const b2t_clm_llama_t& m) { return m.n_kv_heads; }
  static int head_dim(const b2t_clm_llama_t&, const b2t_clm_gemma2_t* g2) { return g2->head_dim; }
  static float attn_cap(const b2t_clm_gemma2_t* g2) { return g2->attn_cap; }
  static bool dims_ok(const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2) {
    return llama_dims_ok(m) && g2 && (g2->head_dim == 128 || g2->head_dim == 256);
  }
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const b2t_clm_gemma2_t* g2) {
    return gemma2_layout(m, g2, rows, hrows, ints);
  }
  template <class P>
  static int check(const char*, const b2t_clm_llama_t* m, const b2t_clm_gemma2_t* g2) { return clm_gemma2_check_model(m, g2); }
  template <class P>
  static int attn(const b2t_clm_llama_t& m, const b2t_clm_gemma2_t* g2, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                  const int* seq_off, int n_seq, hipStream_t s) {
    return P::attn(qkv, out, seq_off, n_seq, m.n_heads, m.n_kv_heads, g2->head_dim, g2->attn_cap, s);
  }
  template <class P>
  static int attn_tree(const b2t_clm_llama_t& m, const b2t_clm_gemma2_t* g2, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                       const int* seq_off, const int* tok_node, const int* own_start, int n_seq, hipStream_t s) {
    return P::attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, m.n_heads, m.n_kv_heads, g2->head_dim, g2->attn_cap, s);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_gemma2_t* g2) {
    return gemma2_forward<P>(m, *g2, r, L, base, attn, s);
  }
};

}  // namespace
}  // namespace b2t
