// clm_phi3.h — the Phi-3 forward (causal_lm_phi3.hip's header has the contract and the kernel sequence), written once for both
// element types like clm_olmo2.h: the one kernel Phi-3 adds, its workspace layout, phi3_forward and Phi3Family, which hands them
// to the entry-point bodies and the size rules of clm_internal.h.  A policy P of this forward is LlamaShared<E> (embed, RMSNorm, the
// SwiGLU, residual and head GEMMs) plus
//   P::gemm_qkv (g, s)                          the QKV GEMM with EP_QKV_F32
//   P::rope                                     the launch of the kernel below
//   P::attn, P::attn_tree (..., hd, s)          the flat and the tree attention: head dim 96 here, 64 and 128 through LlamaShared
#pragma once
#include "clm_llama.h"

namespace b2t {

// dimensions, head dim, rotary dims and weight pointers of a Phi-3 descriptor pair for the entry point `who` (0, or an error
// with the message set); causal_lm_phi3.hip
int clm_phi3_check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3);

namespace {

// One row of the QKV GEMM's fp32 q | k columns t[r][qcols + kcols] -> the q | k columns of qkv[r] (pitch ldo), in front of the v
// columns the GEMM wrote.  Of every head's hd dims the first rot are rotated, pairs (c, c + rot / 2), c < rot / 2, by the angle of
// the row's position (cos / sin tables of pitch rot / 2); dims rot .. hd - 1 pass through; every q dim, rotated or not, gets
// the factor qscale; one rounding.  An element is computed from its own pair alone, so its bits depend only on the row.
template <class E>
__global__ __launch_bounds__(256) void clm_phi3_rope_kernel(const float* t, const int* pos, const float* rope_cos,
                                                            const float* rope_sin, float qscale, E* qkv, int qcols, int kcols, int hd,
                                                            int rot, int ldo) {
  const int r = blockIdx.x, half = rot >> 1;
  const float* tr = t + (long long)r * (qcols + kcols);
  E* o = qkv + (long long)r * ldo;
  const float* cs = rope_cos + (long long)pos[r] * half;
  const float* sn = rope_sin + (long long)pos[r] * half;
  for (int i = threadIdx.x; i < qcols + kcols; i += 256) {
    const int c = i % hd;                       // qcols is a multiple of hd: a head is q or k as a whole
    const float sc = i < qcols ? qscale : 1.f;
    const float x = tr[i];
    float v = x;                                // c >= rot: passes through
    if (c < half) v = x * cs[c] - tr[i + half] * sn[c];
    else if (c < rot) v = x * cs[c - half] + tr[i - half] * sn[c - half];
    o[i] = (E)(v * sc);
  }
}

// the launch of the kernel for element type El (a policy's rope)
template <class El>
struct Phi3Ops {
  static int rope(const float* t, const int* pos, const b2t_clm_llama_t& m, const b2t_clm_phi3_t& p3, El* qkv, long long rows,
                  hipStream_t s) {
    const int hd = p3.head_dim;
    hipLaunchKernelGGL(clm_phi3_rope_kernel<El>, dim3((unsigned)rows), dim3(256), 0, s, t, pos, m.rope_cos, m.rope_sin,
                       1.0f / sqrtf((float)hd), qkv, m.n_heads * hd, m.n_kv_heads * hd, hd, p3.rotary_dims,
                       (m.n_heads + 2 * m.n_kv_heads) * hd);
    B2T_CHECK_LAUNCH("clm_phi3_rope_kernel");
    return 0;
  }
};

// The layout of clm_layout with the QKV width (Hq + 2 Hkv) hd of the descriptor's head dim plus, behind its total, OLMo-2's fp32
// region [padded rows][(Hq + Hkv) hd]: the q | k columns of the QKV GEMM.  Once the rotation has read them the region is free, and
// the attention writes its output [rows][Hq hd] there in the element type (half the bytes of the q columns alone), so that
// Hq hd need not equal d_model.  A cached call's state goes behind the new total.
inline size_t phi3_t32_bytes(const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3, long long Mp) {
  return al256(sizeof(float) * (size_t)(Mp * (m->n_heads + m->n_kv_heads) * p3->head_dim));
}
inline ClmLayout phi3_layout(const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * p3->head_dim;
  ClmLayout L = clm_layout(m->d_model, qw, m->ffn_dim, m->vocab, rows, hrows, ints);
  L.total += phi3_t32_bytes(m, p3, L.Mp);
  return L;
}

// The forward over r.rows rows up to the per-row log-probs; attn(layer, qkv, out) enqueues one layer's attention, out being
// [rows][Hq hd].  norm1_w / norm2_w of a layer are input_layernorm and post_attention_layernorm.
template <class P, class Attn>
int phi3_forward(const b2t_clm_llama_t& m, const b2t_clm_phi3_t& p3, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn,
                 hipStream_t s) {
  using E = typename P::E;
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = p3.head_dim, F = m.ffn_dim, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  float* t32 = reinterpret_cast<float*>(base + L.total - phi3_t32_bytes(&m, &p3, L.Mp));
  E* ao = reinterpret_cast<E*>(t32);   // the attention output, once the rotation has read the q | k columns
  E* x16 = reinterpret_cast<E*>(base + L.x16);
  E* qkv = reinterpret_cast<E*>(base + L.qkv);
  E* hb = reinterpret_cast<E*>(base + L.hbuf);
  auto W = [](const void* p) { return static_cast<const E*>(p); };
  if (int rc = P::embed(r.d_ids, W(m.embed_tokens), resid, d, rows, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm1_w), m.rms_eps, x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = w.qkv_w; g.M = (int)rows; g.N = qw; g.K = d; g.resid = t32; g.rope_cols = (Hq + Hkv) * hd; g.out16 = qkv;
    g.ldo = qw;
    if (int rc = P::gemm_qkv(g, s)) return rc;
    if (int rc = P::rope(t32, r.d_pos, m, p3, qkv, rows, s)) return rc;
    if (int rc = attn(l, qkv, ao)) return rc;
    g = ClmGemm{};
    g.A = ao; g.B = w.o_w; g.M = (int)rows; g.N = d; g.K = Hq * hd; g.resid = resid; g.ldo = d;
    if (int rc = P::gemm_resid(g, s)) return rc;
    if (int rc = P::rmsnorm(resid, nullptr, rows, W(w.norm2_w), m.rms_eps, x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.gate_up_w; g.M = (int)rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (int rc = P::gemm_swiglu(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.down_w; g.M = (int)rows; g.N = d; g.K = F; g.resid = resid; g.ldo = d;
    if (int rc = P::gemm_resid(g, s)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = P::rmsnorm(resid, r.d_src, r.Mh, W(m.final_norm_w), m.rms_eps, x16, d, s)) return rc;
  return clm_head(x16, m.lm_head, m.vocab, d, r, L, base, s, &P::gemm_head);
}

// what the entry-point bodies and the size rules of clm_internal.h take from this family; the extra argument is the b2t_clm_phi3_t.
// Every refusal is under the entry point's name.
struct Phi3Family : LlamaFamilyBase {
  static int head_dim(const b2t_clm_llama_t&, const b2t_clm_phi3_t* p3) { return p3->head_dim; }
  static bool dims_ok(const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3) {
    return llama_dims_ok(m) && p3 && (p3->head_dim == 64 || p3->head_dim == 96 || p3->head_dim == 128);
  }
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const b2t_clm_phi3_t* p3) {
    return phi3_layout(m, p3, rows, hrows, ints);
  }
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_phi3_t* p3) { return clm_phi3_check(who, m, p3); }
  template <class P>
  static int attn(const b2t_clm_llama_t& m, const b2t_clm_phi3_t* p3, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                  const int* seq_off, int n_seq, hipStream_t s) {
    return P::attn(qkv, out, seq_off, n_seq, m.n_heads, m.n_kv_heads, p3->head_dim, s);
  }
  template <class P>
  static int attn_tree(const b2t_clm_llama_t& m, const b2t_clm_phi3_t* p3, int /*layer*/, const typename P::E* qkv, typename P::E* out,
                       const int* seq_off, const int* tok_node, const int* own_start, int n_seq, hipStream_t s) {
    return P::attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, m.n_heads, m.n_kv_heads, p3->head_dim, s);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_phi3_t* p3) {
    return phi3_forward<P>(m, *p3, r, L, base, attn, s);
  }
};

}  // namespace
}  // namespace b2t
