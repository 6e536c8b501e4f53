// clm_olmo2.h — the OLMo-2 forward (causal_lm_olmo2.hip's header has the contract and the kernel sequence), written once for
// both element types like clm_llama.h: the two kernels OLMo-2 adds, its workspace layout, olmo2_forward and Olmo2Family, which
// hands them to the entry-point bodies and the size rules of clm_internal.h.  A policy P of this forward is LlamaShared<E> (embed,
// the final RMSNorm, the SwiGLU and head GEMMs, the attention launchers) plus
//   P::gemm_qkv, P::gemm_f32 (g, s)             the QKV GEMM with EP_QKV_F32 and the o_proj / down GEMM with EP_F32
//   P::qknorm_rope, P::postnorm_add             the launches of the two kernels below
#pragma once
#include "clm_llama.h"

namespace b2t {
namespace {

// One row of the QKV GEMM's fp32 q | k columns t[r][qcols + kcols] -> the q | k columns of qkv[r] (pitch ldo), in front of the v
// columns the GEMM wrote: an RMSNorm over the whole q part and one over the whole k part (one statistic each, all heads
// together; weights [qcols] and [kcols] in checkpoint order), the rotation of every head's pairs (c, c + hd / 2) by the angle
// of the row's position, q's factor qscale, one rounding.  The sums are the strided loop and block_sum256 of
// clm_llama_rmsnorm_kernel, so their order depends on the row alone.
template <class E>
__global__ __launch_bounds__(256) void clm_olmo2_qknorm_rope_kernel(const float* t, const int* pos, const E* qw, const E* kw,
                                                                    const float* rope_cos, const float* rope_sin, float eps,
                                                                    float qscale, E* qkv, int qcols, int kcols, int hd, int ldo) {
  __shared__ float red[4];
  const int r = blockIdx.x, half = hd >> 1;
  const float* tr = t + (long long)r * (qcols + kcols);
  E* o = qkv + (long long)r * ldo;
  float vq = 0.f, vk = 0.f;
  for (int c = threadIdx.x; c < qcols; c += 256) vq += tr[c] * tr[c];
  for (int c = threadIdx.x; c < kcols; c += 256) vk += tr[qcols + c] * tr[qcols + c];
  const float rq = 1.0f / sqrtf(block_sum256(vq, red) / qcols + eps);
  const float rk = 1.0f / sqrtf(block_sum256(vk, red) / kcols + eps);
  const float* cs = rope_cos + (long long)pos[r] * half;
  const float* sn = rope_sin + (long long)pos[r] * half;
  for (int p = threadIdx.x; p < (qcols + kcols) >> 1; p += 256) {   // pair p: frequency p % half of head p / half
    const int i = p % half, c0 = (p / half) * hd + i, c1 = c0 + half;
    const bool isq = c0 < qcols;                                    // qcols is a multiple of hd: a head is q or k as a whole
    const float rstd = isq ? rq : rk, sc = isq ? qscale : 1.f;
    const E* w = isq ? qw + c0 : kw + (c0 - qcols);
    const float x0 = tr[c0] * rstd * (float)w[0], x1 = tr[c1] * rstd * (float)w[half];
    o[c0] = (E)((x0 * cs[i] - x1 * sn[i]) * sc);
    o[c1] = (E)((x1 * cs[i] + x0 * sn[i]) * sc);
  }
}

// resid[r] += RMSNorm(t[r]; w) in fp32 and out[r] = E(resid[r]), the next GEMM's A operand, for r < rows; zeros for
// rows <= r < gridDim.x (the operand's padding).  t null: only the operand (layer 0's, the embedding row itself).
template <class E>
__global__ __launch_bounds__(256) void clm_olmo2_postnorm_add_kernel(const float* t, int rows, const E* w, float eps, float* resid,
                                                                     E* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  E* o = out + (long long)r * d;
  if (r >= rows) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)0.f;
    return;
  }
  float* xr = resid + (long long)r * d;
  if (!t) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (E)xr[c];
    return;
  }
  const float* tr = t + (long long)r * d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) v += tr[c] * tr[c];
  const float rstd = 1.0f / sqrtf(block_sum256(v, red) / d + eps);
  for (int c = threadIdx.x; c < d; c += 256) {
    const float x = xr[c] + tr[c] * rstd * (float)w[c];
    xr[c] = x;
    o[c] = (E)x;
  }
}

// the launches of the two kernels for element type El (a policy's qknorm_rope and postnorm_add)
template <class El>
struct Olmo2Ops {
  static int qknorm_rope(const float* t, const int* pos, const El* qw, const El* kw, const b2t_clm_llama_t& m, El* qkv,
                         long long rows, hipStream_t s) {
    const int hd = m.d_model / m.n_heads;
    hipLaunchKernelGGL(clm_olmo2_qknorm_rope_kernel<El>, dim3((unsigned)rows), dim3(256), 0, s, t, pos, qw, kw, m.rope_cos,
                       m.rope_sin, m.rms_eps, 1.0f / sqrtf((float)hd), qkv, m.n_heads * hd, m.n_kv_heads * hd, hd,
                       (m.n_heads + 2 * m.n_kv_heads) * hd);
    B2T_CHECK_LAUNCH("clm_olmo2_qknorm_rope_kernel");
    return 0;
  }
  static int postnorm_add(const float* t, long long rows, const El* w, float eps, float* resid, El* out, int d, hipStream_t s) {
    hipLaunchKernelGGL(clm_olmo2_postnorm_add_kernel<El>, dim3((unsigned)rup(rows, ROWPAD)), dim3(256), 0, s, t, (int)rows, w, eps,
                       resid, out, d);
    B2T_CHECK_LAUNCH("clm_olmo2_postnorm_add_kernel");
    return 0;
  }
};

// The Llama layout plus, behind its total, one fp32 region [padded rows][(Hq + Hkv) hd]: the q | k columns of the QKV GEMM,
// then the o_proj and the down output (d = Hq hd columns of it).  A cached call's state goes behind the new total.
inline size_t olmo2_t32_bytes(const b2t_clm_llama_t* m, long long Mp) {
  return al256(sizeof(float) * (size_t)(Mp * (m->n_heads + m->n_kv_heads) * (m->d_model / m->n_heads)));
}
inline ClmLayout olmo2_layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints) {
  ClmLayout L = llama_layout(m, rows, hrows, ints);
  L.total += olmo2_t32_bytes(m, L.Mp);
  return L;
}

// The forward over r.rows rows up to the per-row log-probs; attn(layer, qkv, out) enqueues one layer's attention.  x16 holds
// E(resid) on entry to every layer.  qkn is the per-layer q / k norm weights ([Hq hd] and [Hkv hd]), norm1_w / norm2_w of a
// layer are post_attention_layernorm and post_feedforward_layernorm.
template <class P, class Attn>
int olmo2_forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                  const b2t_clm_qknorm_t* qkn) {
  using E = typename P::E;
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = d / Hq, F = m.ffn_dim, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  float* t32 = reinterpret_cast<float*>(base + L.total - olmo2_t32_bytes(&m, L.Mp));
  E* x16 = reinterpret_cast<E*>(base + L.x16);
  E* qkv = reinterpret_cast<E*>(base + L.qkv);
  E* hb = reinterpret_cast<E*>(base + L.hbuf);
  auto W = [](const void* p) { return static_cast<const E*>(p); };
  if (int rc = P::embed(r.d_ids, W(m.embed_tokens), resid, d, rows, s)) return rc;
  if (int rc = P::postnorm_add(nullptr, rows, nullptr, 0.f, resid, x16, d, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    ClmGemm g{};
    g.A = x16; g.B = w.qkv_w; g.M = (int)rows; g.N = qw; g.K = d; g.resid = t32; g.rope_cols = (Hq + Hkv) * hd; g.out16 = qkv;
    g.ldo = qw;
    if (int rc = P::gemm_qkv(g, s)) return rc;
    if (int rc = P::qknorm_rope(t32, r.d_pos, W(qkn[l].q_norm_w), W(qkn[l].k_norm_w), m, qkv, rows, s)) return rc;
    if (int rc = attn(l, qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.o_w; g.M = (int)rows; g.N = d; g.K = d; g.resid = t32; g.ldo = d;
    if (int rc = P::gemm_f32(g, s)) return rc;
    if (int rc = P::postnorm_add(t32, rows, W(w.norm1_w), m.rms_eps, resid, x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = w.gate_up_w; g.M = (int)rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (int rc = P::gemm_swiglu(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = w.down_w; g.M = (int)rows; g.N = d; g.K = F; g.resid = t32; g.ldo = d;
    if (int rc = P::gemm_f32(g, s)) return rc;
    if (int rc = P::postnorm_add(t32, rows, W(w.norm2_w), m.rms_eps, resid, x16, d, s)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = P::rmsnorm(resid, r.d_src, r.Mh, W(m.final_norm_w), m.rms_eps, x16, d, s)) return rc;
  return clm_head(x16, m.lm_head, m.vocab, d, r, L, base, s, &P::gemm_head);
}

// the q / k norm weights of a checked model for the entry point `who`: a null array or entry and a q / k / v bias (OLMo-2 has
// none, and EP_QKV_F32 adds none) are refused
inline int clm_olmo2_check(const char* who, const b2t_clm_llama_t& m, const b2t_clm_qknorm_t* qkn) {
  B2T_REQUIRE(m.n_layers == 0 || qkn, "%s: null qk_norm_host", who);
  for (int l = 0; l < m.n_layers; ++l) {
    B2T_REQUIRE(qkn[l].q_norm_w && qkn[l].k_norm_w, "%s: null q / k norm weight in layer %d", who, l);
    B2T_REQUIRE(!m.layers_host[l].qkv_b, "%s: layer %d has q / k / v biases (qkv_b), which OLMo-2 does not", who, l);
  }
  return 0;
}

// what the entry-point bodies and the size rules of clm_internal.h take from this family
struct Olmo2Family : LlamaFamilyBase {
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const void* /*extra*/ = nullptr) {
    return olmo2_layout(m, rows, hrows, ints);
  }
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_qknorm_t* qkn) {
    if (int rc = clm_llama_check_model(m)) return rc;
    return clm_olmo2_check(who, *m, qkn);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_qknorm_t* qkn) {
    return olmo2_forward<P>(m, r, L, base, attn, s, qkn);
  }
};

}  // namespace
}  // namespace b2t
