// causal_lm_llama.hip — the scoring forward of causal_lm.hip for the Llama family (HF LlamaForCausalLM, MistralForCausalLM,
// Qwen2ForCausalLM): RMSNorm, rotary positions, grouped-query attention, a SwiGLU MLP and an LM head of its own, over packed
// sequences (b2t_clm_llama_score_f16) and over the shared-prefix token tree (b2t_clm_llama_score_tree_f16; the plan is
// causal_lm_tree.hip's, and a node's rotary position is its depth).
//
// Numerics contract (what the fp64 restatement of tests/test_clm_llama_host.py rounds):
//   - weights are fp16; GEMM operands are fp16, accumulation fp32 (v_mfma_f32_32x32x16_f16);
//   - the residual stream (which starts as the fp16 embedding row widened), the RMSNorm statistics, the rotation, softmax /
//     log-softmax and the per-sequence sums are fp32; cos / sin come from an fp32 table the host builds in double;
//   - rounded to fp16, once each: the RMSNorm output x * rsqrt(mean(x^2) + eps) * w; q, k and v -- q and k after the bias, the
//     rotation and (q) the factor head_dim^-0.5, all applied to the fp32 accumulator; the attention output; silu(gate) * up,
//     formed from the two fp32 accumulators (gate and up are never rounded on their own); and the attention's
//     probabilities exp(s - m) per 32-key block as the P.V operand, exactly as in causal_lm.hip.
//   Every output element is computed by one thread in a fixed order that depends only on its own row, so a sequence's score
//   is bit-identical alone or in any batch, and the tree call is bit-identical to the flat call.
//
// Kernels per layer: RMSNorm -> QKV GEMM with the rotation in its epilogue (EP_ROPE, clm_gemm.h) -> causal GQA attention
// (query head h reads K / V head h / (Hq / Hkv)) -> o_proj GEMM into the residual -> RMSNorm -> gate / up GEMM with SwiGLU in
// its epilogue (EP_SWIGLU; the [M][2F] intermediate never exists) -> down GEMM into the residual.  Then the final RMSNorm of
// every position but the last of each sequence and causal_lm.hip's fused head (EP_HEAD with B = lm_head), combine and sums.
// The two weight layouts the epilogues rely on are made at load time (llm_rescore.py): gate / up rows interleaved in blocks
// of 32, and for head dim 128 the q / k rows of each head in the order [0..31, 64..95, 32..63, 96..127] (q . k is invariant
// under one permutation of both; V and o_proj are untouched).
#include <math.h>
#include <vector>

#include "clm_gemm.h"

namespace b2t {
namespace {

__device__ __forceinline__ float llama_block_sum256(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// resid[t] = embed_tokens[id[t]] (fp32)
__global__ __launch_bounds__(256) void clm_llama_embed_kernel(const int* ids, const _Float16* et, float* resid, int d) {
  const int t = blockIdx.x;
  const _Float16* a = et + (long long)ids[t] * d;
  float* o = resid + (long long)t * d;
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (float)a[c];
}

// out[r] = fp16(RMSNorm(x[rowmap ? rowmap[r] : r])) for r < rows; zeros for rows <= r < gridDim.x (the operand's padding)
__global__ __launch_bounds__(256) void clm_llama_rmsnorm_kernel(const float* x, const int* rowmap, int rows, const _Float16* w,
                                                                float eps, _Float16* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  _Float16* o = out + (long long)r * d;
  if (r >= rows) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (_Float16)0.f;
    return;
  }
  const float* xr = x + (long long)(rowmap ? rowmap[r] : r) * d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) v += xr[c] * xr[c];
  const float rstd = 1.0f / sqrtf(llama_block_sum256(v, red) / d + eps);
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (_Float16)(xr[c] * rstd * (float)w[c]);
}

// Causal grouped-query attention, one workgroup per (sequence, query head): clm_attn_kernel's arithmetic (S^T = K . Q^T, a
// lane owns one query column and its online-softmax state, P^T is the B operand of O^T = V^T . P^T) on the row layout
// q[Hq * D] | k[Hkv * D] | v[Hkv * D]; query head h reads K / V head h / G, G = Hq / Hkv.  D is 64 or 128.
template <int D>
__global__ __launch_bounds__(256) void clm_llama_attn_kernel(const _Float16* qkv, _Float16* out, const int* seq_off, int Hq,
                                                             int Hkv) {
  constexpr int KS = D / 16, NF = D / 32;
  const int sq = blockIdx.x, h = blockIdx.y, hk = h / (Hq / Hkv);
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = (long long)(Hq + 2 * Hkv) * D;
  const _Float16* Qb = qkv + (long long)t0 * RS + h * D;
  const _Float16* Kb = qkv + (long long)t0 * RS + (Hq + hk) * D;
  const _Float16* Vb = Kb + Hkv * D;
  const int nqb = (L + 31) / 32;
  for (int qb = wave; qb < nqb; qb += 4) {
    const int q0 = qb * 32, q = q0 + li;
    const _Float16* qp = Qb + (long long)min(q, L - 1) * RS + 8 * hh;
    half8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + 16 * ks);
    float m = -INFINITY, l = 0.f;
    f32x16 o[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[f][e] = 0.f;
    for (int kb = 0; kb <= qb; ++kb) {   // key blocks up to the diagonal; key k0 <= q0 < L is valid for every query row
      const int k0 = kb * 32;
      const _Float16* kp = Kb + (long long)min(k0 + li, L - 1) * RS + 8 * hh;
      f32x16 sacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8*>(kp + 16 * ks), qf[ks], sacc, 0, 0, 0);
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (key > q || key >= L) sacc[e] = -INFINITY;
        mx = fmaxf(mx, sacc[e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(m, mx);
      const float alpha = __expf(m - mnew);
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { const float p = __expf(sacc[e] - mnew); sacc[e] = p; ps += p; }
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = mnew;
      half8 pb[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[s2][j] = (_Float16)sacc[8 * s2 + j];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int e = 0; e < 16; ++e) o[f][e] *= alpha;
        const int dim = 32 * f + li;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          half8 va;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int key = k0 + 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3);
            va[j] = key < L ? Vb[(long long)key * RS + dim] : (_Float16)0.f;
          }
          o[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb[s2], o[f], 0, 0, 0);
        }
      }
    }
    if (q < L) {
      const float inv = 1.0f / l;
      _Float16* op = out + ((long long)(t0 + q) * Hq + h) * D;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int e = 0; e < 16; ++e) op[32 * f + (e & 3) + 8 * (e >> 2) + 4 * hh] = (_Float16)(o[f][e] * inv);
    }
  }
}

// The same over tree paths: clm_attn_tree_kernel's walk (position i of the sequence is row tok_node[seq_off[s] + i]; K and V
// are gathered for all positions 0..q, the wave's LDS slab stages V's 32 x D block, Q is read and the output written only
// for the positions the sequence owns) with the grouped-query row layout above.  Per query the arithmetic order is
// clm_llama_attn_kernel's, so the results are bit-identical to it.
template <int D>
__global__ __launch_bounds__(256) void clm_llama_attn_tree_kernel(const _Float16* qkv, _Float16* out, const int* seq_off,
                                                                  const int* tok_node, const int* own_start, int Hq, int Hkv) {
  constexpr int KS = D / 16, NF = D / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  static_assert(32 * PCS == 64 * NIT, "a V block is a whole number of 16-byte pieces per lane");
  __shared__ __attribute__((aligned(16))) _Float16 vslab[4][32 * VP];
  const int sq = blockIdx.x, h = blockIdx.y, hk = h / (Hq / Hkv);
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0, own = own_start[sq];
  if (own >= L) return;   // every node of this path is owned by an earlier sequence
  const int* path = tok_node + t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = (long long)(Hq + 2 * Hkv) * D;
  const _Float16* Qb = qkv + h * D;
  const _Float16* Kb = qkv + (Hq + hk) * D;
  const _Float16* Vb = Kb + Hkv * D;
  _Float16* vs = vslab[wave];
  const int nqb = (L + 31) / 32;
  for (int qb = own / 32 + wave; qb < nqb; qb += 4) {
    const int q0 = qb * 32, q = q0 + li;
    const int qrow = path[min(q, L - 1)];
    const _Float16* qp = Qb + (long long)qrow * RS + 8 * hh;
    half8 qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + 16 * ks);
    float m = -INFINITY, l = 0.f;
    f32x16 o[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[f][e] = 0.f;
    for (int kb = 0; kb <= qb; ++kb) {
      const int k0 = kb * 32;
      const int krow = path[min(k0 + li, L - 1)];
      const _Float16* kp = Kb + (long long)krow * RS + 8 * hh;
      // stage V[k0 .. k0 + 32) of the path: piece p = 64 * it + lane is columns 8c .. 8c + 7 of key k0 + p / PCS, whose row
      // the lane p / PCS holds
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();   // the previous block's reads of the slab are done
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int p = 64 * it + lane, key = p / PCS, c = p % PCS;
        const int vrow = __shfl(krow, key);
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
        if (k0 + key < L) v = *reinterpret_cast<const half8*>(Vb + (long long)vrow * RS + 8 * c);
        *reinterpret_cast<half8*>(vs + key * VP + 8 * c) = v;
      }
      f32x16 sacc;
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8*>(kp + 16 * ks), qf[ks], sacc, 0, 0, 0);
      float mx = -INFINITY;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (key > q || key >= L) sacc[e] = -INFINITY;
        mx = fmaxf(mx, sacc[e]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(m, mx);
      const float alpha = __expf(m - mnew);
      float ps = 0.f;
#pragma unroll
      for (int e = 0; e < 16; ++e) { const float p = __expf(sacc[e] - mnew); sacc[e] = p; ps += p; }
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = mnew;
      half8 pb[2];
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[s2][j] = (_Float16)sacc[8 * s2 + j];
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();   // the slab is written
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int e = 0; e < 16; ++e) o[f][e] *= alpha;
        const int dim = 32 * f + li;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          half8 va;
#pragma unroll
          for (int j = 0; j < 8; ++j) va[j] = vs[(16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3)) * VP + dim];
          o[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb[s2], o[f], 0, 0, 0);
        }
      }
    }
    if (q >= own && q < L) {
      const float inv = 1.0f / l;
      _Float16* op = out + ((long long)qrow * Hq + h) * D;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int e = 0; e < 16; ++e) op[32 * f + (e & 3) + 8 * (e >> 2) + 4 * hh] = (_Float16)(o[f][e] * inv);
    }
  }
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long rup(long long x, long long m) { return (x + m - 1) / m * m; }

// Workspace of a forward over `rows` rows with `hrows` head rows and `ints` index entries
struct LlamaLayout {
  size_t ints, resid, x16, qkv, hbuf, pmax, psum, tlogit, logp, total;
  long long Mp, ncg;
};

LlamaLayout llama_layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints) {
  LlamaLayout L{};
  const long long d = m->d_model, hd = d / m->n_heads, qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * hd;
  L.Mp = rup(rows > 0 ? rows : 1, ROWPAD); L.ncg = (m->vocab + 63) / 64;
  if (hrows < 0) hrows = 0;
  size_t off = 0;
  L.ints = off;   off += al256(sizeof(int) * ints);
  L.resid = off;  off += al256(sizeof(float) * (size_t)(rows * d));
  L.x16 = off;    off += al256(sizeof(_Float16) * (size_t)(L.Mp * d));
  L.qkv = off;    off += al256(sizeof(_Float16) * (size_t)(rows * qw));
  L.hbuf = off;   off += al256(sizeof(_Float16) * (size_t)(L.Mp * m->ffn_dim));
  L.pmax = off;   off += al256(sizeof(float) * (size_t)(hrows * L.ncg));
  L.psum = off;   off += al256(sizeof(float) * (size_t)(hrows * L.ncg));
  L.tlogit = off; off += al256(sizeof(float) * (size_t)hrows);
  L.logp = off;   off += al256(sizeof(float) * (size_t)hrows);
  L.total = off;
  return L;
}

LlamaLayout llama_flat_layout(const b2t_clm_llama_t* m, long long M, int n_seq) {
  const long long Mh = M - n_seq;
  return llama_layout(m, M, Mh, (size_t)(2 * M + 2 * (Mh > 0 ? Mh : 0) + 2 * ((long long)n_seq + 1)));
}

LlamaLayout llama_tree_layout(const b2t_clm_llama_t* m, long long Mn, long long M, int n_seq) {
  return llama_layout(m, Mn, Mn, tree_ints(Mn, M, n_seq));
}

// dimensions a descriptor must have for the sizes above to mean anything (the full check is clm_llama_check_model)
bool llama_dims_ok(const b2t_clm_llama_t* m) {
  return m && m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->n_kv_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 &&
         m->d_model % m->n_heads == 0;
}

int clm_llama_check_model(const b2t_clm_llama_t* m) {
  B2T_REQUIRE(m, "b2t_clm_llama: null model");
  B2T_REQUIRE(m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->n_kv_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 &&
              m->max_pos > 0,
              "b2t_clm_llama: bad dimensions (layers %d, d %d, heads %d, kv heads %d, ffn %d, vocab %d, max_pos %d)", m->n_layers,
              m->d_model, m->n_heads, m->n_kv_heads, m->ffn_dim, m->vocab, m->max_pos);
  B2T_REQUIRE(m->d_model % m->n_heads == 0, "b2t_clm_llama: d_model %d is not a multiple of n_heads %d", m->d_model, m->n_heads);
  const int hd = m->d_model / m->n_heads;
  B2T_REQUIRE(hd == 64 || hd == 128, "b2t_clm_llama: unsupported head dim %d (64 or 128)", hd);
  B2T_REQUIRE(m->n_heads % m->n_kv_heads == 0, "b2t_clm_llama: n_heads %d is not a multiple of n_kv_heads %d", m->n_heads,
              m->n_kv_heads);
  B2T_REQUIRE(m->d_model % 64 == 0 && m->ffn_dim % 64 == 0, "b2t_clm_llama: d_model %d and ffn_dim %d must be multiples of 64",
              m->d_model, m->ffn_dim);
  B2T_REQUIRE(m->rms_eps >= 0.f && m->rms_eps < 1.f, "b2t_clm_llama: rms_eps %g outside [0, 1)", (double)m->rms_eps);
  B2T_REQUIRE(m->embed_tokens && m->lm_head && m->final_norm_w && m->rope_cos && m->rope_sin && (m->n_layers == 0 || m->layers_host),
              "b2t_clm_llama: null weight pointer");
  for (int l = 0; l < m->n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m->layers_host[l];   // qkv_b may be null (no q / k / v biases)
    B2T_REQUIRE(w.norm1_w && w.norm2_w && w.qkv_w && w.o_w && w.gate_up_w && w.down_w,
                "b2t_clm_llama: null weight pointer in layer %d", l);
  }
  return 0;
}

// refusals of the two score calls that do not depend on the path
int llama_check_lists(const char* fn, const b2t_clm_llama_t& m, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                      const float* scores_out, const void* ws) {
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", fn);
  B2T_REQUIRE(n_seq >= 1, "%s: n_seq %d < 1", fn, n_seq);
  B2T_REQUIRE(seq_off_host[0] == 0, "%s: seq_off[0] = %d, expected 0", fn, seq_off_host[0]);
  for (int s = 0; s < n_seq; ++s) {
    const long long n = (long long)seq_off_host[s + 1] - seq_off_host[s];
    B2T_REQUIRE(n >= 1, "%s: sequence %d is empty", fn, s);
    B2T_REQUIRE(n <= m.max_pos, "%s: sequence %d has %lld tokens, more than max_pos %d", fn, s, n, m.max_pos);
  }
  const long long M = seq_off_host[n_seq];
  for (long long t = 0; t < M; ++t)
    B2T_REQUIRE(ids_host[t] >= 0 && ids_host[t] < m.vocab, "%s: token %lld has id %d outside [0, %d)", fn, t, ids_host[t], m.vocab);
  return 0;
}

struct LlamaRun {
  long long rows, Mh;          // rows of the forward; head rows
  const int *d_ids, *d_pos;    // [rows]
  const int *d_src, *d_tgt;    // [Mh] head source row and target id
};

// The forward over r.rows rows up to the per-row log-probs logp[Mh]; attn(qkv, out) enqueues one layer's attention.
template <class Attn>
int llama_forward(const b2t_clm_llama_t& m, const LlamaRun& r, const LlamaLayout& L, char* base, Attn&& attn, hipStream_t s) {
  const int d = m.d_model, Hq = m.n_heads, Hkv = m.n_kv_heads, hd = d / Hq, F = m.ffn_dim, qw = (Hq + 2 * Hkv) * hd;
  const long long rows = r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  _Float16* x16 = reinterpret_cast<_Float16*>(base + L.x16);
  _Float16* qkv = reinterpret_cast<_Float16*>(base + L.qkv);
  _Float16* hb = reinterpret_cast<_Float16*>(base + L.hbuf);
  auto H16 = [](const void* p) { return static_cast<const _Float16*>(p); };
  auto rmsnorm = [&](const int* rowmap, long long n, const void* w) {
    hipLaunchKernelGGL(clm_llama_rmsnorm_kernel, dim3((unsigned)rup(n, ROWPAD)), dim3(256), 0, s, resid, rowmap, (int)n, H16(w),
                       m.rms_eps, x16, d);
    B2T_CHECK_LAUNCH("clm_llama_rmsnorm_kernel");
    return 0;
  };
  hipLaunchKernelGGL(clm_llama_embed_kernel, dim3((unsigned)rows), dim3(256), 0, s, r.d_ids, H16(m.embed_tokens), resid, d);
  B2T_CHECK_LAUNCH("clm_llama_embed_kernel");
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_llama_layer_t& w = m.layers_host[l];
    if (int rc = rmsnorm(nullptr, rows, w.norm1_w)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = H16(w.qkv_w); g.M = (int)rows; g.N = qw; g.K = d; g.bias = H16(w.qkv_b); g.out16 = qkv; g.ldo = qw;
    g.qscale = 1.0f / sqrtf((float)hd); g.qcols = Hq * hd;
    g.pos = r.d_pos; g.rope_cos = m.rope_cos; g.rope_sin = m.rope_sin; g.rope_cols = (Hq + Hkv) * hd; g.hd = hd;
    if (int rc = launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE>)) return rc;
    if (int rc = attn(qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.o_w); g.M = (int)rows; g.N = d; g.K = d; g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
    if (int rc = rmsnorm(nullptr, rows, w.norm2_w)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.gate_up_w); g.M = (int)rows; g.N = 2 * F; g.K = d; g.out16 = hb; g.ldo = F;
    if (int rc = launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU>)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = H16(w.down_w); g.M = (int)rows; g.N = d; g.K = F; g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
  }
  if (r.Mh > 0) {
    if (int rc = rmsnorm(r.d_src, r.Mh, m.final_norm_w)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = H16(m.lm_head); g.M = (int)r.Mh; g.N = m.vocab; g.K = d;
    g.pmax = reinterpret_cast<float*>(base + L.pmax); g.psum = reinterpret_cast<float*>(base + L.psum);
    g.tlogit = reinterpret_cast<float*>(base + L.tlogit); g.tgt = r.d_tgt; g.ncg = (int)L.ncg;
    if (int rc = launch_gemm<EP_HEAD>(g, s)) return rc;
    if (int rc = clm_launch_head_combine(g.pmax, g.psum, g.tlogit, g.ncg, reinterpret_cast<float*>(base + L.logp), r.Mh, s))
      return rc;
  }
  return 0;
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_llama_ws_bytes(const b2t_clm_llama_t* model, long long n_tokens, int n_seq) {
  if (!llama_dims_ok(model) || n_tokens < 1 || n_seq < 1 || n_seq > n_tokens) return 0;
  return llama_flat_layout(model, n_tokens, n_seq).total;
}

extern "C" int b2t_clm_llama_score_f16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                       int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes,
                                       void* stream) {
  if (int rc = clm_llama_check_model(model)) return rc;
  const b2t_clm_llama_t& m = *model;
  if (int rc = llama_check_lists("b2t_clm_llama_score_f16", m, ids_host, seq_off_host, n_seq, scores_out, ws)) return rc;
  const long long M = seq_off_host[n_seq];
  const LlamaLayout L = llama_flat_layout(model, M, n_seq);
  B2T_REQUIRE(ws_bytes >= L.total, "b2t_clm_llama_score_f16: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  const long long Mh = M - n_seq;

  // index arrays, built on the host and uploaded once: ids[M] pos[M] head_src[Mh] head_tgt[Mh] seq_off[n+1] head_off[n+1]
  static thread_local std::vector<int> host;
  host.assign((size_t)(2 * M + 2 * Mh + 2 * (n_seq + 1)), 0);
  int* h_ids = host.data(); int* h_pos = h_ids + M; int* h_src = h_pos + M; int* h_tgt = h_src + Mh;
  int* h_soff = h_tgt + Mh; int* h_hoff = h_soff + n_seq + 1;
  long long r = 0;
  for (int q = 0; q < n_seq; ++q) {
    const int a = seq_off_host[q], b = seq_off_host[q + 1];
    h_soff[q] = a; h_hoff[q] = (int)r;
    for (int t = a; t < b; ++t) {
      h_ids[t] = ids_host[t]; h_pos[t] = t - a;
      if (t + 1 < b) { h_src[r] = t; h_tgt[r] = ids_host[t + 1]; ++r; }
    }
  }
  h_soff[n_seq] = (int)M; h_hoff[n_seq] = (int)r;
  char* base = static_cast<char*>(ws);
  int* d_ids = reinterpret_cast<int*>(base + L.ints);
  int* d_pos = d_ids + M; int* d_src = d_pos + M; int* d_tgt = d_src + Mh; int* d_soff = d_tgt + Mh; int* d_hoff = d_soff + n_seq + 1;
  if (int rc = check_hip(hipMemcpyAsync(d_ids, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s),
                         "b2t_clm_llama_score_f16 upload"))
    return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), "b2t_clm_llama_score_f16 upload")) return rc;

  const int Hq = m.n_heads, Hkv = m.n_kv_heads, hd = m.d_model / Hq;
  auto attn = [&](const _Float16* qkv, _Float16* out) {
    if (hd == 64) hipLaunchKernelGGL(clm_llama_attn_kernel<64>, dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, d_soff, Hq, Hkv);
    else hipLaunchKernelGGL(clm_llama_attn_kernel<128>, dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, d_soff, Hq, Hkv);
    B2T_CHECK_LAUNCH("clm_llama_attn_kernel");
    return 0;
  };
  const LlamaRun run{M, Mh, d_ids, d_pos, d_src, d_tgt};
  if (int rc = llama_forward(m, run, L, base, attn, s)) return rc;
  return clm_launch_seq_sum(reinterpret_cast<float*>(base + L.logp), d_soff, d_hoff, scores_out, tok_logp_out, n_seq, s);
}

extern "C" size_t b2t_clm_llama_tree_ws_bytes(const b2t_clm_llama_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  if (!llama_dims_ok(model) || n_nodes < 1 || n_nodes > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  return llama_tree_layout(model, n_nodes, n_tokens, n_seq).total;
}

extern "C" int b2t_clm_llama_score_tree_f16(const b2t_clm_llama_t* model, const int32_t* ids_host, const int32_t* seq_off_host,
                                            int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws,
                                            size_t ws_bytes, void* stream) {
  if (int rc = clm_llama_check_model(model)) return rc;
  const b2t_clm_llama_t& m = *model;
  if (int rc = llama_check_lists("b2t_clm_llama_score_tree_f16", m, ids_host, seq_off_host, n_seq, scores_out, ws)) return rc;
  const long long M = seq_off_host[n_seq];

  // the plan, then the index arrays in upload order (tree_ints): node_id[Mn] node_pos[Mn] head_src[Mn] head_tgt[Mn] (Mh used)
  // tok_node[M] tok_hrow[M] seq_off[n+1] own_start[n].  A node's rotary position is its depth, node_pos.
  static thread_local std::vector<int32_t> tok_node, parent, own, host;
  tok_node.resize((size_t)M); parent.resize((size_t)M); own.resize((size_t)n_seq);
  const long long Mn = tree_plan(ids_host, seq_off_host, n_seq, tok_node.data(), parent.data(), M, own.data());
  if (n_nodes_out) *n_nodes_out = Mn;
  const LlamaLayout L = llama_tree_layout(model, Mn, M, n_seq);
  B2T_REQUIRE(ws_bytes >= L.total, "b2t_clm_llama_score_tree_f16: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);

  host.assign(tree_ints(Mn, M, n_seq), 0);
  int* h_id = host.data(); int* h_pos = h_id + Mn; int* h_src = h_pos + Mn; int* h_tgt = h_src + Mn;
  int* h_node = h_tgt + Mn; int* h_hrow = h_node + M; int* h_soff = h_hrow + M; int* h_own = h_soff + n_seq + 1;
  for (int q = 0; q < n_seq; ++q) {
    const int a = seq_off_host[q], b = seq_off_host[q + 1];
    h_soff[q] = a; h_own[q] = own[q];
    for (int t = a; t < b; ++t) {
      const int n = tok_node[t];
      h_node[t] = n; h_id[n] = ids_host[t]; h_pos[n] = t - a;
    }
  }
  h_soff[n_seq] = (int)M;
  long long Mh = 0;   // head rows: the non-root nodes in node order, source = the parent's row, target = the node's id
  {
    std::vector<int32_t>& hrow = parent;   // parent[n] is read before hrow[n] is written
    for (long long n = 0; n < Mn; ++n) {
      const int p = parent[n];
      if (p >= 0) { h_src[Mh] = p; h_tgt[Mh] = h_id[n]; hrow[n] = (int32_t)Mh++; }
      else hrow[n] = 0;
    }
    for (long long t = 0; t < M; ++t) h_hrow[t] = hrow[tok_node[t]];
  }
  char* base = static_cast<char*>(ws);
  int* d_id = reinterpret_cast<int*>(base + L.ints);
  int* d_pos = d_id + Mn; int* d_src = d_pos + Mn; int* d_tgt = d_src + Mn; int* d_node = d_tgt + Mn; int* d_hrow = d_node + M;
  int* d_soff = d_hrow + M; int* d_own = d_soff + n_seq + 1;
  if (int rc = check_hip(hipMemcpyAsync(d_id, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s),
                         "b2t_clm_llama_score_tree_f16 upload"))
    return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), "b2t_clm_llama_score_tree_f16 upload")) return rc;

  const int Hq = m.n_heads, Hkv = m.n_kv_heads, hd = m.d_model / Hq;
  auto attn = [&](const _Float16* qkv, _Float16* out) {
    if (hd == 64)
      hipLaunchKernelGGL(clm_llama_attn_tree_kernel<64>, dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, d_soff, d_node, d_own, Hq, Hkv);
    else
      hipLaunchKernelGGL(clm_llama_attn_tree_kernel<128>, dim3(n_seq, Hq), dim3(256), 0, s, qkv, out, d_soff, d_node, d_own, Hq, Hkv);
    B2T_CHECK_LAUNCH("clm_llama_attn_tree_kernel");
    return 0;
  };
  const LlamaRun run{Mn, Mh, d_id, d_pos, d_src, d_tgt};
  if (int rc = llama_forward(m, run, L, base, attn, s)) return rc;
  return clm_launch_seq_sum_tree(reinterpret_cast<float*>(base + L.logp), d_soff, d_hrow, scores_out, tok_logp_out, n_seq, s);
}
