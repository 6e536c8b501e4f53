// causal_lm.hip — scoring-only OPT decoder forward (the n-best rescoring LLM of language-model-standalone.py:127-162) for gfx950.
// Input: packed variable-length sequences (token ids + per-sequence offsets; no padding, no KV cache).  Output: per sequence the
// sum over t = 1..n-1 of log p(id[t] | id[0..t-1]), and optionally every per-token log-prob.
//
// Numerics contract:
//   - weights are stored fp16 (as the checkpoint and the reference's torch_dtype=float16 hold them);
//   - GEMM operands are fp16, accumulation fp32 (v_mfma_f32_32x32x16_f16);
//   - the residual stream, LayerNorm statistics, softmax / log-softmax and the per-sequence sums are fp32;
//   - the LayerNorm, attention and fc1 outputs (the next GEMM's operands) and q / k / v are rounded to fp16, and so are the
//     attention's probabilities exp(s - m) per 32-key block, m the running maximum, as the P.V operand (its normaliser sums
//     them unrounded).
//   Every output element is computed by one thread in a fixed order that depends only on its own row: a sequence's score is
//   bit-identical alone or anywhere in any batch.
//
// Kernels, per layer (pre-LN OPT): LayerNorm -> QKV GEMM (+bias, q * head_dim^-0.5, fp16) -> causal attention -> out_proj GEMM
// (+bias, added into the fp32 residual) -> LayerNorm -> fc1 GEMM (+bias, ReLU, fp16) -> fc2 GEMM (+bias, residual add).  Then the
// final LayerNorm of every position but the last of each sequence, and the LM head (tied to embed_tokens) fused with
// log-softmax and the gather: the tile epilogue emits per (row, 64-column group) the max and the sum of exp, and the logit of
// the row's target token; a combine kernel forms logp = logit[target] - logsumexp.  The [tokens x vocab] logits never exist.
//
// GEMM: the packed tile design of gemm_bf16p.hip (k-contiguous operands read as 16-byte rows straight into double-buffered
// LDS with 144-byte rows, one barrier per 64-k tile) as a sibling fp16 kernel, 128 x 128 (4 waves) and 256 x 256 (8 waves)
// tiles.  Operands are never packed at run time: the LayerNorm / attention / fc1 kernels write the k-contiguous, row-padded
// fp16 A operand directly, and nn.Linear weights ([N][K], k-contiguous) are padded once at load time to 256 rows.
//
// The host-side pieces the other paths (causal_lm_tree.hip, causal_lm_cache.hip, causal_lm_llama.hip) reuse -- launch_gemm,
// the embed / LayerNorm / attention / head launchers, clm_check_model, the list check, the workspace layout and the flat
// index builder -- have external linkage and are declared in clm_internal.h, which also holds the layer loop (clm_forward),
// this descriptor's family (OptFamily) and the bodies of the entry points and the size rules of every family (GPT-2,
// causal_lm_gpt2.hip, enters them with a policy of its own for the fc1 launcher).
// The kernels stay private to this file: the GEMM's template is clm_gemm.h, instantiated here for the four epilogues of this
// forward; the attention's arithmetic and clm_attn_kernel itself are clm_attn.h's templates (instantiated here in fp16 for
// head dims 64, 80 and 128, behind clm_launch_attn), and the kernel serves the Llama family's row layout too.
#include <math.h>
#include <vector>

#include "clm_attn.h"
#include "clm_gemm.h"

namespace b2t {

// B2T_CLM_GEMM_256 (read on every call): 0 = 128 x 128 tiles always, 1 or unset = 256 x 256 tiles where they fill the chip,
// 2 = 256 x 256 tiles always.  Both kernels give bit-identical results (same k order per output element); every A operand and
// weight is padded to ROWPAD = 256 rows, so either tile reads inside its buffers at any M and N.  The rule is here alone:
// `tiles` is the caller's instantiation of clm_gemm_tiles (clm_gemm.h) for its epilogue.
int launch_gemm(const ClmGemm& g, hipStream_t s, ClmGemmTiles tiles) {
  const char* e = getenv("B2T_CLM_GEMM_256");
  const int mode = e ? atoi(e) : 1;
  const int m256 = (g.M + 255) / 256, n256 = (g.N + 255) / 256;
  // the 256-tiles fill the chip's 256 CUs: one 8-wave workgroup per CU
  return tiles(g, s, mode == 2 || (mode != 0 && (long long)m256 * n256 >= 256));
}
template <int EP>
int launch_gemm(const ClmGemm& g, hipStream_t s) {
  return launch_gemm(g, s, &clm_gemm_tiles<EP>);
}
template int launch_gemm<EP_F16>(const ClmGemm&, hipStream_t);
template int launch_gemm<EP_RELU>(const ClmGemm&, hipStream_t);
template int launch_gemm<EP_RESID>(const ClmGemm&, hipStream_t);
template int launch_gemm<EP_HEAD>(const ClmGemm&, hipStream_t);

namespace {

__device__ __forceinline__ float block_max256(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// resid[t] = embed_tokens[id[t]] + embed_positions[pos[t] + 2] (fp32)
__global__ __launch_bounds__(256) void clm_embed_kernel(const int* ids, const int* pos, const _Float16* et, const _Float16* ep,
                                                        float* resid, int d) {
  const int t = blockIdx.x;
  const _Float16* a = et + (long long)ids[t] * d;
  const _Float16* b = ep + (long long)(pos[t] + 2) * d;
  float* o = resid + (long long)t * d;
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (float)a[c] + (float)b[c];
}

// out[r] = fp16(LayerNorm(x[rowmap ? rowmap[r] : r])) for r < rows; zeros for rows <= r < gridDim.x (the operand's padding)
__global__ __launch_bounds__(256) void clm_layernorm_kernel(const float* x, const int* rowmap, int rows, const _Float16* w,
                                                            const _Float16* b, _Float16* out, int d) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  _Float16* o = out + (long long)r * d;
  if (r >= rows) {
    for (int c = threadIdx.x; c < d; c += 256) o[c] = (_Float16)0.f;
    return;
  }
  const float* xr = x + (long long)(rowmap ? rowmap[r] : r) * d;
  float s = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) s += xr[c];
  const float mean = block_sum256(s, red) / d;
  float v = 0.f;
  for (int c = threadIdx.x; c < d; c += 256) { const float q = xr[c] - mean; v += q * q; }
  const float rstd = 1.0f / sqrtf(block_sum256(v, red) / d + 1e-5f);
  for (int c = threadIdx.x; c < d; c += 256) o[c] = (_Float16)((xr[c] - mean) * rstd * (float)w[c] + (float)b[c]);
}

// logp[r] = tlogit[r] - logsumexp over the row's 64-column groups
__global__ __launch_bounds__(256) void clm_head_combine_kernel(const float* pmax, const float* psum, const float* tlogit, int ncg,
                                                               float* logp) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  const float* pm = pmax + (long long)r * ncg;
  const float* ps = psum + (long long)r * ncg;
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < ncg; c += 256) mx = fmaxf(mx, pm[c]);
  mx = block_max256(mx, red);
  float s = 0.f;
  for (int c = threadIdx.x; c < ncg; c += 256) s += ps[c] * expf(pm[c] - mx);
  s = block_sum256(s, red);
  if (threadIdx.x == 0) logp[r] = tlogit[r] - (mx + logf(s));
}

// scores[s] = sum of the sequence's log-probs in token order; tok_logp (optional) = per token, 0 at each sequence's first token
__global__ __launch_bounds__(64) void clm_seq_sum_kernel(const float* logp, const int* seq_off, const int* head_off, float* scores,
                                                         float* tok_logp) {
  const int s = blockIdx.x, h0 = head_off[s], n = head_off[s + 1] - h0, t0 = seq_off[s];
  if (tok_logp) {
    if (threadIdx.x == 0) tok_logp[t0] = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) tok_logp[t0 + 1 + i] = logp[h0 + i];
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc += logp[h0 + i];
    scores[s] = acc;
  }
}

}  // namespace

int clm_check_model(const b2t_clm_t* m) {
  const char* pre = "b2t_clm";
  if (int rc = clm_check_mha_dims(pre, m)) return rc;
  const int hd = m->d_model / m->n_heads;
  B2T_REQUIRE(hd == 64 || hd == 80 || hd == 128, "b2t_clm: unsupported head dim %d (64, 80 or 128)", hd);
  if (int rc = clm_check_mult64(pre, m->d_model, m->ffn_dim)) return rc;
  B2T_REQUIRE(m->embed_tokens && m->embed_positions && m->final_ln_w && m->final_ln_b && (m->n_layers == 0 || m->layers_host),
              "b2t_clm: null weight pointer");
  for (int l = 0; l < m->n_layers; ++l)
    if (int rc = clm_check_mha_layer(pre, m->layers_host[l], l)) return rc;
  return 0;
}

// the launchers clm_internal.h declares, used below and by the tree path (causal_lm_tree.hip)
int clm_launch_embed(const int* ids, const int* pos, const _Float16* et, const _Float16* ep, float* resid, int d, long long rows,
                     hipStream_t s) {
  hipLaunchKernelGGL(clm_embed_kernel, dim3((unsigned)rows), dim3(256), 0, s, ids, pos, et, ep, resid, d);
  B2T_CHECK_LAUNCH("clm_embed_kernel");
  return 0;
}

int clm_launch_layernorm(const float* x, const int* rowmap, long long rows, const _Float16* w, const _Float16* b, _Float16* out,
                         int d, hipStream_t s) {
  hipLaunchKernelGGL(clm_layernorm_kernel, dim3((unsigned)rup(rows, ROWPAD)), dim3(256), 0, s, x, rowmap, (int)rows, w, b, out, d);
  B2T_CHECK_LAUNCH("clm_layernorm_kernel");
  return 0;
}

int clm_launch_head_combine(const float* pmax, const float* psum, const float* tlogit, int ncg, float* logp, long long rows,
                            hipStream_t s) {
  hipLaunchKernelGGL(clm_head_combine_kernel, dim3((unsigned)rows), dim3(256), 0, s, pmax, psum, tlogit, ncg, logp);
  B2T_CHECK_LAUNCH("clm_head_combine_kernel");
  return 0;
}

int clm_launch_seq_sum(const float* logp, const int* seq_off, const int* head_off, float* scores, float* tok_logp, int n_seq,
                       hipStream_t s) {
  hipLaunchKernelGGL(clm_seq_sum_kernel, dim3(n_seq), dim3(64), 0, s, logp, seq_off, head_off, scores, tok_logp);
  B2T_CHECK_LAUNCH("clm_seq_sum_kernel");
  return 0;
}

int clm_launch_attn(const _Float16* qkv, _Float16* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  const dim3 grid(n_seq, Hq);
  if (hd == 64) hipLaunchKernelGGL(clm_attn_kernel<64>, grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);
  else if (hd == 80) hipLaunchKernelGGL(clm_attn_kernel<80>, grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);
  else hipLaunchKernelGGL(clm_attn_kernel<128>, grid, dim3(256), 0, s, qkv, out, seq_off, Hq, Hkv);
  B2T_CHECK_LAUNCH("clm_attn_kernel");
  return 0;
}

ClmLayout clm_layout(int d_model, long long qkv_width, int ffn, int vocab, long long rows, long long head_rows, size_t ints) {
  ClmLayout L{};
  const long long d = d_model, Mh = head_rows > 0 ? head_rows : 0;
  L.Mp = rup(rows > 0 ? rows : 1, ROWPAD); L.ncg = (vocab + 63) / 64;
  size_t off = 0;
  L.ints = off;   off += al256(sizeof(int) * ints);
  L.resid = off;  off += al256(sizeof(float) * (size_t)(rows * d));
  L.x16 = off;    off += al256(sizeof(_Float16) * (size_t)(L.Mp * d));
  L.qkv = off;    off += al256(sizeof(_Float16) * (size_t)(rows * qkv_width));
  L.hbuf = off;   off += al256(sizeof(_Float16) * (size_t)(L.Mp * ffn));
  L.pmax = off;   off += al256(sizeof(float) * (size_t)(Mh * L.ncg));
  L.psum = off;   off += al256(sizeof(float) * (size_t)(Mh * L.ncg));
  L.tlogit = off; off += al256(sizeof(float) * (size_t)Mh);
  L.logp = off;   off += al256(sizeof(float) * (size_t)Mh);
  L.total = off;
  return L;
}

size_t flat_ints(long long M, int n_seq) {
  const long long Mh = M - n_seq;
  return (size_t)(2 * M + 2 * (Mh > 0 ? Mh : 0) + 2 * ((long long)n_seq + 1));
}

int clm_check_lists(const char* who, const int32_t* ids, const int32_t* seq_off, int n_seq, int vocab, int max_pos) {
  B2T_REQUIRE(n_seq >= 1, "%s: n_seq %d < 1", who, n_seq);
  B2T_REQUIRE(seq_off[0] == 0, "%s: seq_off[0] = %d, expected 0", who, seq_off[0]);
  for (int s = 0; s < n_seq; ++s) {
    const long long n = (long long)seq_off[s + 1] - seq_off[s];
    B2T_REQUIRE(n >= 1, "%s: sequence %d is empty", who, s);
    B2T_REQUIRE(max_pos <= 0 || n <= max_pos, "%s: sequence %d has %lld tokens, more than max_pos %d", who, s, n, max_pos);
  }
  if (vocab > 0) {
    const long long M = seq_off[n_seq];
    for (long long t = 0; t < M; ++t)
      B2T_REQUIRE(ids[t] >= 0 && ids[t] < vocab, "%s: token %lld has id %d outside [0, %d)", who, t, ids[t], vocab);
  }
  return 0;
}

int clm_build_flat_index(const char* what, const int32_t* ids, const int32_t* seq_off, int n_seq, int* d_ints, hipStream_t s,
                         ClmFlatIndex* ix) {
  const long long M = seq_off[n_seq], Mh = M - n_seq;
  static thread_local std::vector<int> host;
  host.assign(flat_ints(M, n_seq), 0);
  int* h_ids = host.data(); int* h_pos = h_ids + M; int* h_src = h_pos + M; int* h_tgt = h_src + Mh;
  int* h_soff = h_tgt + Mh; int* h_hoff = h_soff + n_seq + 1;
  long long r = 0;
  for (int q = 0; q < n_seq; ++q) {
    const int a = seq_off[q], b = seq_off[q + 1];
    h_soff[q] = a; h_hoff[q] = (int)r;
    for (int t = a; t < b; ++t) {
      h_ids[t] = ids[t]; h_pos[t] = t - a;
      if (t + 1 < b) { h_src[r] = t; h_tgt[r] = ids[t + 1]; ++r; }
    }
  }
  h_soff[n_seq] = (int)M; h_hoff[n_seq] = (int)r;
  if (int rc = check_hip(hipMemcpyAsync(d_ints, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s), what)) return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), what)) return rc;
  const int* d_src = d_ints + 2 * M;
  *ix = ClmFlatIndex{{M, Mh, d_ints, d_ints + M, d_src, d_src + Mh}, d_src + 2 * Mh, d_src + 2 * Mh + n_seq + 1};
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_ws_bytes(const b2t_clm_t* model, long long n_tokens, int n_seq) {
  return clm_family_ws_bytes<OptFamily>(model, n_tokens, n_seq);
}

extern "C" int b2t_clm_score_f16(const b2t_clm_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                 float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score<OptPolicy, OptFamily>("b2t_clm_score_f16", model, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                ws, ws_bytes, stream);
}
