// clm_internal.h — what the units of the causal-LM forward share, for every family and both element types: the epilogue names
// and the GEMM's arguments, the declarations of the launchers, the layout, the list check, the plan and the index builders that
// causal_lm.hip, causal_lm_tree.hip and causal_lm_cache.hip define, the family-independent body of a cached call
// (clm_score_tree_cached), and at the end the family contract with the bodies of the flat, the tree and the cached entry point and
// the size rules that every family's exported functions are one call of.  The OPT forward (clm_forward) and its family are
// here too; GPT-NeoX's is in its unit, the Llama-derived families' are in clm_llama.h and the headers beside it.  This header
// holds no kernel: kernels stay private to their units (the attention's templates are clm_attn.h's, the GEMM's clm_gemm.h's).  All attention launchers
// serve every family: OPT's row q[d] | k[d] | v[d] is the Llama row q[Hq * D] | k[Hkv * D] | v[Hkv * D] with Hkv = Hq.
#pragma once
#include <math.h>
#include <string>
#include <vector>

#include "common.h"

namespace b2t {

constexpr int CLM_ROWPAD = 256;   // A operands and weights are padded to this many rows

// EP_ROPE and EP_SWIGLU (the Llama family) pair the two 32-column halves of a wave's 64-column slice in one lane:
//   EP_ROPE   out16[r][c], out16[r][c + 32] = the rotation of (C[r][c], C[r][c + 32]) + bias by the angle of row r's position
//             and frequency (c % hd) / 2 + c % 32 (columns < rope_cols; the others are written as EP_F16 writes them);
//   EP_SWIGLU out16[r][c0 / 2 + i] = silu(C[r][c0 + i]) * C[r][c0 + 32 + i], c0 a multiple of 64, i < 32 (ldo = N / 2).
// EP_QKNORM_ROPE (Qwen3) is EP_ROPE without a bias and with an RMSNorm over every q and k head of a row in front of the rotation:
//   x[c] * rsqrt(mean over the head of x^2 + rms_eps) * w[c % hd], w = qnorm_w (columns < qcols) or knorm_w (< rope_cols).
// EP_GELU (GPT-2) is EP_RELU with gelu_new in ReLU's place: out16[r][c] = gelu_new(C[r][c] + bias[c]), gelu_new(v) =
//   0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3))) in fp32, rounded once.
// EP_ROPE_PART (GPT-NeoX) is EP_ROPE with only the first rotary_ndims = 2 * rope_half dims of a head rotated: the loader stores a
//   head so that in the 64-column slice at 32 * j rows of rope_half the lanes li < clamp(rope_half - 32 j, 0, 32) hold a rotary
//   pair (frequency 32 j + li) in their two fragments and the other lanes two pass-through columns; the table's row stride is
//   rope_half.  Bias, rotation or pass-through, the q scale, one rounding, as in EP_ROPE.
// EP_GELU_ERF (GPT-NeoX) is EP_GELU with the erf form: gelu(v) = 0.5 v (1 + erf(v / sqrt 2)) in fp32, rounded once.
// EP_F32 (OLMo-2) stores the fp32 accumulator unrounded: resid[r][c] = C[r][c] (`=`, no bias; pitch ldo) -- the o_proj and down
//   outputs, whose whole row a post-norm reads before anything reaches the residual.
// EP_QKV_F32 (OLMo-2, Phi-3) splits the QKV row: columns < rope_cols (q | k) are stored as EP_F32 stores them, resid[r][c] with
//   pitch rope_cols, for the whole-row q / k norm that no column tile can hold (Phi-3: for the rotation of heads of 96 dims);
//   the others (v) are rounded once, out16[r][c] (pitch ldo).
// EP_GEGLU (Gemma-2) is EP_SWIGLU with gelu_new in silu's place: out16[r][c0 / 2 + i] = gelu_new(C[r][c0 + i]) * C[r][c0 + 32 + i].
// EP_HEAD_CAP (Gemma-2) is EP_HEAD on soft-capped logits: v = cap * tanh(C[r][c] / cap) in fp32 (tanh written as gelu_new's) in
//   front of the group max, the group sum and the target pick; cap > 0.
// EP_OSS_GLU (gpt-oss) is EP_SWIGLU with the bias of the two columns and the family's clamped activation: g = min(C[r][c0 + i] +
//   bias[c0 + i], limit), u = clamp(C[r][c0 + 32 + i] + bias[c0 + 32 + i], -limit, limit), out16[r][c0 / 2 + i] =
//   (u + 1) * g * (1 / (1 + exp(-1.702 g))) in fp32, rounded once; a saturated g gives g or -0, never inf / inf.
// EP_F32_BIAS (gpt-oss) is EP_F32 with the bias added to the accumulator: resid[r][c] = C[r][c] + bias[c], unrounded.
//   In the grouped kernel both take the bias of the tile's expert, bias + expert * bias_stride.
enum { EP_F16 = 0, EP_RELU = 1, EP_RESID = 2, EP_HEAD = 3, EP_ROPE = 4, EP_SWIGLU = 5, EP_QKNORM_ROPE = 6, EP_GELU = 7,
       EP_ROPE_PART = 8, EP_GELU_ERF = 9, EP_F32 = 10, EP_QKV_F32 = 11, EP_GEGLU = 12, EP_HEAD_CAP = 13,
       EP_OSS_GLU = 14, EP_F32_BIAS = 15 };

using f32x16 = float __attribute__((ext_vector_type(16)));

// The element type E of a forward's 16-bit operands: _Float16 (every fp16 entry point, and the default of every template
// below and in clm_gemm.h / clm_attn.h) or __bf16 (causal_lm_llama_bf16.hip).  Both are 2 bytes, and the two MFMAs have one
// shape, operand lane layout and issue rate, so LDS images, workspace sizes and the tile rule do not depend on E.
template <class E> struct ClmElem;
template <> struct ClmElem<_Float16> {
  using v8 = _Float16 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
};
template <> struct ClmElem<__bf16> {
  using v8 = __bf16 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(v8 a, v8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
};

// A, B, bias and out16 hold elements of the launched kernel's element type (clm_gemm_kernel's E).
struct ClmGemm {
  const void* A;          // [round_up(M, 256)][K]
  const void* B;          // [round_up(N, 256)][K]
  int M, N, K;            // K % 64 == 0
  const void* bias;       // [N] or null
  void* out16;            // EP_F16 / EP_RELU: [M][ldo]
  float* resid;           // EP_RESID: [M][ldo] += C; EP_F32: [M][ldo] = C; EP_QKV_F32: [M][rope_cols] = C's q | k columns
  int ldo;
  float qscale; int qcols;   // EP_F16: columns < qcols are multiplied by qscale after the bias (OPT's q scaling)
  float* pmax; float* psum;  // EP_HEAD: [M][ncg] per 64-column group max / sum exp(v - max)
  float* tlogit; const int* tgt; int ncg;   // EP_HEAD: tlogit[r] = C[r][tgt[r]]
  const int* pos;                           // EP_ROPE: [M] position of each row
  const float* rope_cos; const float* rope_sin;   // EP_ROPE: fp32 [max_pos][hd / 2]
  int rope_cols, hd;                        // EP_ROPE: columns < rope_cols (q | k) are rotated; head dim (a multiple of 64)
  const void* qnorm_w; const void* knorm_w; // EP_QKNORM_ROPE: [hd] weights of the q heads' and the k heads' RMSNorm
  float rms_eps;                            // EP_QKNORM_ROPE
  int rope_half;                            // EP_ROPE_PART: rotary_ndims / 2, the row stride of rope_cos / rope_sin (hd/8, hd/4 or hd/2)
  // the grouped kernel only (clm_gemm_grouped_kernel; the routed experts of clm_moe.h): M is a multiple of 256
  const int* blk_expert;                    // [M / 128] the matrix of B that the 128-row block of A multiplies, -1: no rows, no tile
  long long b_stride;                       // elements between two consecutive matrices of B
  float cap;                                // EP_HEAD_CAP: the soft cap on the logits (> 0)
  long long bias_stride;                    // grouped EP_OSS_GLU / EP_F32_BIAS: elements between two consecutive experts' biases
  float glu_limit;                          // EP_OSS_GLU: the clamp on gate (from above) and up (both sides), > 0
  // the packed grouped kernel only (clm_gemm_grouped_mx_kernel): B is MXFP4 nibbles, K / 2 bytes a row, low nibble first
  const void* b_scale;                      // E8M0 scale bytes, K / 32 a row, in the rows and strides of B
  // the packed plain kernel only (clm_gemm_fp8_kernel): B is e4m3fn codes, K bytes a row, and b_scale fp32
  // [round_up(N, 256) / 32][K / b_block_k], the scale of 32 stored rows by b_block_k columns
  int b_block_k;                            // a multiple of 64 that divides K
};

// The tile rule (B2T_CLM_GEMM_256) lives in one definition, causal_lm.hip: it picks the tile and hands the launch to `tiles`,
// the caller's instantiation of clm_gemm_tiles<EP> (clm_gemm.h).  The template form is instantiated in causal_lm.hip for the
// four epilogues of the OPT forward.
typedef int (*ClmGemmTiles)(const ClmGemm& g, hipStream_t s, bool use256);
int launch_gemm(const ClmGemm& g, hipStream_t s, ClmGemmTiles tiles);
template <int EP>
int launch_gemm(const ClmGemm& g, hipStream_t s);
extern template int launch_gemm<EP_F16>(const ClmGemm&, hipStream_t);
extern template int launch_gemm<EP_RELU>(const ClmGemm&, hipStream_t);
extern template int launch_gemm<EP_RESID>(const ClmGemm&, hipStream_t);
extern template int launch_gemm<EP_HEAD>(const ClmGemm&, hipStream_t);
// the EP_GELU GEMM through the tile rule, for the families whose fc1 has the tanh GELU (causal_lm_gpt2.hip instantiates it)
int clm_gemm_gelu(const ClmGemm& g, hipStream_t s);

// resid[r] = embed_tokens[ids[r]] + embed_positions[pos[r] + 2] for r < rows
int clm_launch_embed(const int* ids, const int* pos, const _Float16* et, const _Float16* ep, float* resid, int d, long long rows,
                     hipStream_t s);
// out[r] = fp16(LayerNorm(x[rowmap ? rowmap[r] : r])) for r < rows, zeros for rows <= r < round_up(rows, 256)
int clm_launch_layernorm(const float* x, const int* rowmap, long long rows, const _Float16* w, const _Float16* b, _Float16* out,
                         int d, hipStream_t s);
// logp[r] = tlogit[r] - logsumexp over the row's 64-column groups, r < rows
int clm_launch_head_combine(const float* pmax, const float* psum, const float* tlogit, int ncg, float* logp, long long rows,
                            hipStream_t s);
// scores[q] = sum of logp[head_off[q] .. head_off[q + 1]) in order; tok_logp (optional) per packed token, 0 at first tokens
int clm_launch_seq_sum(const float* logp, const int* seq_off, const int* head_off, float* scores, float* tok_logp, int n_seq,
                       hipStream_t s);
// dimensions, head dim and weight pointers of a model descriptor (0, or an error with the message set)
int clm_check_model(const b2t_clm_t* m);
// The statements the checks of the two descriptors with one head count share (M: b2t_clm_t, clm_check_model, or b2t_clm_neox_t,
// causal_lm_neox.hip), `pre` being the prefix of their messages; the head-dim set, the extras and the order stay with the check.
template <class M>
int clm_check_mha_dims(const char* pre, const M* m) {
  B2T_REQUIRE(m, "%s: null model", pre);
  B2T_REQUIRE(m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 && m->max_pos > 0,
              "%s: bad dimensions (layers %d, d %d, heads %d, ffn %d, vocab %d, max_pos %d)", pre, m->n_layers, m->d_model,
              m->n_heads, m->ffn_dim, m->vocab, m->max_pos);
  B2T_REQUIRE(m->d_model % m->n_heads == 0, "%s: d_model %d is not a multiple of n_heads %d", pre, m->d_model, m->n_heads);
  return 0;
}
inline int clm_check_mult64(const char* pre, int d_model, int ffn_dim) {
  B2T_REQUIRE(d_model % 64 == 0 && ffn_dim % 64 == 0, "%s: d_model %d and ffn_dim %d must be multiples of 64", pre, d_model, ffn_dim);
  return 0;
}
// layer l's twelve pointers
inline int clm_check_mha_layer(const char* pre, const b2t_clm_layer_t& w, int l) {
  B2T_REQUIRE(w.ln1_w && w.ln1_b && w.qkv_w && w.qkv_b && w.out_w && w.out_b && w.ln2_w && w.ln2_b && w.fc1_w && w.fc1_b &&
              w.fc2_w && w.fc2_b, "%s: null weight pointer in layer %d", pre, l);
  return 0;
}
// dimensions such a descriptor must have for the sizes of its layout to mean anything (the full check is the family's check)
template <class M>
bool clm_mha_dims_ok(const M* m) {
  return m && m->n_layers >= 0 && m->d_model > 0 && m->n_heads > 0 && m->ffn_dim > 0 && m->vocab > 0 && m->d_model % m->n_heads == 0;
}

// ---- sizes ----
inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long rup(long long x, long long m) { return (x + m - 1) / m * m; }

// sum of v over a 256-thread block (red: 4 floats of LDS); every thread gets the same value
static __device__ __forceinline__ float block_sum256(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// Workspace of a forward over `rows` rows (qkv_width fp16 per row of the QKV GEMM's output) with `head_rows` head rows and
// `ints` index entries.  The tree paths size the head by their rows (it has at most a row per computed row).
struct ClmLayout {
  size_t ints, resid, x16, qkv, hbuf, pmax, psum, tlogit, logp, total;
  long long Mp, ncg;
};
ClmLayout clm_layout(int d_model, long long qkv_width, int ffn, int vocab, long long rows, long long head_rows, size_t ints);
// ints of the flat index arrays: ids[M] pos[M] head_src[Mh] head_tgt[Mh] seq_off[n+1] head_off[n+1], Mh = M - n_seq
size_t flat_ints(long long M, int n_seq);
// ints of the tree index arrays: row_id[rows] row_pos[rows] head_src[rows] head_tgt[rows] (Mh used) tok_node[M] tok_hrow[M]
// seq_off[n+1] own_start[n]
size_t tree_ints(long long rows, long long M, int n_seq);

// ---- the lists ----
// Refusals of a packed list: n_seq < 1, seq_off[0] != 0, an empty sequence, one longer than max_pos (max_pos > 0), an id
// outside [0, vocab) (vocab > 0).  `who` is the entry point's name.
int clm_check_lists(const char* who, const int32_t* ids, const int32_t* seq_off, int n_seq, int vocab, int max_pos);

// the rows of a forward and their index arrays on the device
struct ClmRun {
  long long rows, Mh;          // rows of the forward; head rows
  const int *d_ids, *d_pos;    // [rows] token id and position
  const int *d_src, *d_tgt;    // [Mh] head source row and target id
};
struct ClmFlatIndex { ClmRun run; const int *d_soff, *d_hoff; };
struct ClmTreeIndex { ClmRun run; const int *d_node, *d_hrow, *d_soff, *d_own; };
// Builds the flat index arrays on the host, uploads them to d_ints (flat_ints entries) and waits for the copy; `what` names
// the upload in an error.
int clm_build_flat_index(const char* what, const int32_t* ids, const int32_t* seq_off, int n_seq, int* d_ints, hipStream_t s,
                         ClmFlatIndex* ix);

// The shared-prefix plan: tok_node gets all n_tokens entries; parent_of_node (and own_start, optional, per sequence) only
// below cap.  Returns the number of nodes.
long long tree_plan(const int32_t* ids, const int32_t* seq_off, int n_seq, int32_t* node_of_token, int32_t* parent_of_node,
                    long long cap, int32_t* own_start);
struct ClmTreePlan { std::vector<int32_t> tok_node, parent, own; long long Mn; };
// the plan of a checked list in this thread's buffers, valid until the thread's next call
ClmTreePlan& clm_plan_tree(const int32_t* ids, const int32_t* seq_off, int n_seq);
// The tree index arrays over the computed rows, node n >= R being row n - R (R = 0: every node; R > 0: the first R nodes are
// a context cache's, causal_lm_cache.hip).  Head rows are the non-root nodes > R in node order, source = the parent's row,
// target = the node's id.  Uploads to d_ints (tree_ints(Mn - R, ..) entries) and waits for the copy.  Uses up plan.parent.
int clm_build_tree_index(const char* what, const int32_t* ids, const int32_t* seq_off, int n_seq, ClmTreePlan& plan, int R,
                         int* d_ints, hipStream_t s, ClmTreeIndex* ix);

// ---- attention and sums ----
// Causal attention of every sequence over the rows [seq_off[s], seq_off[s + 1]) of qkv (row q[Hq * D] | k[Hkv * D] |
// v[Hkv * D], query head h reads K / V head h / (Hq / Hkv)) into out ([rows][Hq * D]); D = hd is 64, 80 or 128.
int clm_launch_attn(const _Float16* qkv, _Float16* out, const int* seq_off, int n_seq, int Hq, int Hkv, int hd, hipStream_t s);
// The same over tree paths: position i of sequence s is row tok_node[seq_off[s] + i]; written are the rows a sequence owns.
int clm_launch_attn_tree(const _Float16* qkv, _Float16* out, const int* seq_off, const int* tok_node, const int* own_start,
                         int n_seq, int Hq, int Hkv, int hd, hipStream_t s);
// scores[q] = sum of logp[tok_hrow[t]] along sequence q's tokens 1.. in order; tok_logp as above
int clm_launch_seq_sum_tree(const float* logp, const int* seq_off, const int* tok_hrow, float* scores, float* tok_logp,
                            int n_seq, hipStream_t s);

// ---- the OPT forward ----
inline ClmLayout clm_opt_layout(const b2t_clm_t* m, long long rows, long long head_rows, size_t ints) {
  return clm_layout(m->d_model, 3LL * m->d_model, m->ffn_dim, m->vocab, rows, head_rows, ints);
}

// Fused LM head over r.Mh rows of x16 (already normalised): logp[i] = log p(r.d_tgt[i]) under the logits x16[i] . W^T;
// `head` launches the EP_HEAD GEMM in the element type of x16 and W (the default: fp16)
typedef int (*ClmGemmLaunch)(const ClmGemm& g, hipStream_t s);
inline int clm_head(const void* x16, const void* W, int vocab, int d, const ClmRun& r, const ClmLayout& L, char* base,
                    hipStream_t s, ClmGemmLaunch head = &launch_gemm<EP_HEAD>) {
  ClmGemm g{};
  g.A = x16; g.B = W; g.M = (int)r.Mh; g.N = vocab; g.K = d;
  g.pmax = reinterpret_cast<float*>(base + L.pmax); g.psum = reinterpret_cast<float*>(base + L.psum);
  g.tlogit = reinterpret_cast<float*>(base + L.tlogit); g.tgt = r.d_tgt; g.ncg = (int)L.ncg;
  if (int rc = head(g, s)) return rc;
  return clm_launch_head_combine(g.pmax, g.psum, g.tlogit, g.ncg, reinterpret_cast<float*>(base + L.logp), r.Mh, s);
}

// The pre-LN OPT forward over r.rows rows up to the per-row log-probs logp[r.Mh] (base + L.logp); attn(layer, qkv, out)
// enqueues one layer's attention from qkv ([rows][3d]) into out ([rows][d]).  `fc1` launches the fc1 GEMM with the policy's
// activation in its epilogue: OPT's ReLU (OptPolicy, below), or GPT-2's gelu_new (causal_lm_gpt2.hip) -- the two differ in
// nothing else behind the loader.
template <class Attn>
int clm_forward(const b2t_clm_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s, ClmGemmLaunch fc1) {
  const int d = m.d_model, hd = d / m.n_heads, F = m.ffn_dim, M = (int)r.rows;
  float* resid = reinterpret_cast<float*>(base + L.resid);
  _Float16* x16 = reinterpret_cast<_Float16*>(base + L.x16);
  _Float16* qkv = reinterpret_cast<_Float16*>(base + L.qkv);
  _Float16* hb = reinterpret_cast<_Float16*>(base + L.hbuf);
  auto H16 = [](const void* p) { return static_cast<const _Float16*>(p); };
  if (int rc = clm_launch_embed(r.d_ids, r.d_pos, H16(m.embed_tokens), H16(m.embed_positions), resid, d, r.rows, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_layer_t& w = m.layers_host[l];
    if (int rc = clm_launch_layernorm(resid, nullptr, r.rows, H16(w.ln1_w), H16(w.ln1_b), x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = H16(w.qkv_w); g.M = M; g.N = 3 * d; g.K = d; g.bias = H16(w.qkv_b); g.out16 = qkv; g.ldo = 3 * d;
    g.qscale = 1.0f / sqrtf((float)hd); g.qcols = d;
    if (int rc = launch_gemm<EP_F16>(g, s)) return rc;
    if (int rc = attn(l, qkv, x16)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.out_w); g.M = M; g.N = d; g.K = d; g.bias = H16(w.out_b); g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
    if (int rc = clm_launch_layernorm(resid, nullptr, r.rows, H16(w.ln2_w), H16(w.ln2_b), x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.fc1_w); g.M = M; g.N = F; g.K = d; g.bias = H16(w.fc1_b); g.out16 = hb; g.ldo = F;
    if (int rc = fc1(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = H16(w.fc2_w); g.M = M; g.N = d; g.K = F; g.bias = H16(w.fc2_b); g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
  }
  if (r.Mh <= 0) return 0;
  if (int rc = clm_launch_layernorm(resid, r.d_src, r.Mh, H16(m.final_ln_w), H16(m.final_ln_b), x16, d, s)) return rc;
  return clm_head(x16, H16(m.embed_tokens), m.vocab, d, r, L, base, s);   // the head is tied to embed_tokens
}

// ---- the context cache (causal_lm_cache.hip) ----
// The rule of a cached call (causal_lm_cache.hip's header; b2t_clm_cache_plan_host exports it): trunk Tn, common prefix P with
// the cached chain, reused R = max(P - 1, 0), n_after = min(Tn, cap).  Family-independent.
struct ClmCachePlan { int Tn, P, R, n_after; };
ClmCachePlan clm_cache_plan(const int32_t* cache_ids, int cache_n, int cap, const int32_t* ids, const int32_t* seq_off, int n_seq);
// the state of stage B behind a tree layout of tree_total bytes: m, l per (row, query head) and the unnormalised o per row
struct ClmCachedState { size_t st_ml, st_o, total; };
ClmCachedState clm_cached_state(size_t tree_total, long long rows, int Hq, int d_model);
// One layer's attention of a cached call on the row q[Hq * hd] | k[Hkv * hd] | v[Hkv * hd]: the append of the trunk's K | V
// (columns [Hq * hd, (Hq + 2 * Hkv) * hd) of qkv rows 0..app_rows-1 -> slab rows R.., slab row = k[Hkv * hd] | v[Hkv * hd]),
// stage B over the whole cached blocks (trunk on and R >= 32), then the tree walk.  clm_cached_attn reads B2T_CLM_TRUNK_ATTN.
struct ClmCachedAttn {
  const int *soff, *node, *own;
  int Hq, Hkv, hd, n_seq, R, app_rows;
  long long rows;
  bool trunk;
  float *st_ml, *st_o;
  float cap;   // Gemma-2: the soft cap on the scores, 0 = none (every other family)
};
ClmCachedAttn clm_cached_attn(const ClmTreeIndex& ix, int n_seq, int Hq, int Hkv, int hd, int R, int app_rows, char* base,
                              const ClmCachedState& S, float cap = 0.f);
int clm_launch_attn_cached(const ClmCachedAttn& a, const _Float16* qkv, _Float16* slab, _Float16* out, hipStream_t s);
// the attention of clm_launch_attn_cached (behind its append) with the soft-capped kernels, for head dim 256 or a.cap > 0
// (Gemma-2: head dim 128 or 256); causal_lm_gemma2.hip
int clm_launch_attn_cached_cap(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s);
// the attention of clm_launch_attn_cached (behind its append) at head dim 96 (Phi-3); causal_lm_phi3.hip
int clm_launch_attn_cached_96(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s);
// dst[i] = logp[i], i < n: the trunk's head rows -> the cache's logp at R + 1
int clm_launch_cache_logp(const float* logp, float* dst, int n, hipStream_t s);
// clm_launch_seq_sum_tree with the log-probs of positions 1..R taken from cache_logp
int clm_launch_seq_sum_tree_cached(const float* logp, const float* cache_logp, int R, const int* seq_off, const int* tok_hrow,
                                   float* scores, float* tok_logp, int n_seq, hipStream_t s);

// What a family's cached entry point does behind its model check (b2t_clm_score_tree_cached_f16 and
// b2t_clm_llama_score_tree_cached_f16): the refusals, the plan and the rule, the forward over the computed rows with the
// cached attention, the appends, the sums and the cache's bookkeeping; `uncached` names the call for callers without a cache.
// layout(rows, ints) is the family's tree layout; forward(run, L, base, attn, s) its forward, attn(layer, qkv, out) being one
// layer's attention.  The cache's kv is [n_layers][cap][2 * Hkv * hd].
// attn_cap: Gemma-2's soft cap on the attention scores (0, the default: none).
struct ClmCacheDims { int vocab, max_pos, Hq, Hkv, hd; float attn_cap = 0.f; };
template <class Layout, class Forward>
int clm_score_tree_cached(const char* who, const char* uncached, const ClmCacheDims& m, b2t_clm_cache_t* cache, int update,
                          const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                          long long* n_rows_out, int* n_reused_out, void* ws, size_t ws_bytes, hipStream_t s, Layout&& layout,
                          Forward&& forward) {
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  B2T_REQUIRE(cache, "%s: null cache (callers without one use %s)", who, uncached);
  B2T_REQUIRE(cache->kv && cache->logp && cache->ids_host, "%s: null cache member", who);
  B2T_REQUIRE(cache->cap >= 1, "%s: cache cap %d < 1", who, cache->cap);
  B2T_REQUIRE(cache->cap <= m.max_pos, "%s: cache cap %d above max_pos %d", who, cache->cap, m.max_pos);
  B2T_REQUIRE(cache->n >= 0 && cache->n <= cache->cap, "%s: cache n %d outside [0, cap %d]", who, cache->n, cache->cap);
  for (int t = 0; t < cache->n; ++t)
    B2T_REQUIRE(cache->ids_host[t] >= 0 && cache->ids_host[t] < m.vocab, "%s: cached token %d has id %d outside [0, %d)", who, t,
                cache->ids_host[t], m.vocab);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];

  // the tree plan and the rule; the index arrays are over the computed rows (node n is row n - R)
  ClmTreePlan& plan = clm_plan_tree(ids_host, seq_off_host, n_seq);
  const ClmCachePlan P = clm_cache_plan(cache->ids_host, cache->n, cache->cap, ids_host, seq_off_host, n_seq);
  const int R = P.R;
  const long long rows = plan.Mn - R;
  if (n_rows_out) *n_rows_out = rows;
  if (n_reused_out) *n_reused_out = R;
  const ClmLayout L = layout(rows, tree_ints(rows, M, n_seq));
  const ClmCachedState S = clm_cached_state(L.total, rows, m.Hq, m.Hq * m.hd);
  B2T_REQUIRE(ws_bytes >= S.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, S.total);
  // what the cache gains: positions R .. n_after - 1 (K | V rows 0.. of qkv, head rows 0.. of logp)
  const int app_rows = update && P.n_after > R ? P.n_after - R : 0;
  const int app_logp = update && P.n_after > R + 1 ? P.n_after - R - 1 : 0;

  char* base = static_cast<char*>(ws);
  ClmTreeIndex ix;
  if (int rc = clm_build_tree_index(who, ids_host, seq_off_host, n_seq, plan, R, reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  float* logp = reinterpret_cast<float*>(base + L.logp);
  const ClmCachedAttn ca = clm_cached_attn(ix, n_seq, m.Hq, m.Hkv, m.hd, R, app_rows, base, S, m.attn_cap);
  _Float16* kv = static_cast<_Float16*>(cache->kv);
  const size_t slab_elems = (size_t)cache->cap * 2 * m.Hkv * m.hd;
  // a layer's K | V append, then its attention against the layer's slab
  auto attn = [&](int l, const _Float16* qkv, _Float16* out) -> int {
    return clm_launch_attn_cached(ca, qkv, kv + (size_t)l * slab_elems, out, s);
  };
  // from here on rows >= R of the cache may be overwritten: an error return leaves it at min(n, R)
  auto run = [&]() -> int {
    if (int rc = forward(ix.run, L, base, attn, s)) return rc;
    if (app_logp > 0)
      if (int rc = clm_launch_cache_logp(logp, cache->logp + R + 1, app_logp, s)) return rc;
    return clm_launch_seq_sum_tree_cached(logp, cache->logp, R, ix.d_soff, ix.d_hrow, scores_out, tok_logp_out, n_seq, s);
  };
  if (int rc = run()) {
    if (update && cache->n > R) cache->n = R;
    return rc;
  }
  if (update) {
    for (int t = R; t < P.n_after; ++t) cache->ids_host[t] = ids_host[t];
    cache->n = P.n_after;
  }
  return 0;
}

// ---- the entry points and the size rules of every family ----
// A policy P names the element type and supplies the launches that differ with it:
//   P::E                                        _Float16 or __bf16 (ClmElem)
// and whatever the family's forward asks of it: the Llama-derived families' policies are described in clm_llama.h; the two
// policies over OptFamily (below) have P::fc1, the launch of the fc1 GEMM with the activation in its epilogue.
//
// A family Fam is what the bodies and the size rules take beside the policy; x is the family's extra argument, of its own type X
// (the q / k norm array of Qwen3 and OLMo-2, or a descriptor: b2t_clm_moe_t, b2t_clm_gemma2_t, b2t_clm_phi3_t, b2t_clm_gptoss_t;
// a family without one ignores a null const void*):
//   Fam::Model                                  the descriptor: b2t_clm_t, b2t_clm_neox_t or b2t_clm_llama_t.  The bodies and the
//                                               rules read its n_layers, n_heads, vocab and max_pos themselves
//   Fam::Extra                                  the type X of a call that passes no extra argument
//   Fam::kv_heads(m)                            the K / V heads: n_kv_heads, or n_heads where the descriptor has one head count
//   Fam::layout(model, rows, hrows, ints, x)    the workspace layout of a forward
//   Fam::forward<P>(m, run, L, base, attn, s, x)   the forward; attn(layer, qkv, out) enqueues one layer's attention
//   Fam::attn<P>, Fam::attn_tree<P>(m, x, layer, ...)   the flat and the tree attention of one layer
//   Fam::head_dim(m, x)                         d_model / n_heads, or the descriptor's field (Gemma-2, Phi-3, gpt-oss)
//   Fam::attn_cap(x)                            the soft cap on the attention scores: 0, or Gemma-2's
//   Fam::dims_ok(model, x)                      what the size rules need of the descriptors: every field they divide by or size a
//                                               buffer with is vouched for here (llama_dims_ok or clm_mha_dims_ok and the family's term)
//   Fam::check<P>(who, model, x)                every refusal of the descriptors, a null model included, for the entry point `who`
// ClmMhaFamily (below) has everything but Model, layout, forward and check for a descriptor with one head count and hd = d_model /
// n_heads: OptFamily (OPT and GPT-2, below) and NeoxFamily (causal_lm_neox.hip) derive it.  LlamaFamilyBase (clm_llama.h) has the
// same for a b2t_clm_llama_t that obeys the Llama rule: the defaults, which a family derives and replaces where it differs.
// LlamaFamily is the Llama family's (Qwen3 included: P::qk_norm), Olmo2Family (clm_olmo2.h), MixtralFamily (clm_moe.h),
// Gemma2Family (clm_gemma2.h), Phi3Family (clm_phi3.h) and GptOssFamily (clm_gptoss.h) the others'.

// The flat entry point of a policy and a family; `who` is its name in every message, `extra` the family's extra argument.
template <class P, class Fam, class X = typename Fam::Extra>
int clm_family_score(const char* who, const typename Fam::Model* model, const int32_t* ids_host, const int32_t* seq_off_host,
                     int n_seq, float* scores_out, float* tok_logp_out, void* ws, size_t ws_bytes, void* stream,
                     const X* extra = nullptr) {
  using E = typename P::E;
  if (int rc = Fam::template check<P>(who, model, extra)) return rc;
  const typename Fam::Model& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  const ClmLayout L = Fam::layout(model, M, M - n_seq, flat_ints(M, n_seq), extra);
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmFlatIndex ix;
  if (int rc = clm_build_flat_index((std::string(who) + " upload").c_str(), ids_host, seq_off_host, n_seq,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int l, const E* qkv, E* out) { return Fam::template attn<P>(m, extra, l, qkv, out, ix.d_soff, n_seq, s); };
  if (int rc = Fam::template forward<P>(m, ix.run, L, base, attn, s, extra)) return rc;
  return clm_launch_seq_sum(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hoff, scores_out, tok_logp_out, n_seq, s);
}

// The tree entry point of a policy and a family.
template <class P, class Fam, class X = typename Fam::Extra>
int clm_family_score_tree(const char* who, const typename Fam::Model* model, const int32_t* ids_host, const int32_t* seq_off_host,
                          int n_seq, float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                          void* stream, const X* extra = nullptr) {
  using E = typename P::E;
  if (int rc = Fam::template check<P>(who, model, extra)) return rc;
  const typename Fam::Model& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];
  ClmTreePlan& plan = clm_plan_tree(ids_host, seq_off_host, n_seq);   // a node's position (learned or rotary) is its depth
  const long long Mn = plan.Mn;
  if (n_nodes_out) *n_nodes_out = Mn;
  const ClmLayout L = Fam::layout(model, Mn, Mn, tree_ints(Mn, M, n_seq), extra);
  B2T_REQUIRE(ws_bytes >= L.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(ws);
  ClmTreeIndex ix;
  if (int rc = clm_build_tree_index((std::string(who) + " upload").c_str(), ids_host, seq_off_host, n_seq, plan, 0,
                                    reinterpret_cast<int*>(base + L.ints), s, &ix))
    return rc;
  auto attn = [&](int l, const E* qkv, E* out) {
    return Fam::template attn_tree<P>(m, extra, l, qkv, out, ix.d_soff, ix.d_node, ix.d_own, n_seq, s);
  };
  if (int rc = Fam::template forward<P>(m, ix.run, L, base, attn, s, extra)) return rc;
  return clm_launch_seq_sum_tree(reinterpret_cast<float*>(base + L.logp), ix.d_soff, ix.d_hrow, scores_out, tok_logp_out, n_seq, s);
}

// The cached entry point of a policy and a family: the family's check, then the family-independent rule (clm_score_tree_cached)
// over the family's layout and forward; `uncached` names the tree call for callers without a cache.
template <class P, class Fam, class X = typename Fam::Extra>
int clm_family_score_tree_cached(const char* who, const char* uncached, const typename Fam::Model* model, b2t_clm_cache_t* cache,
                                 int update, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, float* scores_out,
                                 float* tok_logp_out, long long* n_rows_out, int* n_reused_out, void* ws, size_t ws_bytes,
                                 void* stream, const X* extra = nullptr) {
  if (int rc = Fam::template check<P>(who, model, extra)) return rc;
  const typename Fam::Model& m = *model;
  const ClmCacheDims dims{m.vocab, m.max_pos, m.n_heads, Fam::kv_heads(m), Fam::head_dim(m, extra), Fam::attn_cap(extra)};
  return clm_score_tree_cached(
      who, uncached, dims, cache, update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out, n_rows_out, n_reused_out, ws,
      ws_bytes, as_stream(stream), [&](long long rows, size_t ints) { return Fam::layout(model, rows, rows, ints, extra); },
      [&](const ClmRun& r, const ClmLayout& L, char* base, auto&& attn, hipStream_t s) {
        return Fam::template forward<P>(m, r, L, base, attn, s, extra);
      });
}

// The size rules behind every family's exported size functions: 0 for descriptors or counts no call would accept, else the bytes
// of the flat, the tree and the cached call's workspace and of a cache's K | V for `cap` positions.  The cached state is sized by
// n_heads * head_dim, which is d_model only where hd = d_model / n_heads.
template <class Fam, class X = typename Fam::Extra>
size_t clm_family_ws_bytes(const typename Fam::Model* m, long long n_tokens, int n_seq, const X* x = nullptr) {
  if (!Fam::dims_ok(m, x) || n_tokens < 1 || n_seq < 1 || n_seq > n_tokens) return 0;
  return Fam::layout(m, n_tokens, n_tokens - n_seq, flat_ints(n_tokens, n_seq), x).total;
}
template <class Fam, class X = typename Fam::Extra>
size_t clm_family_tree_ws_bytes(const typename Fam::Model* m, long long n_nodes, long long n_tokens, int n_seq, const X* x = nullptr) {
  if (!Fam::dims_ok(m, x) || n_nodes < 1 || n_nodes > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  return Fam::layout(m, n_nodes, n_nodes, tree_ints(n_nodes, n_tokens, n_seq), x).total;
}
template <class Fam, class X = typename Fam::Extra>
size_t clm_family_cache_kv_bytes(const typename Fam::Model* m, int cap, const X* x = nullptr) {
  if (!Fam::dims_ok(m, x) || cap < 1 || cap > m->max_pos || m->n_layers < 1) return 0;
  return (size_t)m->n_layers * (size_t)cap * 2 * (size_t)Fam::kv_heads(*m) * (size_t)Fam::head_dim(*m, x) * sizeof(_Float16);
}
template <class Fam, class X = typename Fam::Extra>
size_t clm_family_tree_cached_ws_bytes(const typename Fam::Model* m, long long n_rows, long long n_tokens, int n_seq,
                                       const X* x = nullptr) {
  const size_t tree = clm_family_tree_ws_bytes<Fam>(m, n_rows, n_tokens, n_seq, x);
  return tree ? clm_cached_state(tree, n_rows, m->n_heads, m->n_heads * Fam::head_dim(*m, x)).total : 0;
}

// What the families of a descriptor with one head count and hd = d_model / n_heads (M: b2t_clm_t or b2t_clm_neox_t) hand the
// bodies and the size rules beside Model, layout, forward and check: no extra argument, and the OPT paths' two fp16 attention
// launches with Hkv = Hq.
struct ClmMhaFamily {
  using Extra = void;
  template <class M>
  static int kv_heads(const M& m) { return m.n_heads; }
  template <class M>
  static int head_dim(const M& m, const void*) { return m.d_model / m.n_heads; }
  static float attn_cap(const void*) { return 0.f; }
  template <class M>
  static bool dims_ok(const M* m, const void*) { return clm_mha_dims_ok(m); }
  template <class P, class M>
  static int attn(const M& m, const void*, int /*layer*/, const _Float16* qkv, _Float16* out, const int* seq_off, int n_seq,
                  hipStream_t s) {
    return clm_launch_attn(qkv, out, seq_off, n_seq, m.n_heads, m.n_heads, m.d_model / m.n_heads, s);
  }
  template <class P, class M>
  static int attn_tree(const M& m, const void*, int /*layer*/, const _Float16* qkv, _Float16* out, const int* seq_off,
                       const int* tok_node, const int* own_start, int n_seq, hipStream_t s) {
    return clm_launch_attn_tree(qkv, out, seq_off, tok_node, own_start, n_seq, m.n_heads, m.n_heads, m.d_model / m.n_heads, s);
  }
};

// The family of b2t_clm_t: clm_opt_layout, clm_check_model (its messages say "b2t_clm:", not the entry point's name) and
// clm_forward with the policy's fc1.  OptPolicy is OPT's (ReLU); GPT-2's is causal_lm_gpt2.hip's.
struct OptFamily : ClmMhaFamily {
  using Model = b2t_clm_t;
  static ClmLayout layout(const b2t_clm_t* m, long long rows, long long hrows, size_t ints, const void*) {
    return clm_opt_layout(m, rows, hrows, ints);
  }
  template <class P>
  static int check(const char*, const b2t_clm_t* m, const void*) { return clm_check_model(m); }
  template <class P, class Attn>
  static int forward(const b2t_clm_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s, const void*) {
    return clm_forward(m, r, L, base, attn, s, P::fc1);
  }
};
struct OptPolicy {
  using E = _Float16;
  static constexpr ClmGemmLaunch fc1 = &launch_gemm<EP_RELU>;
};

}  // namespace b2t
