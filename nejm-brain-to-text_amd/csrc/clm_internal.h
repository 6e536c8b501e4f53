// clm_internal.h — host-side pieces of the causal-LM forward shared by causal_lm.hip (the flat scoring path, which defines
// them), causal_lm_tree.hip (the shared-prefix tree path, which defines the plan and the workspace layout),
// causal_lm_cache.hip (the tree path behind a context cache) and causal_lm_llama.hip (the Llama family, flat and tree).  The
// kernels themselves stay private to their files; these are their launchers, so each GEMM epilogue is instantiated once.
#pragma once
#include "common.h"

namespace b2t {

constexpr int CLM_ROWPAD = 256;   // A operands and weights are padded to this many rows

// EP_ROPE and EP_SWIGLU (the Llama family) pair the two 32-column halves of a wave's 64-column slice in one lane:
//   EP_ROPE   out16[r][c], out16[r][c + 32] = the rotation of (C[r][c], C[r][c + 32]) + bias by the angle of row r's position
//             and frequency (c % hd) / 2 + c % 32 (columns < rope_cols; the others are written as EP_F16 writes them);
//   EP_SWIGLU out16[r][c0 / 2 + i] = silu(C[r][c0 + i]) * C[r][c0 + 32 + i], c0 a multiple of 64, i < 32 (ldo = N / 2).
enum { EP_F16 = 0, EP_RELU = 1, EP_RESID = 2, EP_HEAD = 3, EP_ROPE = 4, EP_SWIGLU = 5 };

struct ClmGemm {
  const _Float16* A;      // [round_up(M, 256)][K]
  const _Float16* B;      // [round_up(N, 256)][K]
  int M, N, K;            // K % 64 == 0
  const _Float16* bias;   // [N] or null
  _Float16* out16;        // EP_F16 / EP_RELU: [M][ldo]
  float* resid;           // EP_RESID: [M][ldo] += C
  int ldo;
  float qscale; int qcols;   // EP_F16: columns < qcols are multiplied by qscale after the bias (OPT's q scaling)
  float* pmax; float* psum;  // EP_HEAD: [M][ncg] per 64-column group max / sum exp(v - max)
  float* tlogit; const int* tgt; int ncg;   // EP_HEAD: tlogit[r] = C[r][tgt[r]]
  const int* pos;                           // EP_ROPE: [M] position of each row
  const float* rope_cos; const float* rope_sin;   // EP_ROPE: fp32 [max_pos][hd / 2]
  int rope_cols, hd;                        // EP_ROPE: columns < rope_cols (q | k) are rotated; head dim (64 or 128)
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

// ---- causal_lm_tree.hip ----
// Workspace of a forward over Mn rows for M packed tokens in n_seq sequences: sized by Mn alone where the flat path has
// n_tokens - n_seq head rows (the head has at most a row per computed row).
struct TreeLayout {
  size_t ints, resid, x16, qkv, hbuf, pmax, psum, tlogit, logp, total;
  long long Mp, ncg;
};
// ints of the index arrays: node_id[Mn] node_pos[Mn] head_src[Mn] head_tgt[Mn] tok_node[M] tok_hrow[M] seq_off[n+1] own_start[n]
size_t tree_ints(long long Mn, long long M, int n_seq);
TreeLayout tree_layout(const b2t_clm_t* m, long long Mn, long long M, int n_seq);
// The shared-prefix plan (b2t_clm_tree_plan_host): node_of_token gets all n_tokens entries; parent_of_node (and own_start,
// optional, per sequence) only below cap.  Returns the number of nodes.
// scores[q] = sum of logp[tok_hrow[t]] along sequence q's tokens 1.. in order; tok_logp as above
int clm_launch_seq_sum_tree(const float* logp, const int* seq_off, const int* tok_hrow, float* scores, float* tok_logp,
                            int n_seq, hipStream_t s);
long long tree_plan(const int32_t* ids, const int32_t* seq_off, int n_seq, int32_t* node_of_token, int32_t* parent_of_node,
                    long long cap, int32_t* own_start);

}  // namespace b2t
