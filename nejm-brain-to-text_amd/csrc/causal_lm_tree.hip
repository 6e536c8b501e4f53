// causal_lm_tree.hip — the scoring forward of causal_lm.hip over a shared-prefix token tree (b2t_clm_score_tree_f16).
// The candidates of an n-best list repeat each other's prefixes, and with contextual decoding all of them start with the same
// context.  In a causal LM a token's hidden state depends only on the tokens before it, and causal_lm.hip's kernels compute
// every row in an order that depends only on that row, so a token whose whole prefix is shared has bit for bit the same
// residual row, K and V in every candidate.  This path computes each distinct prefix once.
//
// The tree (host): a NODE is a distinct token prefix -- token t of sequence a and token u of sequence b are the same node
// iff they sit at the same position p and the two sequences have identical ids at positions 0..p.  Nodes are numbered in
// order of first appearance in the packed ids, so a list with no sharing gives node_of_token[t] == t.  Different first tokens
// give several roots; duplicate candidates map to the same nodes throughout.  Two facts the kernels rely on:
//   (a) along one sequence, the nodes it is the first to meet (the nodes it OWNS) form a suffix of its path: once a prefix
//       is new, every longer prefix is new.  So ownership is one start index per sequence (own_start[s], = its length when it
//       owns nothing), every node has exactly one owner, and no two workgroups write the same row;
//   (b) a node's depth is its position: embed_positions is indexed as in the flat path and the max_pos check is unchanged.
//
// The forward runs over n_nodes rows instead of n_tokens: it is clm_forward (clm_internal.h) -- embedding, LayerNorm, the four
// GEMMs per layer and the fused LM head are causal_lm.hip's kernels (B2T_CLM_GEMM_256 applies through launch_gemm).  New
// here are the plan, the index arrays built from it (clm_build_tree_index, which the cached path and the Llama family use
// too), the attention, which reaches its rows through the sequence's path, and the gathered per-sequence sum.  The head has
// one row per non-root node: source = the parent's row, target = the node's id.
//
// Numerics: causal_lm.hip's contract, and bit-identical to the flat path: the attention keeps a query's arithmetic order
// (key blocks of 32 aligned at position 0, query blocks 32-aligned too, online softmax per lane, P rounded to fp16 per block),
// and a sequence's log-probs are added along its path in token order by one thread.
#include <math.h>
#include <unordered_map>
#include <vector>

#include "clm_attn.h"

namespace b2t {
namespace {

// The attention kernel, clm_attn_tree_kernel, is clm_attn.h's template; this unit instantiates it in fp16 (clm_launch_attn_tree).

// scores[s] = sum of the log-probs along the sequence's path in token order (one thread, as clm_seq_sum_kernel);
// tok_hrow[t] = the head row of token t's node (unused at a sequence's first token); tok_logp (optional) = per token in the
// caller's packed order, 0 at each sequence's first token
__global__ __launch_bounds__(64) void clm_seq_sum_tree_kernel(const float* logp, const int* seq_off, const int* tok_hrow,
                                                              float* scores, float* tok_logp) {
  const int s = blockIdx.x, t0 = seq_off[s], n = seq_off[s + 1] - t0;
  if (tok_logp) {
    if (threadIdx.x == 0) tok_logp[t0] = 0.f;
    for (int i = 1 + threadIdx.x; i < n; i += 64) tok_logp[t0 + i] = logp[tok_hrow[t0 + i]];
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int i = 1; i < n; ++i) acc += logp[tok_hrow[t0 + i]];
    scores[s] = acc;
  }
}

}  // namespace

// The sizes, the plan and the index builder have external linkage (clm_internal.h): causal_lm_cache.hip and
// causal_lm_llama.hip size, plan and index their calls with them.
size_t tree_ints(long long rows, long long M, int n_seq) { return (size_t)(4 * rows + 2 * M + 2 * (long long)n_seq + 1); }

// The plan.  node_of_token gets all n_tokens entries; parent_of_node (and own_start, optional, per sequence) only below cap.
// Returns the number of nodes.  A node's key is (parent node + 1, id): one hash lookup per token.
long long tree_plan(const int32_t* ids, const int32_t* seq_off, int n_seq, int32_t* node_of_token, int32_t* parent_of_node,
                    long long cap, int32_t* own_start) {
  static thread_local std::unordered_map<uint64_t, int32_t> map;
  map.clear();
  map.reserve((size_t)seq_off[n_seq]);
  long long n = 0;
  for (int s = 0; s < n_seq; ++s) {
    const int a = seq_off[s], b = seq_off[s + 1];
    int32_t parent = -1, own = b - a;
    for (int t = a; t < b; ++t) {
      const uint64_t key = ((uint64_t)(uint32_t)(parent + 1) << 32) | (uint32_t)ids[t];
      auto ins = map.emplace(key, (int32_t)n);
      if (ins.second) {
        if (own == b - a) own = t - a;
        if (n < cap) parent_of_node[n] = parent;
        ++n;
      }
      parent = node_of_token[t] = ins.first->second;
    }
    if (own_start) own_start[s] = own;
  }
  return n;
}

ClmTreePlan& clm_plan_tree(const int32_t* ids, const int32_t* seq_off, int n_seq) {
  static thread_local ClmTreePlan P;
  const long long M = seq_off[n_seq];
  P.tok_node.resize((size_t)M); P.parent.resize((size_t)M); P.own.resize((size_t)n_seq);
  P.Mn = tree_plan(ids, seq_off, n_seq, P.tok_node.data(), P.parent.data(), M, P.own.data());
  return P;
}

int clm_build_tree_index(const char* what, const int32_t* ids, const int32_t* seq_off, int n_seq, ClmTreePlan& plan, int R,
                         int* d_ints, hipStream_t s, ClmTreeIndex* ix) {
  const long long M = seq_off[n_seq], Mn = plan.Mn, rows = Mn - R;
  const std::vector<int32_t>& tok_node = plan.tok_node;
  static thread_local std::vector<int32_t> host;
  host.assign(tree_ints(rows, M, n_seq), 0);
  int* h_id = host.data(); int* h_pos = h_id + rows; int* h_src = h_pos + rows; int* h_tgt = h_src + rows;
  int* h_node = h_tgt + rows; int* h_hrow = h_node + M; int* h_soff = h_hrow + M; int* h_own = h_soff + n_seq + 1;
  for (int q = 0; q < n_seq; ++q) {
    const int a = seq_off[q], b = seq_off[q + 1];
    h_soff[q] = a; h_own[q] = plan.own[q];
    for (int t = a; t < b; ++t) {
      const int n = tok_node[t];
      h_node[t] = n;
      if (n >= R) { h_id[n - R] = ids[t]; h_pos[n - R] = t - a; }   // the true position: a node's depth
    }
  }
  h_soff[n_seq] = (int)M;
  long long Mh = 0;
  {
    std::vector<int32_t>& hrow = plan.parent;   // parent[n] is read before hrow[n] is written
    for (long long n = 0; n < Mn; ++n) {
      const int p = plan.parent[n];
      if (n > R && p >= 0) { h_src[Mh] = p - R; h_tgt[Mh] = h_id[n - R]; hrow[n] = (int32_t)Mh++; }
      else hrow[n] = 0;
    }
    for (long long t = 0; t < M; ++t) h_hrow[t] = hrow[tok_node[t]];
  }
  if (int rc = check_hip(hipMemcpyAsync(d_ints, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s), what)) return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), what)) return rc;
  const int* d_node = d_ints + 4 * rows;
  *ix = ClmTreeIndex{{rows, Mh, d_ints, d_ints + rows, d_ints + 2 * rows, d_ints + 3 * rows}, d_node, d_node + M, d_node + 2 * M,
                     d_node + 2 * M + n_seq + 1};
  return 0;
}

int clm_launch_attn_tree(const _Float16* qkv, _Float16* out, const int* seq_off, const int* tok_node, const int* own_start,
                         int n_seq, int Hq, int Hkv, int hd, hipStream_t s) {
  const dim3 grid(n_seq, Hq);
  if (hd == 64) hipLaunchKernelGGL(clm_attn_tree_kernel<64>, grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv);
  else if (hd == 80) hipLaunchKernelGGL(clm_attn_tree_kernel<80>, grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv);
  else hipLaunchKernelGGL(clm_attn_tree_kernel<128>, grid, dim3(256), 0, s, qkv, out, seq_off, tok_node, own_start, Hq, Hkv);
  B2T_CHECK_LAUNCH("clm_attn_tree_kernel");
  return 0;
}

int clm_launch_seq_sum_tree(const float* logp, const int* seq_off, const int* tok_hrow, float* scores, float* tok_logp,
                            int n_seq, hipStream_t s) {
  hipLaunchKernelGGL(clm_seq_sum_tree_kernel, dim3(n_seq), dim3(64), 0, s, logp, seq_off, tok_hrow, scores, tok_logp);
  B2T_CHECK_LAUNCH("clm_seq_sum_tree_kernel");
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" int b2t_clm_tree_plan_host(const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, int32_t* node_of_token,
                                      int32_t* parent_of_node, long long cap, long long* n_nodes) {
  const char* who = "b2t_clm_tree_plan_host";
  B2T_REQUIRE(ids_host && seq_off_host && node_of_token && n_nodes && (parent_of_node || cap <= 0), "%s: null argument", who);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, 0, 0)) return rc;
  *n_nodes = tree_plan(ids_host, seq_off_host, n_seq, node_of_token, parent_of_node, cap < 0 ? 0 : cap, nullptr);
  if (*n_nodes > cap) {
    set_error("%s: %lld nodes, room for %lld", who, *n_nodes, cap);
    return -2;
  }
  return 0;
}

extern "C" size_t b2t_clm_tree_ws_bytes(const b2t_clm_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  return clm_family_tree_ws_bytes<OptFamily>(model, n_nodes, n_tokens, n_seq);
}

extern "C" int b2t_clm_score_tree_f16(const b2t_clm_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                      float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                      void* stream) {
  return clm_family_score_tree<OptPolicy, OptFamily>("b2t_clm_score_tree_f16", model, ids_host, seq_off_host, n_seq, scores_out,
                                                     tok_logp_out, n_nodes_out, ws, ws_bytes, stream);
}
