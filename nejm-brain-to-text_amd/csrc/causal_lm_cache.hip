// causal_lm_cache.hip — the shared-prefix tree forward of causal_lm_tree.hip behind a context cache
// (b2t_clm_score_tree_cached_f16, and through the launchers of clm_internal.h b2t_clm_llama_score_tree_cached_f16 of
// causal_lm_llama.hip: the kernels work on the row q[Hq * D] | k[Hkv * D] | v[Hkv * D], OPT being Hkv = Hq).  In closed-loop
// decoding every rescoring call scores its candidates behind the decoding
// context (language-model-standalone.py:188-190), and the context only grows: context k+1 = context k + the sentence just
// chosen.  The kernels compute a row in an order that depends only on that row, so the K and V rows and the log-prob of a
// context token computed by an earlier call ARE the values this call would compute.  The cache keeps them; scores stay
// byte-identical to the flat and the tree call.
//
// The rule (host, cache_plan; b2t_clm_cache_plan_host exports it).  The cache holds ONE token chain c[0..n).  For a call:
//   trunk  Tn = the longest token prefix common to ALL sequences of the call; in the tree plan's numbering (first appearance)
//               the trunk is nodes 0..Tn-1 = positions 0..Tn-1 of sequence 0, and every other node is >= Tn;
//   P         = the longest common prefix of the trunk and the cached chain;
//   reused R  = max(P - 1, 0): nodes 0..R-1 are not computed, their K / V come from the cache in every layer and the log-probs
//               of positions 1..R come from the cache.  Position P-1 IS recomputed: its final hidden row is the head source
//               of its children, and hidden states are not cached.  Computed row of node n >= R: n - R.
//   after the call (update on) the cache holds the trunk: positions R..min(Tn, cap)-1 are written from this call's K / V of
//               every layer and from its head log-probs, n = min(Tn, cap).
// Facts the kernels rely on: R < Tn whenever Tn > 0, so every sequence is longer than R, path position i < Tn is node i, and
// path[i] >= R iff i >= R; a head row exists for every non-root node > R, its source (the parent) is a computed row; the
// trunk's head rows are head rows 0..Tn-R-2 in order, so the log-prob append is one contiguous copy.
//
// Stage B (B2T_CLM_TRUNK_ATTN, read per call): the keys [0, Rb), Rb = R - R % 32, are whole 32-key blocks of the cache, the
// same for every computed row, and no causal mask applies to them (every computed row sits at a position >= R).
// clm_attn_trunk_kernel runs them for 32 computed rows at a time in row order and leaves each row's online-softmax state
// (m, l, unnormalised o, exact fp32) in the workspace; clm_attn_tree_cached_kernel then starts at key block Rb / 32 from that
// state.  A lane owns one query column of the 32 x 32 x 16 MFMA and a column's result depends on that column's B operand
// alone, so a query meets the same key blocks in the same order with the same values: which other queries share its block
// is the only thing that changes.
#include <math.h>
#include <stdlib.h>
#include <vector>

#include "clm_attn.h"

namespace b2t {
namespace {

// The two attention kernels of this path, clm_attn_tree_cached_kernel and clm_attn_trunk_kernel, are templates of clm_attn.h
// (this unit instantiates them for head dims 64, 80 and 128; causal_lm_gemma2.hip their soft-capped forms, causal_lm_phi3.hip
// head dim 96).

// cache append: K | V of the trunk's computed rows (qkv rows 0..rows-1 of width rs, columns qc .. qc + cs) -> dst rows 0..
// ([.][cs], the layer slab at row R), as 16-byte pieces; qc = Hq * D, cs = 2 * Hkv * D, rs = qc + cs
__global__ __launch_bounds__(256) void clm_cache_append_kernel(const _Float16* qkv, _Float16* dst, int qc, int cs, long long rows) {
  const int pcs = cs / 8;
  const long long n = rows * pcs, rs = (long long)qc + cs;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const long long r = i / pcs;
    const int c = (int)(i % pcs);
    *reinterpret_cast<half8*>(dst + r * cs + 8 * c) = *reinterpret_cast<const half8*>(qkv + r * rs + qc + 8 * c);
  }
}

// cache append of the trunk's log-probs: head rows 0..n-1 -> dst (the cache's logp at R + 1)
__global__ __launch_bounds__(256) void clm_cache_logp_kernel(const float* logp, float* dst, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = logp[i];
}

// clm_seq_sum_tree_kernel with the log-probs of positions 1..R taken from the cache: one thread adds in token order, so the
// sum is the tree path's operand for operand.  tok_hrow[t] = the head row of token t's node (unused at positions <= R).
__global__ __launch_bounds__(64) void clm_seq_sum_tree_cached_kernel(const float* logp, const float* cache_logp, int R,
                                                                     const int* seq_off, const int* tok_hrow, float* scores,
                                                                     float* tok_logp) {
  const int s = blockIdx.x, t0 = seq_off[s], n = seq_off[s + 1] - t0;
  if (tok_logp) {
    if (threadIdx.x == 0) tok_logp[t0] = 0.f;
    for (int i = 1 + threadIdx.x; i < n; i += 64) {
      const float* src = i <= R ? cache_logp + i : logp + tok_hrow[t0 + i];
      tok_logp[t0 + i] = *src;
    }
  }
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int i = 1; i < n; ++i) {
      const float* src = i <= R ? cache_logp + i : logp + tok_hrow[t0 + i];
      acc += *src;
    }
    scores[s] = acc;
  }
}

constexpr bool CLM_TRUNK_ATTN_DEFAULT = false;

// one layer's attention of the cached call: stage B over the whole cached blocks (trunk on and R >= 32), then the tree walk
template <int D>
int launch_attn(const ClmCachedAttn& a, const _Float16* qkv, const _Float16* slab, _Float16* out, hipStream_t s) {
  const int Rb = a.trunk ? a.R - a.R % 32 : 0;
  if (Rb > 0) {
    hipLaunchKernelGGL(clm_attn_trunk_kernel<D>, dim3((unsigned)((a.rows + 31) / 32), a.Hq), dim3(64), 0, s, qkv, slab, a.Hkv,
                       (int)a.rows, Rb / 32, a.st_ml, a.st_o);
    B2T_CHECK_LAUNCH("clm_attn_trunk_kernel");
  }
  hipLaunchKernelGGL(clm_attn_tree_cached_kernel<D>, dim3(a.n_seq, a.Hq), dim3(256), 0, s, qkv, slab, out, a.soff, a.node, a.own,
                     a.Hkv, a.R, Rb > 0 ? a.st_ml : nullptr, Rb > 0 ? a.st_o : nullptr, Rb / 32);
  B2T_CHECK_LAUNCH("clm_attn_tree_cached_kernel");
  return 0;
}

}  // namespace

// The rule of the file header.  Sequences are non-empty, seq_off[0] == 0, 0 <= cache_n <= cap.
ClmCachePlan clm_cache_plan(const int32_t* cache_ids, int cache_n, int cap, const int32_t* ids, const int32_t* seq_off, int n_seq) {
  long long Tn = seq_off[1];
  for (int s = 1; s < n_seq && Tn > 0; ++s) {
    const int32_t* b = ids + seq_off[s];
    const long long len = seq_off[s + 1] - seq_off[s];
    long long k = 0;
    while (k < Tn && k < len && b[k] == ids[k]) ++k;
    Tn = k;
  }
  long long P = 0;
  while (P < Tn && P < cache_n && cache_ids[P] == ids[P]) ++P;
  ClmCachePlan p;
  p.Tn = (int)Tn; p.P = (int)P; p.R = P > 0 ? (int)P - 1 : 0;
  p.n_after = (int)(Tn < cap ? Tn : cap);
  return p;
}

ClmCachedState clm_cached_state(size_t tree_total, long long rows, int Hq, int d_model) {
  ClmCachedState S{};
  size_t off = tree_total;
  S.st_ml = off; off += al256(sizeof(float) * (size_t)(rows * Hq * 2));
  S.st_o = off;  off += al256(sizeof(float) * (size_t)(rows * d_model));
  S.total = off;
  return S;
}

// What clm_launch_attn_cached needs for every layer of one call: the index arrays, the shapes, the rows to append, where the
// state of stage B lives in the workspace, and whether stage B runs.
ClmCachedAttn clm_cached_attn(const ClmTreeIndex& ix, int n_seq, int Hq, int Hkv, int hd, int R, int app_rows, char* base,
                              const ClmCachedState& S, float cap) {
  // B2T_CLM_TRUNK_ATTN, read per call: 0 = every key block in clm_attn_tree_cached_kernel (stage A); 1 = the cached blocks
  // in clm_attn_trunk_kernel (stage B)
  const char* e = getenv("B2T_CLM_TRUNK_ATTN");
  const bool trunk = e && *e ? atoi(e) != 0 : CLM_TRUNK_ATTN_DEFAULT;
  return ClmCachedAttn{ix.d_soff, ix.d_node, ix.d_own, Hq, Hkv, hd, n_seq, R, app_rows, ix.run.rows, trunk,
                       reinterpret_cast<float*>(base + S.st_ml), reinterpret_cast<float*>(base + S.st_o), cap};
}

int clm_launch_attn_cached(const ClmCachedAttn& a, const _Float16* qkv, _Float16* slab, _Float16* out, hipStream_t s) {
  const int qc = a.Hq * a.hd, cs = 2 * a.Hkv * a.hd;
  if (a.app_rows > 0) {
    const long long pieces = (long long)a.app_rows * (cs / 8);
    hipLaunchKernelGGL(clm_cache_append_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, qkv,
                       slab + (size_t)a.R * cs, qc, cs, (long long)a.app_rows);
    B2T_CHECK_LAUNCH("clm_cache_append_kernel");
  }
  if (a.hd == 256 || a.cap > 0.f) return clm_launch_attn_cached_cap(a, qkv, slab, out, s);   // Gemma-2 (causal_lm_gemma2.hip)
  if (a.hd == 96) return clm_launch_attn_cached_96(a, qkv, slab, out, s);   // Phi-3 (causal_lm_phi3.hip)
  if (a.hd == 64) return launch_attn<64>(a, qkv, slab, out, s);
  if (a.hd == 80) return launch_attn<80>(a, qkv, slab, out, s);
  return launch_attn<128>(a, qkv, slab, out, s);
}

int clm_launch_cache_logp(const float* logp, float* dst, int n, hipStream_t s) {
  hipLaunchKernelGGL(clm_cache_logp_kernel, dim3((n + 255) / 256), dim3(256), 0, s, logp, dst, n);
  B2T_CHECK_LAUNCH("clm_cache_logp_kernel");
  return 0;
}

int clm_launch_seq_sum_tree_cached(const float* logp, const float* cache_logp, int R, const int* seq_off, const int* tok_hrow,
                                   float* scores, float* tok_logp, int n_seq, hipStream_t s) {
  hipLaunchKernelGGL(clm_seq_sum_tree_cached_kernel, dim3(n_seq), dim3(64), 0, s, logp, cache_logp, R, seq_off, tok_hrow, scores,
                     tok_logp);
  B2T_CHECK_LAUNCH("clm_seq_sum_tree_cached_kernel");
  return 0;
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_cache_kv_bytes(const b2t_clm_t* model, int cap) {
  return clm_family_cache_kv_bytes<OptFamily>(model, cap);
}

extern "C" int b2t_clm_cache_plan_host(const int32_t* cache_ids_host, int cache_n, int cap, const int32_t* ids_host,
                                       const int32_t* seq_off_host, int n_seq, int* trunk, int* common, int* reused,
                                       long long* n_nodes, long long* n_rows, int* n_after) {
  const char* who = "b2t_clm_cache_plan_host";
  B2T_REQUIRE(ids_host && seq_off_host && (cache_ids_host || cache_n == 0), "%s: null argument", who);
  B2T_REQUIRE(cap >= 1, "%s: cap %d < 1", who, cap);
  B2T_REQUIRE(cache_n >= 0 && cache_n <= cap, "%s: n %d outside [0, cap %d]", who, cache_n, cap);
  if (int rc = clm_check_lists(who, ids_host, seq_off_host, n_seq, 0, 0)) return rc;
  const ClmCachePlan p = clm_cache_plan(cache_ids_host, cache_n, cap, ids_host, seq_off_host, n_seq);
  if (trunk) *trunk = p.Tn;
  if (common) *common = p.P;
  if (reused) *reused = p.R;
  if (n_after) *n_after = p.n_after;
  if (n_nodes || n_rows) {
    std::vector<int32_t> node((size_t)seq_off_host[n_seq]);
    const long long Mn = tree_plan(ids_host, seq_off_host, n_seq, node.data(), nullptr, 0, nullptr);
    if (n_nodes) *n_nodes = Mn;
    if (n_rows) *n_rows = Mn - p.R;
  }
  return 0;
}

extern "C" size_t b2t_clm_tree_cached_ws_bytes(const b2t_clm_t* model, long long n_rows, long long n_tokens, int n_seq) {
  return clm_family_tree_cached_ws_bytes<OptFamily>(model, n_rows, n_tokens, n_seq);
}

extern "C" int b2t_clm_score_tree_cached_f16(const b2t_clm_t* model, b2t_clm_cache_t* cache, int update, const int32_t* ids_host,
                                             const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                             long long* n_rows_out, int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  return clm_family_score_tree_cached<OptPolicy, OptFamily>("b2t_clm_score_tree_cached_f16", "b2t_clm_score_tree_f16", model, cache,
                                                            update, ids_host, seq_off_host, n_seq, scores_out, tok_logp_out,
                                                            n_rows_out, n_reused_out, ws, ws_bytes, stream);
}
