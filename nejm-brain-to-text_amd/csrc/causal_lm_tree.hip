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
// The forward runs over n_nodes rows instead of n_tokens: embedding, LayerNorm, the four GEMMs per layer and the fused LM
// head are causal_lm.hip's kernels through the launchers of clm_internal.h (B2T_CLM_GEMM_256 applies through launch_gemm).
// New here are the attention, which reaches its rows through the sequence's path, and the gathered per-sequence sum.  The
// head has one row per non-root node: source = the parent's row, target = the node's id.
//
// Numerics: causal_lm.hip's contract, and bit-identical to the flat path: the attention keeps a query's arithmetic order
// (key blocks of 32 aligned at position 0, query blocks 32-aligned too, online softmax per lane, P rounded to fp16 per block),
// and a sequence's log-probs are added along its path in token order by one thread.
#include <math.h>
#include <unordered_map>
#include <vector>

#include "clm_internal.h"

namespace b2t {
namespace {

using f32x16 = float __attribute__((ext_vector_type(16)));
using half8 = _Float16 __attribute__((ext_vector_type(8)));

// Causal attention over tree paths, one workgroup per (sequence, head), 4 waves; a wave takes 32 query positions at a time,
// starting with the 32-aligned block that holds the sequence's first owned position.  Position i of the sequence is row
// path[i] = tok_node[seq_off[s] + i] of qkv: K and V are gathered for all positions 0..q, Q is read and the output row is
// written only for owned positions (fact (a) of the file header).  The arithmetic per query is clm_attn_kernel's: S^T = K . Q^T,
// a lane owns one query column and its online-softmax state, P^T is the B operand of O^T = V^T . P^T.
// The gather: a lane holds the row of key k0 + (lane & 31) and reads K from it as 16-byte pieces; V's 32 x D block is staged
// as whole 16-byte row pieces into the wave's own LDS slab (row pitch D + 8: the two lane halves, 4 keys apart, fall on
// disjoint banks) and read back transposed, rows of keys beyond the path zeroed.  The slab is private to the wave, so the
// key loop needs no workgroup barrier.
template <int D>
__global__ __launch_bounds__(256) void clm_attn_tree_kernel(const _Float16* qkv, _Float16* out, const int* seq_off,
                                                            const int* tok_node, const int* own_start, int d) {
  constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  static_assert(32 * PCS == 64 * NIT, "a V block is a whole number of 16-byte pieces per lane");
  __shared__ __attribute__((aligned(16))) _Float16 vslab[4][32 * VP];
  const int sq = blockIdx.x, h = blockIdx.y;
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0, own = own_start[sq];
  if (own >= L) return;   // every node of this path is owned by an earlier sequence
  const int* path = tok_node + t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = 3LL * d;
  const _Float16* Qb = qkv + h * D;
  const _Float16* Kb = Qb + d;
  const _Float16* Vb = Qb + 2 * d;
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
    for (int kb = 0; kb <= qb; ++kb) {   // key blocks up to the diagonal; key k0 <= q0 < L is valid for every query row
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
          for (int j = 0; j < 8; ++j) {
            const int key = 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3);
            va[j] = dim < D ? vs[key * VP + dim] : (_Float16)0.f;
          }
          o[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb[s2], o[f], 0, 0, 0);
        }
      }
    }
    if (q >= own && q < L) {
      const float inv = 1.0f / l;
      _Float16* op = out + (long long)qrow * d + h * D;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int dim = 32 * f + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (dim < D) op[dim] = (_Float16)(o[f][e] * inv);
        }
    }
  }
}

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

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline long long rup(long long x, long long m) { return (x + m - 1) / m * m; }

}  // namespace

// The layout and the plan have external linkage (clm_internal.h): causal_lm_cache.hip sizes and plans its call with them.
size_t tree_ints(long long Mn, long long M, int n_seq) { return (size_t)(4 * Mn + 2 * M + 2 * (long long)n_seq + 1); }

TreeLayout tree_layout(const b2t_clm_t* m, long long Mn, long long M, int n_seq) {
  TreeLayout L{};
  const long long d = m->d_model;
  L.Mp = rup(Mn, CLM_ROWPAD); L.ncg = (m->vocab + 63) / 64;
  size_t off = 0;
  L.ints = off;   off += al256(sizeof(int) * tree_ints(Mn, M, n_seq));
  L.resid = off;  off += al256(sizeof(float) * (size_t)(Mn * d));
  L.x16 = off;    off += al256(sizeof(_Float16) * (size_t)(L.Mp * d));
  L.qkv = off;    off += al256(sizeof(_Float16) * (size_t)(Mn * 3 * d));
  L.hbuf = off;   off += al256(sizeof(_Float16) * (size_t)(L.Mp * m->ffn_dim));
  L.pmax = off;   off += al256(sizeof(float) * (size_t)(Mn * L.ncg));
  L.psum = off;   off += al256(sizeof(float) * (size_t)(Mn * L.ncg));
  L.tlogit = off; off += al256(sizeof(float) * (size_t)Mn);
  L.logp = off;   off += al256(sizeof(float) * (size_t)Mn);
  L.total = off;
  return L;
}

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
  B2T_REQUIRE(ids_host && seq_off_host && node_of_token && n_nodes && (parent_of_node || cap <= 0),
              "b2t_clm_tree_plan_host: null argument");
  B2T_REQUIRE(n_seq >= 1, "b2t_clm_tree_plan_host: n_seq %d < 1", n_seq);
  B2T_REQUIRE(seq_off_host[0] == 0, "b2t_clm_tree_plan_host: seq_off[0] = %d, expected 0", seq_off_host[0]);
  for (int s = 0; s < n_seq; ++s)
    B2T_REQUIRE(seq_off_host[s + 1] > seq_off_host[s], "b2t_clm_tree_plan_host: sequence %d is empty", s);
  *n_nodes = tree_plan(ids_host, seq_off_host, n_seq, node_of_token, parent_of_node, cap < 0 ? 0 : cap, nullptr);
  if (*n_nodes > cap) {
    set_error("b2t_clm_tree_plan_host: %lld nodes, room for %lld", *n_nodes, cap);
    return -2;
  }
  return 0;
}

extern "C" size_t b2t_clm_tree_ws_bytes(const b2t_clm_t* model, long long n_nodes, long long n_tokens, int n_seq) {
  if (!model || n_nodes < 1 || n_nodes > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  return tree_layout(model, n_nodes, n_tokens, n_seq).total;
}

extern "C" int b2t_clm_score_tree_f16(const b2t_clm_t* model, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq,
                                      float* scores_out, float* tok_logp_out, long long* n_nodes_out, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (int rc = clm_check_model(model)) return rc;
  const b2t_clm_t& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "b2t_clm_score_tree_f16: null argument");
  B2T_REQUIRE(n_seq >= 1, "b2t_clm_score_tree_f16: n_seq %d < 1", n_seq);
  B2T_REQUIRE(seq_off_host[0] == 0, "b2t_clm_score_tree_f16: seq_off[0] = %d, expected 0", seq_off_host[0]);
  for (int s = 0; s < n_seq; ++s) {
    const long long n = (long long)seq_off_host[s + 1] - seq_off_host[s];
    B2T_REQUIRE(n >= 1, "b2t_clm_score_tree_f16: sequence %d is empty", s);
    B2T_REQUIRE(n <= m.max_pos, "b2t_clm_score_tree_f16: sequence %d has %lld tokens, more than max_pos %d", s, n, m.max_pos);
  }
  const long long M = seq_off_host[n_seq];
  for (long long t = 0; t < M; ++t)
    B2T_REQUIRE(ids_host[t] >= 0 && ids_host[t] < m.vocab, "b2t_clm_score_tree_f16: token %lld has id %d outside [0, %d)", t,
                ids_host[t], m.vocab);

  // the plan, then the index arrays in upload order: node_id[Mn] node_pos[Mn] head_src[Mn] head_tgt[Mn] (Mh used)
  // tok_node[M] tok_hrow[M] seq_off[n+1] own_start[n]
  static thread_local std::vector<int32_t> tok_node, parent, own, host;
  tok_node.resize((size_t)M); parent.resize((size_t)M); own.resize((size_t)n_seq);
  const long long Mn = tree_plan(ids_host, seq_off_host, n_seq, tok_node.data(), parent.data(), M, own.data());
  if (n_nodes_out) *n_nodes_out = Mn;
  const TreeLayout L = tree_layout(model, Mn, M, n_seq);
  B2T_REQUIRE(ws_bytes >= L.total, "b2t_clm_score_tree_f16: workspace of %zu bytes, %zu needed", ws_bytes, L.total);
  const hipStream_t s = as_stream(stream);
  const int d = m.d_model, H = m.n_heads, hd = d / H, F = m.ffn_dim;

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
                         "b2t_clm_score_tree_f16 upload"))
    return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), "b2t_clm_score_tree_f16 upload")) return rc;

  float* resid = reinterpret_cast<float*>(base + L.resid);
  _Float16* x16 = reinterpret_cast<_Float16*>(base + L.x16);
  _Float16* qkv = reinterpret_cast<_Float16*>(base + L.qkv);
  _Float16* hb = reinterpret_cast<_Float16*>(base + L.hbuf);
  auto H16 = [](const void* p) { return static_cast<const _Float16*>(p); };
  const _Float16* et = H16(m.embed_tokens);

  if (int rc = clm_launch_embed(d_id, d_pos, et, H16(m.embed_positions), resid, d, Mn, s)) return rc;
  for (int l = 0; l < m.n_layers; ++l) {
    const b2t_clm_layer_t& w = m.layers_host[l];
    if (int rc = clm_launch_layernorm(resid, nullptr, Mn, H16(w.ln1_w), H16(w.ln1_b), x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = H16(w.qkv_w); g.M = (int)Mn; g.N = 3 * d; g.K = d; g.bias = H16(w.qkv_b); g.out16 = qkv; g.ldo = 3 * d;
    g.qscale = 1.0f / sqrtf((float)hd); g.qcols = d;
    if (int rc = launch_gemm<EP_F16>(g, s)) return rc;
    if (hd == 64) hipLaunchKernelGGL(clm_attn_tree_kernel<64>, dim3(n_seq, H), dim3(256), 0, s, qkv, x16, d_soff, d_node, d_own, d);
    else if (hd == 80) hipLaunchKernelGGL(clm_attn_tree_kernel<80>, dim3(n_seq, H), dim3(256), 0, s, qkv, x16, d_soff, d_node, d_own, d);
    else hipLaunchKernelGGL(clm_attn_tree_kernel<128>, dim3(n_seq, H), dim3(256), 0, s, qkv, x16, d_soff, d_node, d_own, d);
    B2T_CHECK_LAUNCH("clm_attn_tree_kernel");
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.out_w); g.M = (int)Mn; g.N = d; g.K = d; g.bias = H16(w.out_b); g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
    if (int rc = clm_launch_layernorm(resid, nullptr, Mn, H16(w.ln2_w), H16(w.ln2_b), x16, d, s)) return rc;
    g = ClmGemm{};
    g.A = x16; g.B = H16(w.fc1_w); g.M = (int)Mn; g.N = F; g.K = d; g.bias = H16(w.fc1_b); g.out16 = hb; g.ldo = F;
    if (int rc = launch_gemm<EP_RELU>(g, s)) return rc;
    g = ClmGemm{};
    g.A = hb; g.B = H16(w.fc2_w); g.M = (int)Mn; g.N = d; g.K = F; g.bias = H16(w.fc2_b); g.resid = resid; g.ldo = d;
    if (int rc = launch_gemm<EP_RESID>(g, s)) return rc;
  }
  float* logp = reinterpret_cast<float*>(base + L.logp);
  if (Mh > 0) {
    if (int rc = clm_launch_layernorm(resid, d_src, Mh, H16(m.final_ln_w), H16(m.final_ln_b), x16, d, s)) return rc;
    ClmGemm g{};
    g.A = x16; g.B = et; g.M = (int)Mh; g.N = m.vocab; g.K = d;
    g.pmax = reinterpret_cast<float*>(base + L.pmax); g.psum = reinterpret_cast<float*>(base + L.psum);
    g.tlogit = reinterpret_cast<float*>(base + L.tlogit); g.tgt = d_tgt; g.ncg = (int)L.ncg;
    if (int rc = launch_gemm<EP_HEAD>(g, s)) return rc;
    if (int rc = clm_launch_head_combine(g.pmax, g.psum, g.tlogit, g.ncg, logp, Mh, s)) return rc;
  }
  return clm_launch_seq_sum_tree(logp, d_soff, d_hrow, scores_out, tok_logp_out, n_seq, s);
}
