// causal_lm_cache.hip — the shared-prefix tree forward of causal_lm_tree.hip behind a context cache
// (b2t_clm_score_tree_cached_f16).  In closed-loop decoding every rescoring call scores its candidates behind the decoding
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

#include "clm_internal.h"

namespace b2t {
namespace {

using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using half8 = _Float16 __attribute__((ext_vector_type(8)));

// One key block of clm_attn_tree_kernel's online softmax, operand for operand: S^T = K . Q^T from the lane's key row kp,
// the mask (keys beyond the query or the path; `masked` false = no key of the block can be either), the per-lane state
// update, P rounded to fp16, O^T += V^T . P^T from the wave's LDS slab vs (written by the caller before the second barrier).
template <int D, bool MASK>
__device__ __forceinline__ void attn_block(const _Float16* kp, const half8* qf, const _Float16* vs, int k0, int q, int L, int li,
                                           int hh, float& m, float& l, f32x16* o) {
  constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8;
  f32x16 sacc;
#pragma unroll
  for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
    sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(*reinterpret_cast<const half8*>(kp + 16 * ks), qf[ks], sacc, 0, 0, 0);
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (MASK) {
      const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (key > q || key >= L) sacc[e] = -INFINITY;
    }
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

// clm_attn_tree_kernel with a two-source gather: path node < R is row `node` of the cache's layer slab ([cap][2d], K then V),
// else row node - R of this call's qkv ([rows][3d], Q K V).  In both a row's V sits d elements behind its K, so one address
// per key row serves both; the select is on the address (base and pitch), the loads behind it are unconditional 16-byte
// pieces.  Queries start at max(own_start, R); out has the computed rows.  With st_o set (stage B) the key loop starts at
// block kb0 = Rb / 32 from the state clm_attn_trunk_kernel left for the query's row: st_ml [rows][H][2], st_o [rows][d].
template <int D>
__global__ __launch_bounds__(256) void clm_attn_tree_cached_kernel(const _Float16* qkv, const _Float16* slab, _Float16* out,
                                                                   const int* seq_off, const int* tok_node, const int* own_start,
                                                                   int d, int R, const float* st_ml, const float* st_o, int kb0) {
  constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  static_assert(32 * PCS == 64 * NIT, "a V block is a whole number of 16-byte pieces per lane");
  __shared__ __attribute__((aligned(16))) _Float16 vslab[4][32 * VP];
  const int sq = blockIdx.x, h = blockIdx.y, H = gridDim.y;
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0, start = max(own_start[sq], R);
  if (start >= L) return;   // every node of this path is owned by an earlier sequence or held by the cache
  const int* path = tok_node + t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = 3LL * d, CS = 2LL * d;
  const _Float16* Qb = qkv + h * D;
  const _Float16* Kq = Qb + d;           // K of a computed row; its V is d further
  const _Float16* Kc = slab + h * D;     // K of a cached row; its V is d further
  _Float16* vs = vslab[wave];
  const int nqb = (L + 31) / 32;
  for (int qb = start / 32 + wave; qb < nqb; qb += 4) {
    const int q0 = qb * 32, q = q0 + li;
    const bool live = q >= start && q < L;
    const int qrow = max(path[min(q, L - 1)] - R, 0);   // lanes below R read row 0 and write nothing
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
    if (st_o) {   // wave-uniform
      const float* mp = st_ml + ((long long)qrow * H + h) * 2;
      const float m_in = mp[0], l_in = mp[1];
      if (live) { m = m_in; l = l_in; }
      const float* op = st_o + (long long)qrow * d + h * D + 4 * hh;
#pragma unroll
      for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          if (32 * f + 8 * g < D) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(op + 32 * f + 8 * g);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[f][4 * g + j] = live ? v[j] : 0.f;
          }
        }
    }
    for (int kb = kb0; kb <= qb; ++kb) {   // key blocks up to the diagonal; key k0 <= q0 < L is valid for every query row
      const int k0 = kb * 32;
      const int knode = path[min(k0 + li, L - 1)];
      const bool kc = knode < R;
      const _Float16* krow = (kc ? Kc : Kq) + (long long)(kc ? knode : knode - R) * (kc ? CS : RS);
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();   // the previous block's reads of the slab are done
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int p = 64 * it + lane, key = p / PCS, c = p % PCS;
        const int vnode = __shfl(knode, key);
        const bool vc = vnode < R;
        const _Float16* vrow = (vc ? Kc : Kq) + (long long)(vc ? vnode : vnode - R) * (vc ? CS : RS) + d;
        half8 v = *reinterpret_cast<const half8*>(vrow + 8 * c);   // the row is clamped to the path: always readable
        if (k0 + key >= L) {
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
        }
        *reinterpret_cast<half8*>(vs + key * VP + 8 * c) = v;
      }
      attn_block<D, true>(krow + 8 * hh, qf, vs, k0, q, L, li, hh, m, l, o);
    }
    if (live) {
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

// Stage B: the cached key blocks 0 .. nkb-1 (keys [0, Rb), contiguous slab rows, no mask) for 32 computed rows at a time, a
// wave per (row block, head).  Leaves m, l (st_ml [rows][H][2]) and the unnormalised o (st_o [rows][d]) of every row < rows.
template <int D>
__global__ __launch_bounds__(64) void clm_attn_trunk_kernel(const _Float16* qkv, const _Float16* slab, int d, int rows, int nkb,
                                                            float* st_ml, float* st_o) {
  constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  __shared__ __attribute__((aligned(16))) _Float16 vs[32 * VP];
  const int h = blockIdx.y, H = gridDim.y;
  const int lane = threadIdx.x, li = lane & 31, hh = lane >> 5;
  const long long RS = 3LL * d, CS = 2LL * d;
  const int r = blockIdx.x * 32 + li, row = min(r, rows - 1);
  const _Float16* qp = qkv + h * D + (long long)row * RS + 8 * hh;
  const _Float16* Kc = slab + h * D;
  half8 qf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + 16 * ks);
  float m = -INFINITY, l = 0.f;
  f32x16 o[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[f][e] = 0.f;
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * 32;
    const _Float16* krow = Kc + (long long)(k0 + li) * CS;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the previous block's reads of the slab are done
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int p = 64 * it + lane, key = p / PCS, c = p % PCS;
      *reinterpret_cast<half8*>(vs + key * VP + 8 * c) =
          *reinterpret_cast<const half8*>(Kc + (long long)(k0 + key) * CS + d + 8 * c);
    }
    attn_block<D, false>(krow + 8 * hh, qf, vs, k0, 0, 0, li, hh, m, l, o);
  }
  if (r < rows) {
    if (hh == 0) {
      float* mp = st_ml + ((long long)row * H + h) * 2;
      mp[0] = m; mp[1] = l;
    }
    float* op = st_o + (long long)row * d + h * D + 4 * hh;
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        if (32 * f + 8 * g < D) {
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = o[f][4 * g + j];
          *reinterpret_cast<f32x4*>(op + 32 * f + 8 * g) = v;
        }
      }
  }
}

// cache append: K | V of the trunk's computed rows (qkv rows 0..rows-1, columns d..3d) -> dst rows 0.. ([.][2d], the layer slab
// at row R), as 16-byte pieces
__global__ __launch_bounds__(256) void clm_cache_append_kernel(const _Float16* qkv, _Float16* dst, int d, long long rows) {
  const int pcs = d / 4;   // 2d / 8 pieces per row
  const long long n = rows * pcs;
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += gridDim.x * 256LL) {
    const long long r = i / pcs;
    const int c = (int)(i % pcs);
    *reinterpret_cast<half8*>(dst + r * 2 * d + 8 * c) = *reinterpret_cast<const half8*>(qkv + r * 3 * d + d + 8 * c);
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

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct CachePlan { int Tn, P, R, n_after; };

// The rule of the file header.  Sequences are non-empty, seq_off[0] == 0, 0 <= cache_n <= cap.
CachePlan cache_plan(const int32_t* cache_ids, int cache_n, int cap, const int32_t* ids, const int32_t* seq_off, int n_seq) {
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
  CachePlan p;
  p.Tn = (int)Tn; p.P = (int)P; p.R = P > 0 ? (int)P - 1 : 0;
  p.n_after = (int)(Tn < cap ? Tn : cap);
  return p;
}

// the state of stage B behind the tree layout: m, l per (row, head) and the unnormalised o per row
struct CachedLayout { TreeLayout T; size_t st_ml, st_o, total; };

CachedLayout cached_layout(const b2t_clm_t* m, long long rows, long long M, int n_seq) {
  CachedLayout L{};
  L.T = tree_layout(m, rows, M, n_seq);
  size_t off = L.T.total;
  L.st_ml = off; off += al256(sizeof(float) * (size_t)(rows * m->n_heads * 2));
  L.st_o = off;  off += al256(sizeof(float) * (size_t)(rows * m->d_model));
  L.total = off;
  return L;
}

constexpr bool CLM_TRUNK_ATTN_DEFAULT = false;

// B2T_CLM_TRUNK_ATTN, read per call: 0 = every key block in clm_attn_tree_cached_kernel (stage A); 1 = the cached blocks in
// clm_attn_trunk_kernel (stage B).
bool trunk_attn_on() {
  const char* e = getenv("B2T_CLM_TRUNK_ATTN");
  return e && *e ? atoi(e) != 0 : CLM_TRUNK_ATTN_DEFAULT;
}

template <int D>
int launch_attn(const _Float16* qkv, const _Float16* slab, _Float16* out, const int* soff, const int* node, const int* own, int d,
                int H, int n_seq, int R, long long rows, bool trunk, float* st_ml, float* st_o, hipStream_t s) {
  const int Rb = trunk ? R - R % 32 : 0;
  if (Rb > 0) {
    hipLaunchKernelGGL(clm_attn_trunk_kernel<D>, dim3((unsigned)((rows + 31) / 32), H), dim3(64), 0, s, qkv, slab, d, (int)rows,
                       Rb / 32, st_ml, st_o);
    B2T_CHECK_LAUNCH("clm_attn_trunk_kernel");
  }
  hipLaunchKernelGGL(clm_attn_tree_cached_kernel<D>, dim3(n_seq, H), dim3(256), 0, s, qkv, slab, out, soff, node, own, d, R,
                     Rb > 0 ? st_ml : nullptr, Rb > 0 ? st_o : nullptr, Rb / 32);
  B2T_CHECK_LAUNCH("clm_attn_tree_cached_kernel");
  return 0;
}

int check_lists(const char* who, const int32_t* ids_host, const int32_t* seq_off_host, int n_seq, int vocab, int max_pos) {
  B2T_REQUIRE(n_seq >= 1, "%s: n_seq %d < 1", who, n_seq);
  B2T_REQUIRE(seq_off_host[0] == 0, "%s: seq_off[0] = %d, expected 0", who, seq_off_host[0]);
  for (int s = 0; s < n_seq; ++s) {
    const long long n = (long long)seq_off_host[s + 1] - seq_off_host[s];
    B2T_REQUIRE(n >= 1, "%s: sequence %d is empty", who, s);
    B2T_REQUIRE(max_pos <= 0 || n <= max_pos, "%s: sequence %d has %lld tokens, more than max_pos %d", who, s, n, max_pos);
  }
  if (vocab > 0) {
    const long long M = seq_off_host[n_seq];
    for (long long t = 0; t < M; ++t)
      B2T_REQUIRE(ids_host[t] >= 0 && ids_host[t] < vocab, "%s: token %lld has id %d outside [0, %d)", who, t, ids_host[t], vocab);
  }
  return 0;
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_clm_cache_kv_bytes(const b2t_clm_t* model, int cap) {
  if (!model || cap < 1 || cap > model->max_pos || model->n_layers < 1 || model->d_model < 1) return 0;
  return (size_t)model->n_layers * (size_t)cap * 2 * (size_t)model->d_model * sizeof(_Float16);
}

extern "C" int b2t_clm_cache_plan_host(const int32_t* cache_ids_host, int cache_n, int cap, const int32_t* ids_host,
                                       const int32_t* seq_off_host, int n_seq, int* trunk, int* common, int* reused,
                                       long long* n_nodes, long long* n_rows, int* n_after) {
  const char* who = "b2t_clm_cache_plan_host";
  B2T_REQUIRE(ids_host && seq_off_host && (cache_ids_host || cache_n == 0), "%s: null argument", who);
  B2T_REQUIRE(cap >= 1, "%s: cap %d < 1", who, cap);
  B2T_REQUIRE(cache_n >= 0 && cache_n <= cap, "%s: n %d outside [0, cap %d]", who, cache_n, cap);
  if (int rc = check_lists(who, ids_host, seq_off_host, n_seq, 0, 0)) return rc;
  const CachePlan p = cache_plan(cache_ids_host, cache_n, cap, ids_host, seq_off_host, n_seq);
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
  if (!model || n_rows < 1 || n_rows > n_tokens || n_seq < 1 || n_seq > n_tokens) return 0;
  return cached_layout(model, n_rows, n_tokens, n_seq).total;
}

extern "C" int b2t_clm_score_tree_cached_f16(const b2t_clm_t* model, b2t_clm_cache_t* cache, int update, const int32_t* ids_host,
                                             const int32_t* seq_off_host, int n_seq, float* scores_out, float* tok_logp_out,
                                             long long* n_rows_out, int* n_reused_out, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "b2t_clm_score_tree_cached_f16";
  if (int rc = clm_check_model(model)) return rc;
  const b2t_clm_t& m = *model;
  B2T_REQUIRE(ids_host && seq_off_host && scores_out && ws, "%s: null argument", who);
  B2T_REQUIRE(cache, "%s: null cache (callers without one use b2t_clm_score_tree_f16)", who);
  B2T_REQUIRE(cache->kv && cache->logp && cache->ids_host, "%s: null cache member", who);
  B2T_REQUIRE(cache->cap >= 1, "%s: cache cap %d < 1", who, cache->cap);
  B2T_REQUIRE(cache->cap <= m.max_pos, "%s: cache cap %d above max_pos %d", who, cache->cap, m.max_pos);
  B2T_REQUIRE(cache->n >= 0 && cache->n <= cache->cap, "%s: cache n %d outside [0, cap %d]", who, cache->n, cache->cap);
  for (int t = 0; t < cache->n; ++t)
    B2T_REQUIRE(cache->ids_host[t] >= 0 && cache->ids_host[t] < m.vocab, "%s: cached token %d has id %d outside [0, %d)", who, t,
                cache->ids_host[t], m.vocab);
  if (int rc = check_lists(who, ids_host, seq_off_host, n_seq, m.vocab, m.max_pos)) return rc;
  const long long M = seq_off_host[n_seq];

  // the tree plan and the rule; the index arrays in upload order, over the computed rows (node n is row n - R):
  // row_id[rows] row_pos[rows] head_src[rows] head_tgt[rows] (Mh used) tok_node[M] tok_hrow[M] seq_off[n+1] own_start[n]
  static thread_local std::vector<int32_t> tok_node, parent, own, host;
  tok_node.resize((size_t)M); parent.resize((size_t)M); own.resize((size_t)n_seq);
  const long long Mn = tree_plan(ids_host, seq_off_host, n_seq, tok_node.data(), parent.data(), M, own.data());
  const CachePlan P = cache_plan(cache->ids_host, cache->n, cache->cap, ids_host, seq_off_host, n_seq);
  const int R = P.R;
  const long long rows = Mn - R;
  if (n_rows_out) *n_rows_out = rows;
  if (n_reused_out) *n_reused_out = R;
  const CachedLayout CL = cached_layout(model, rows, M, n_seq);
  const TreeLayout& L = CL.T;
  B2T_REQUIRE(ws_bytes >= CL.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, CL.total);
  const hipStream_t s = as_stream(stream);
  const int d = m.d_model, H = m.n_heads, hd = d / H, F = m.ffn_dim;
  const bool trunk = trunk_attn_on();

  host.assign(tree_ints(rows, M, n_seq), 0);
  int* h_id = host.data(); int* h_pos = h_id + rows; int* h_src = h_pos + rows; int* h_tgt = h_src + rows;
  int* h_node = h_tgt + rows; int* h_hrow = h_node + M; int* h_soff = h_hrow + M; int* h_own = h_soff + n_seq + 1;
  for (int q = 0; q < n_seq; ++q) {
    const int a = seq_off_host[q], b = seq_off_host[q + 1];
    h_soff[q] = a; h_own[q] = own[q];
    for (int t = a; t < b; ++t) {
      const int n = tok_node[t];
      h_node[t] = n;
      if (n >= R) { h_id[n - R] = ids_host[t]; h_pos[n - R] = t - a; }   // the true position: R + the row's depth below R
    }
  }
  h_soff[n_seq] = (int)M;
  long long Mh = 0;   // head rows: the non-root nodes > R in node order, source = the parent's row, target = the node's id
  {
    std::vector<int32_t>& hrow = parent;   // parent[n] is read before hrow[n] is written
    for (long long n = 0; n < Mn; ++n) {
      const int p = parent[n];
      if (n > R && p >= 0) { h_src[Mh] = p - R; h_tgt[Mh] = h_id[n - R]; hrow[n] = (int32_t)Mh++; }
      else hrow[n] = 0;
    }
    for (long long t = 0; t < M; ++t) h_hrow[t] = hrow[tok_node[t]];
  }
  // what the cache gains: positions R .. n_after - 1 (K | V rows 0.. of qkv, head rows 0.. of logp)
  const int app_rows = update && P.n_after > R ? P.n_after - R : 0;
  const int app_logp = update && P.n_after > R + 1 ? P.n_after - R - 1 : 0;

  char* base = static_cast<char*>(ws);
  int* d_id = reinterpret_cast<int*>(base + L.ints);
  int* d_pos = d_id + rows; int* d_src = d_pos + rows; int* d_tgt = d_src + rows; int* d_node = d_tgt + rows;
  int* d_hrow = d_node + M; int* d_soff = d_hrow + M; int* d_own = d_soff + n_seq + 1;
  if (int rc = check_hip(hipMemcpyAsync(d_id, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s), who)) return rc;
  // the staging vector is reused by the next call on this thread: wait for the copy out of it
  if (int rc = check_hip(hipStreamSynchronize(s), who)) return rc;

  float* resid = reinterpret_cast<float*>(base + L.resid);
  _Float16* x16 = reinterpret_cast<_Float16*>(base + L.x16);
  _Float16* qkv = reinterpret_cast<_Float16*>(base + L.qkv);
  _Float16* hb = reinterpret_cast<_Float16*>(base + L.hbuf);
  float* logp = reinterpret_cast<float*>(base + L.logp);
  float* st_ml = reinterpret_cast<float*>(base + CL.st_ml);
  float* st_o = reinterpret_cast<float*>(base + CL.st_o);
  auto H16 = [](const void* p) { return static_cast<const _Float16*>(p); };
  const _Float16* et = H16(m.embed_tokens);
  _Float16* kv = static_cast<_Float16*>(cache->kv);
  const size_t slab_elems = (size_t)cache->cap * 2 * d;

  // from here on rows >= R of the cache may be overwritten: an error return leaves it at min(n, R)
  auto forward = [&]() -> int {
    if (int rc = clm_launch_embed(d_id, d_pos, et, H16(m.embed_positions), resid, d, rows, s)) return rc;
    for (int l = 0; l < m.n_layers; ++l) {
      const b2t_clm_layer_t& w = m.layers_host[l];
      _Float16* slab = kv + (size_t)l * slab_elems;
      if (int rc = clm_launch_layernorm(resid, nullptr, rows, H16(w.ln1_w), H16(w.ln1_b), x16, d, s)) return rc;
      ClmGemm g{};
      g.A = x16; g.B = H16(w.qkv_w); g.M = (int)rows; g.N = 3 * d; g.K = d; g.bias = H16(w.qkv_b); g.out16 = qkv; g.ldo = 3 * d;
      g.qscale = 1.0f / sqrtf((float)hd); g.qcols = d;
      if (int rc = launch_gemm<EP_F16>(g, s)) return rc;
      if (app_rows > 0) {
        const long long pieces = (long long)app_rows * (d / 4);
        hipLaunchKernelGGL(clm_cache_append_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, qkv,
                           slab + (size_t)R * 2 * d, d, (long long)app_rows);
        B2T_CHECK_LAUNCH("clm_cache_append_kernel");
      }
      int rc;
      if (hd == 64) rc = launch_attn<64>(qkv, slab, x16, d_soff, d_node, d_own, d, H, n_seq, R, rows, trunk, st_ml, st_o, s);
      else if (hd == 80) rc = launch_attn<80>(qkv, slab, x16, d_soff, d_node, d_own, d, H, n_seq, R, rows, trunk, st_ml, st_o, s);
      else rc = launch_attn<128>(qkv, slab, x16, d_soff, d_node, d_own, d, H, n_seq, R, rows, trunk, st_ml, st_o, s);
      if (rc) return rc;
      g = ClmGemm{};
      g.A = x16; g.B = H16(w.out_w); g.M = (int)rows; g.N = d; g.K = d; g.bias = H16(w.out_b); g.resid = resid; g.ldo = d;
      if (int rc2 = launch_gemm<EP_RESID>(g, s)) return rc2;
      if (int rc2 = clm_launch_layernorm(resid, nullptr, rows, H16(w.ln2_w), H16(w.ln2_b), x16, d, s)) return rc2;
      g = ClmGemm{};
      g.A = x16; g.B = H16(w.fc1_w); g.M = (int)rows; g.N = F; g.K = d; g.bias = H16(w.fc1_b); g.out16 = hb; g.ldo = F;
      if (int rc2 = launch_gemm<EP_RELU>(g, s)) return rc2;
      g = ClmGemm{};
      g.A = hb; g.B = H16(w.fc2_w); g.M = (int)rows; g.N = d; g.K = F; g.bias = H16(w.fc2_b); g.resid = resid; g.ldo = d;
      if (int rc2 = launch_gemm<EP_RESID>(g, s)) return rc2;
    }
    if (Mh > 0) {
      if (int rc = clm_launch_layernorm(resid, d_src, Mh, H16(m.final_ln_w), H16(m.final_ln_b), x16, d, s)) return rc;
      ClmGemm g{};
      g.A = x16; g.B = et; g.M = (int)Mh; g.N = m.vocab; g.K = d;
      g.pmax = reinterpret_cast<float*>(base + L.pmax); g.psum = reinterpret_cast<float*>(base + L.psum);
      g.tlogit = reinterpret_cast<float*>(base + L.tlogit); g.tgt = d_tgt; g.ncg = (int)L.ncg;
      if (int rc = launch_gemm<EP_HEAD>(g, s)) return rc;
      if (int rc = clm_launch_head_combine(g.pmax, g.psum, g.tlogit, g.ncg, logp, Mh, s)) return rc;
    }
    if (app_logp > 0) {
      hipLaunchKernelGGL(clm_cache_logp_kernel, dim3((app_logp + 255) / 256), dim3(256), 0, s, logp, cache->logp + R + 1, app_logp);
      B2T_CHECK_LAUNCH("clm_cache_logp_kernel");
    }
    hipLaunchKernelGGL(clm_seq_sum_tree_cached_kernel, dim3(n_seq), dim3(64), 0, s, logp, cache->logp, R, d_soff, d_hrow, scores_out,
                       tok_logp_out);
    B2T_CHECK_LAUNCH("clm_seq_sum_tree_cached_kernel");
    return 0;
  };
  if (int rc = forward()) {
    if (update && cache->n > R) cache->n = R;
    return rc;
  }
  if (update) {
    for (int t = R; t < P.n_after; ++t) cache->ids_host[t] = ids_host[t];
    cache->n = P.n_after;
  }
  return 0;
}
