// clm_attn.h — the attention arithmetic of the causal-LM forward, written once (device code, internal linkage).  Every
// attention kernel -- clm_attn_kernel and clm_attn_tree_kernel (launched by causal_lm.hip, causal_lm_tree.hip and, in bf16,
// causal_lm_llama_bf16.hip), clm_attn_tree_cached_kernel and clm_attn_trunk_kernel (launched by causal_lm_cache.hip), all at the
// end of this file, their soft-capped `_cap_` forms (causal_lm_gemma2.hip), their head-dim-96 instances (causal_lm_phi3.hip) and the
// flat and tree `_sink_` forms with a sink logit and a sliding window (causal_lm_gptoss.hip) -- walks its own rows and calls attn_block per 32-key block, so a query meets the same operands in
// the same order on every path: that is what keeps the paths bit-identical.  The element type E (ClmElem, clm_internal.h)
// is deduced from the pointers: _Float16 everywhere but in the bf16 unit.
//
// The score tile is computed transposed, S^T = K . Q^T (v_mfma_f32_32x32x16_f16 / _bf16: A = 32 keys, B = 32 queries), so a lane owns
// one query column: its online-softmax state (m, l) is per lane and the row reductions are in-lane plus one swap of the lane
// halves.  P^T is then the B operand of O^T = V^T . P^T with no data movement (registers 8s..8s+7 of the accumulator are
// k-step s, keys in the order 16s + 8(j >> 2) + 4h + (j & 3)), and O^T's rescale by exp(m_old - m_new) is per lane too.
// Throughout: lane = 32 * hh + li; D is the head dim (64, 80, 96, 128 or 256), KS its k-steps, NF its 32-dim fragments of O^T; the
// `dim < D` guards exist only where NF * 32 != D (head dim 80).
// CAP (Gemma-2, causal_lm_gemma2.hip): the fp32 score tile is soft-capped, s = cap * tanh(s / cap), before the mask and the
// running max; cap == 0 at run time means off.  CAP is false in every kernel without `_cap_` in its name: the body functions
// below are inlined into them with the cap's code compiled out.
#pragma once
#include <limits.h>
#include <math.h>

#include "clm_internal.h"

namespace b2t {
namespace {

using f32x4 = float __attribute__((ext_vector_type(4)));
using half8 = ClmElem<_Float16>::v8;

template <int D>
struct AttnDims {
  static constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  static constexpr bool GUARD = NF * 32 != D;
  static_assert(32 * PCS == 64 * NIT, "a V block is a whole number of 16-byte pieces per lane");
};

// Where the V operand of a key block comes from.  at(key, dim): V[key of the block][dim] (key < 32).
// Global gather (the flat kernel): row k0 + key of Vb at pitch RS, zero beyond the sequence's L rows; nothing to wait for.
template <class E>
struct VGather {
  const E* Vb; long long RS; int k0, L;
  __device__ __forceinline__ void ready() const {}
  __device__ __forceinline__ E at(int key, int dim) const {
    return k0 + key < L ? Vb[(long long)(k0 + key) * RS + dim] : (E)0.f;
  }
};
// The wave's own LDS slab (the tree, cached and trunk kernels), staged by stage_v: row pitch VP = D + 8, so that the two lane
// halves, 4 keys apart, fall on disjoint banks.  The slab is private to the wave: a wave barrier orders its writes and reads.
template <int D, class E = _Float16>
struct VSlab {
  const E* vs;
  __device__ __forceinline__ void ready() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the slab is written
  }
  __device__ __forceinline__ E at(int key, int dim) const { return vs[key * AttnDims<D>::VP + dim]; }
};

// Stage a 32 x D V block into the slab as whole 16-byte row pieces: piece p = 64 * it + lane is columns 8c .. 8c + 7 of block
// key p / PCS, whose V row is vrow(key); the rows of keys >= nvalid are zeroed (not read).
template <int D, class E, class VRow>
__device__ __forceinline__ void stage_v(E* vs, int lane, int nvalid, VRow&& vrow) {
  using A = AttnDims<D>;
  using vec8 = typename ClmElem<E>::v8;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();   // the previous block's reads of the slab are done
#pragma unroll
  for (int it = 0; it < A::NIT; ++it) {
    const int p = 64 * it + lane, key = p / A::PCS, c = p % A::PCS;
    const E* row = vrow(key);
    vec8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (E)0.f;
    if (key < nvalid) v = *reinterpret_cast<const vec8*>(row + 8 * c);
    *reinterpret_cast<vec8*>(vs + key * A::VP + 8 * c) = v;
  }
}

// the lane's Q fragment: qp = the query row's head + 8 * hh
template <int D, class E>
__device__ __forceinline__ void load_q(const E* qp, typename ClmElem<E>::v8* qf) {
#pragma unroll
  for (int ks = 0; ks < AttnDims<D>::KS; ++ks) qf[ks] = *reinterpret_cast<const typename ClmElem<E>::v8*>(qp + 16 * ks);
}

template <int D>
__device__ __forceinline__ void attn_zero(float& m, float& l, f32x16* o) {
  m = -INFINITY; l = 0.f;
#pragma unroll
  for (int f = 0; f < AttnDims<D>::NF; ++f)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[f][e] = 0.f;
}

// One key block of the online softmax: S^T = K . Q^T from the lane's key row kp (+ 8 * hh), the mask (keys beyond the query q
// or the L keys; MASK false = no key of the block can be either), the per-lane state update, P rounded to the element type,
// O^T += V^T . P^T with V from `v`.  CAP: the scores are soft-capped first (soft_cap; cap > 0).
// tanh(u) is written 1 - 2 / (exp(2u) + 1) like gelu_new's (clm_gemm.h): a saturated argument yields +-1, never inf / inf.
__device__ __forceinline__ float soft_cap(float v, float cap, float inv_cap) {
  return cap * (1.0f - 2.0f / (expf(2.0f * (v * inv_cap)) + 1.0f));
}
// WIN: keys at or below q - W are masked as well (the sliding window; W >= 1).
template <int D, bool MASK, bool CAP = false, bool WIN = false, class E, class VSrc>
__device__ __forceinline__ void attn_block(const E* kp, const typename ClmElem<E>::v8* qf, const VSrc& v, int k0, int q, int L,
                                           int li, int hh, float& m, float& l, f32x16* o, float cap = 0.f, int W = 0) {
  using A = AttnDims<D>;
  using vec8 = typename ClmElem<E>::v8;
  f32x16 sacc;
#pragma unroll
  for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < A::KS; ++ks)
    sacc = ClmElem<E>::mfma(*reinterpret_cast<const vec8*>(kp + 16 * ks), qf[ks], sacc);
  if (CAP) {
    if (cap > 0.f) {   // uniform
      const float inv_cap = 1.0f / cap;
#pragma unroll
      for (int e = 0; e < 16; ++e) sacc[e] = soft_cap(sacc[e], cap, inv_cap);
    }
  }
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    if (MASK) {
      const int key = k0 + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (key > q || key >= L) sacc[e] = -INFINITY;
      if (WIN) {
        if (key <= q - W) sacc[e] = -INFINITY;
      }
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
  vec8 pb[2];
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int j = 0; j < 8; ++j) pb[s2][j] = (E)sacc[8 * s2 + j];
  v.ready();
#pragma unroll
  for (int f = 0; f < A::NF; ++f) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[f][e] *= alpha;
    const int dim = 32 * f + li;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      vec8 va;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3);
        va[j] = !A::GUARD || dim < D ? v.at(key, dim) : (E)0.f;
      }
      o[f] = ClmElem<E>::mfma(va, pb[s2], o[f]);
    }
  }
}

// the lane's query row of the output, o * (1 / l) in the C / D layout: op = the output row's head
template <int D, class E>
__device__ __forceinline__ void attn_store(E* op, const f32x16* o, float l, int hh) {
  const float inv = 1.0f / l;
#pragma unroll
  for (int f = 0; f < AttnDims<D>::NF; ++f)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int dim = 32 * f + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (!AttnDims<D>::GUARD || dim < D) op[dim] = (E)(o[f][e] * inv);
    }
}

// ---- the flat and the tree kernel ----
// Templates on the head dim and the element type; a unit instantiates what it launches: causal_lm.hip the flat kernel and
// causal_lm_tree.hip the tree kernel in fp16 (head dims 64, 80 and 128, behind clm_launch_attn / clm_launch_attn_tree),
// causal_lm_llama_bf16.hip both in bf16 (64 and 128).

// Causal attention, one workgroup per (sequence, query head), 4 waves; a wave takes 32 query rows at a time and runs the key
// blocks up to the diagonal through attn_block, V gathered from global memory.  The row is q[Hq * D] | k[Hkv * D] |
// v[Hkv * D]; query head h reads K / V head h / (Hq / Hkv) (OPT: Hkv = Hq).
//
// clm_attn_flat is the body; SLAB stages V through the wave's LDS slab as the tree kernel does (the same values reach the same
// MFMAs, so the bits are VGather's) -- the capped kernel at head dim 256 needs the registers the gather holds.
//
// SINK / WIN (gpt-oss, causal_lm_gptoss.hip; both false in every other kernel, their code compiled out).  SINK: head h has a
// learned logit sinks[h] in the softmax's denominator and nowhere else, so a query's state starts at (m, l, o) = (sinks[h], 1, 0)
// in place of (-inf, 0, 0).  WIN: key j is visible to query i iff i - W < j <= i (W <= 0 at run time: no window); the key loop
// starts at the first block that holds a visible key of the block's lowest query, 32 qb, and attn_block masks the keys at or
// below i - W in the blocks that remain.  Which blocks a query meets depends on its position alone, on every path.
template <int D, class E, bool CAP, bool SLAB, bool SINK = false, bool WIN = false>
__device__ __forceinline__ void clm_attn_flat(const E* qkv, E* out, const int* seq_off, int Hq, int Hkv, float cap,
                                              const float* sinks = nullptr, int W = 0) {
  const int sq = blockIdx.x, h = blockIdx.y, hk = h / (Hq / Hkv);
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = (long long)(Hq + 2 * Hkv) * D;
  const E* Qb = qkv + (long long)t0 * RS + h * D;
  const E* Kb = qkv + (long long)t0 * RS + (Hq + hk) * D;
  const E* Vb = Kb + Hkv * D;
  const int nqb = (L + 31) / 32;
  if constexpr (WIN) { if (W <= 0) W = INT_MAX; }   // no window: q - W < 0 for every query
  for (int qb = wave; qb < nqb; qb += 4) {
    const int q = qb * 32 + li;
    typename ClmElem<E>::v8 qf[AttnDims<D>::KS];
    load_q<D>(Qb + (long long)min(q, L - 1) * RS + 8 * hh, qf);
    float m, l;
    f32x16 o[AttnDims<D>::NF];
    attn_zero<D>(m, l, o);
    if constexpr (SINK) { m = sinks[h]; l = 1.f; }
    int kb = 0;
    if constexpr (WIN) kb = max(qb * 32 - W + 1, 0) / 32;   // the block of the lowest query's first visible key
    for (; kb <= qb; ++kb) {   // key blocks up to the diagonal; key k0 <= q0 < L is valid for every query row
      const int k0 = kb * 32;
      const E* kp = Kb + (long long)min(k0 + li, L - 1) * RS + 8 * hh;
      if constexpr (SLAB) {
        __shared__ __attribute__((aligned(16))) E vslab[4][32 * AttnDims<D>::VP];
        stage_v<D>(vslab[wave], lane, L - k0, [&](int key) { return Vb + (long long)(k0 + key) * RS; });
        attn_block<D, true, CAP, WIN>(kp, qf, VSlab<D, E>{vslab[wave]}, k0, q, L, li, hh, m, l, o, cap, W);
      } else {
        attn_block<D, true, CAP, WIN>(kp, qf, VGather<E>{Vb, RS, k0, L}, k0, q, L, li, hh, m, l, o, cap, W);
      }
    }
    if (q < L) attn_store<D>(out + ((long long)(t0 + q) * Hq + h) * D, o, l, hh);
  }
}
template <int D, class E = _Float16>
__global__ __launch_bounds__(256) void clm_attn_kernel(const E* qkv, E* out, const int* seq_off, int Hq, int Hkv) {
  clm_attn_flat<D, E, false, false>(qkv, out, seq_off, Hq, Hkv, 0.f);
}
template <int D, class E, bool SLAB>
__global__ __launch_bounds__(256) void clm_attn_cap_kernel(const E* qkv, E* out, const int* seq_off, int Hq, int Hkv, float cap) {
  clm_attn_flat<D, E, true, SLAB>(qkv, out, seq_off, Hq, Hkv, cap);
}
// gpt-oss: sinks fp32 [Hq]; W the layer's window, 0 = full causal attention
template <int D, class E>
__global__ __launch_bounds__(256) void clm_attn_sink_kernel(const E* qkv, E* out, const int* seq_off, int Hq, int Hkv,
                                                            const float* sinks, int W) {
  clm_attn_flat<D, E, false, false, true, true>(qkv, out, seq_off, Hq, Hkv, 0.f, sinks, W);
}

// Causal attention over tree paths, one workgroup per (sequence, query head), 4 waves; a wave takes 32 query positions at a
// time, starting with the 32-aligned block that holds the sequence's first owned position.  Position i of the sequence is row
// path[i] = tok_node[seq_off[s] + i] of qkv: K and V are gathered for all positions 0..q, Q is read and the output row is
// written only for owned positions (fact (a) of causal_lm_tree.hip's header).  The arithmetic per query is clm_attn_kernel's:
// the same attn_block over the same key blocks, on the same row layout q[Hq * D] | k[Hkv * D] | v[Hkv * D].
// The gather: a lane holds the row of key k0 + (lane & 31) and reads K from it as 16-byte pieces; V's 32 x D block is staged
// as whole 16-byte row pieces into the wave's own LDS slab and read back transposed, rows of keys beyond the path zeroed.
// The slab is private to the wave, so the key loop needs no workgroup barrier.
// SINK / WIN as in clm_attn_flat: a position is the depth along the path, so the window's rule is the flat kernel's on path
// positions, and a query at position i meets the key blocks the flat kernel's query i meets.
template <int D, class E, bool CAP, bool SINK = false, bool WIN = false>
__device__ __forceinline__ void clm_attn_tree(const E* qkv, E* out, const int* seq_off, const int* tok_node, const int* own_start,
                                              int Hq, int Hkv, float cap, const float* sinks = nullptr, int W = 0) {
  __shared__ __attribute__((aligned(16))) E vslab[4][32 * AttnDims<D>::VP];
  const int sq = blockIdx.x, h = blockIdx.y, hk = h / (Hq / Hkv);
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0, own = own_start[sq];
  if (own >= L) return;   // every node of this path is owned by an earlier sequence
  const int* path = tok_node + t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const long long RS = (long long)(Hq + 2 * Hkv) * D;
  const E* Qb = qkv + h * D;
  const E* Kb = qkv + (Hq + hk) * D;
  const E* Vb = Kb + Hkv * D;
  E* vs = vslab[wave];
  const int nqb = (L + 31) / 32;
  if constexpr (WIN) { if (W <= 0) W = INT_MAX; }   // no window: q - W < 0 for every query
  for (int qb = own / 32 + wave; qb < nqb; qb += 4) {
    const int q = qb * 32 + li;
    const int qrow = path[min(q, L - 1)];
    typename ClmElem<E>::v8 qf[AttnDims<D>::KS];
    load_q<D>(Qb + (long long)qrow * RS + 8 * hh, qf);
    float m, l;
    f32x16 o[AttnDims<D>::NF];
    attn_zero<D>(m, l, o);
    if constexpr (SINK) { m = sinks[h]; l = 1.f; }
    int kb = 0;
    if constexpr (WIN) kb = max(qb * 32 - W + 1, 0) / 32;   // the block of the lowest query's first visible key
    for (; kb <= qb; ++kb) {   // key blocks up to the diagonal; key k0 <= q0 < L is valid for every query row
      const int k0 = kb * 32;
      const int krow = path[min(k0 + li, L - 1)];
      stage_v<D>(vs, lane, L - k0, [&](int key) { return Vb + (long long)__shfl(krow, key) * RS; });
      attn_block<D, true, CAP, WIN>(Kb + (long long)krow * RS + 8 * hh, qf, VSlab<D, E>{vs}, k0, q, L, li, hh, m, l, o, cap, W);
    }
    if (q >= own && q < L) attn_store<D>(out + ((long long)qrow * Hq + h) * D, o, l, hh);
  }
}
template <int D, class E = _Float16>
__global__ __launch_bounds__(256) void clm_attn_tree_kernel(const E* qkv, E* out, const int* seq_off, const int* tok_node,
                                                            const int* own_start, int Hq, int Hkv) {
  clm_attn_tree<D, E, false>(qkv, out, seq_off, tok_node, own_start, Hq, Hkv, 0.f);
}
template <int D, class E>
__global__ __launch_bounds__(256) void clm_attn_tree_cap_kernel(const E* qkv, E* out, const int* seq_off, const int* tok_node,
                                                                const int* own_start, int Hq, int Hkv, float cap) {
  clm_attn_tree<D, E, true>(qkv, out, seq_off, tok_node, own_start, Hq, Hkv, cap);
}
template <int D, class E>
__global__ __launch_bounds__(256) void clm_attn_tree_sink_kernel(const E* qkv, E* out, const int* seq_off, const int* tok_node,
                                                                 const int* own_start, int Hq, int Hkv, const float* sinks, int W) {
  clm_attn_tree<D, E, false, true, true>(qkv, out, seq_off, tok_node, own_start, Hq, Hkv, 0.f, sinks, W);
}

// ---- the cached tree kernel and the trunk kernel (the context cache: causal_lm_cache.hip has the rule and the launches) ----

// clm_attn_tree_kernel with a two-source gather, on the row layout the flat and tree kernels share (query head h reads K / V
// head hk = h / (Hq / Hkv); OPT is Hkv = Hq): path node < R is row `node` of the cache's layer slab ([cap][2 * Hkv * D],
// k[Hkv * D] | v[Hkv * D]), else row node - R of this call's qkv ([rows][(Hq + 2 * Hkv) * D], q | k | v).  In both a row's V
// sits Hkv * D elements behind its K, so one address per key row serves both; the select is on the address (base and pitch),
// not around the loads, which are 16-byte pieces (stage_v and attn_block, clm_attn.h).  Queries start at max(own_start, R);
// out has the computed rows.  With st_o set (stage B) the key loop starts at block kb0 = Rb / 32 from the state
// clm_attn_trunk_kernel left for the query's row: st_ml [rows][Hq][2], st_o [rows][Hq * D].
// The body is clm_attn_tree_cached; the `_cap_` kernel (Gemma-2) soft-caps the scores in attn_block, the plain one compiles the
// cap out (clm_attn.h).
template <int D, bool CAP>
__device__ __forceinline__ void clm_attn_tree_cached(const _Float16* qkv, const _Float16* slab, _Float16* out, const int* seq_off,
                                                     const int* tok_node, const int* own_start, int Hkv, int R, const float* st_ml,
                                                     const float* st_o, int kb0, float cap) {
  constexpr int NF = AttnDims<D>::NF;
  __shared__ __attribute__((aligned(16))) _Float16 vslab[4][32 * AttnDims<D>::VP];
  const int sq = blockIdx.x, h = blockIdx.y, H = gridDim.y, hk = h / (H / Hkv);
  const int t0 = seq_off[sq], L = seq_off[sq + 1] - t0, start = max(own_start[sq], R);
  if (start >= L) return;   // every node of this path is owned by an earlier sequence or held by the cache
  const int* path = tok_node + t0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, hh = lane >> 5;
  const int d = H * D, vo = Hkv * D;     // the output row; V behind K in both sources
  const long long RS = (long long)(H + 2 * Hkv) * D, CS = 2LL * vo;
  const _Float16* Qb = qkv + h * D;
  const _Float16* Kq = qkv + (H + hk) * D;   // K of a computed row
  const _Float16* Kc = slab + hk * D;        // K of a cached row
  auto krow_of = [&](int node) {
    const bool c = node < R;
    return (c ? Kc : Kq) + (long long)(c ? node : node - R) * (c ? CS : RS);
  };
  _Float16* vs = vslab[wave];
  const int nqb = (L + 31) / 32;
  for (int qb = start / 32 + wave; qb < nqb; qb += 4) {
    const int q = qb * 32 + li;
    const bool live = q >= start && q < L;
    const int qrow = max(path[min(q, L - 1)] - R, 0);   // lanes below R read row 0 and write nothing
    half8 qf[AttnDims<D>::KS];
    load_q<D>(Qb + (long long)qrow * RS + 8 * hh, qf);
    float m, l;
    f32x16 o[NF];
    attn_zero<D>(m, l, o);
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
      stage_v<D>(vs, lane, L - k0, [&](int key) { return krow_of(__shfl(knode, key)) + vo; });
      attn_block<D, true, CAP>(krow_of(knode) + 8 * hh, qf, VSlab<D>{vs}, k0, q, L, li, hh, m, l, o, cap);
    }
    if (live) attn_store<D>(out + (long long)qrow * d + h * D, o, l, hh);
  }
}
template <int D>
__global__ __launch_bounds__(256) void clm_attn_tree_cached_kernel(const _Float16* qkv, const _Float16* slab, _Float16* out,
                                                                   const int* seq_off, const int* tok_node, const int* own_start,
                                                                   int Hkv, int R, const float* st_ml, const float* st_o, int kb0) {
  clm_attn_tree_cached<D, false>(qkv, slab, out, seq_off, tok_node, own_start, Hkv, R, st_ml, st_o, kb0, 0.f);
}
template <int D>
__global__ __launch_bounds__(256) void clm_attn_tree_cached_cap_kernel(const _Float16* qkv, const _Float16* slab, _Float16* out,
                                                                       const int* seq_off, const int* tok_node,
                                                                       const int* own_start, int Hkv, int R, const float* st_ml,
                                                                       const float* st_o, int kb0, float cap) {
  clm_attn_tree_cached<D, true>(qkv, slab, out, seq_off, tok_node, own_start, Hkv, R, st_ml, st_o, kb0, cap);
}

// Stage B: the cached key blocks 0 .. nkb-1 (keys [0, Rb), contiguous slab rows, no mask) for 32 computed rows at a time, a
// wave per (row block, query head), reading slab head hk.  Leaves m, l (st_ml [rows][Hq][2]) and the unnormalised o (st_o
// [rows][Hq * D]) of every row < rows.
template <int D, bool CAP>
__device__ __forceinline__ void clm_attn_trunk(const _Float16* qkv, const _Float16* slab, int Hkv, int rows, int nkb, float* st_ml,
                                               float* st_o, float cap) {
  constexpr int NF = AttnDims<D>::NF;
  __shared__ __attribute__((aligned(16))) _Float16 vs[32 * AttnDims<D>::VP];
  const int h = blockIdx.y, H = gridDim.y, hk = h / (H / Hkv);
  const int lane = threadIdx.x, li = lane & 31, hh = lane >> 5;
  const int d = H * D, vo = Hkv * D;
  const long long RS = (long long)(H + 2 * Hkv) * D, CS = 2LL * vo;
  const int r = blockIdx.x * 32 + li, row = min(r, rows - 1);
  const _Float16* Kc = slab + hk * D;
  half8 qf[AttnDims<D>::KS];
  load_q<D>(qkv + h * D + (long long)row * RS + 8 * hh, qf);
  float m, l;
  f32x16 o[NF];
  attn_zero<D>(m, l, o);
  for (int kb = 0; kb < nkb; ++kb) {
    const int k0 = kb * 32;
    stage_v<D>(vs, lane, 32, [&](int key) { return Kc + (long long)(k0 + key) * CS + vo; });
    attn_block<D, false, CAP>(Kc + (long long)(k0 + li) * CS + 8 * hh, qf, VSlab<D>{vs}, k0, 0, 0, li, hh, m, l, o, cap);
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
template <int D>
__global__ __launch_bounds__(64) void clm_attn_trunk_kernel(const _Float16* qkv, const _Float16* slab, int Hkv, int rows, int nkb,
                                                            float* st_ml, float* st_o) {
  clm_attn_trunk<D, false>(qkv, slab, Hkv, rows, nkb, st_ml, st_o, 0.f);
}
template <int D>
__global__ __launch_bounds__(64) void clm_attn_trunk_cap_kernel(const _Float16* qkv, const _Float16* slab, int Hkv, int rows, int nkb,
                                                                float* st_ml, float* st_o, float cap) {
  clm_attn_trunk<D, true>(qkv, slab, Hkv, rows, nkb, st_ml, st_o, cap);
}

}  // namespace
}  // namespace b2t
