// clm_attn.h — the attention arithmetic of the causal-LM forward, written once (device code, internal linkage).  Every
// attention kernel -- clm_attn_kernel (causal_lm.hip), clm_attn_tree_kernel (causal_lm_tree.hip), clm_attn_tree_cached_kernel
// and clm_attn_trunk_kernel (causal_lm_cache.hip) -- walks its own rows and calls attn_block per 32-key block, so a query
// meets the same operands in the same order on every path: that is what keeps the paths bit-identical.
//
// The score tile is computed transposed, S^T = K . Q^T (v_mfma_f32_32x32x16_f16: A = 32 keys, B = 32 queries), so a lane owns
// one query column: its online-softmax state (m, l) is per lane and the row reductions are in-lane plus one swap of the lane
// halves.  P^T is then the B operand of O^T = V^T . P^T with no data movement (registers 8s..8s+7 of the accumulator are
// k-step s, keys in the order 16s + 8(j >> 2) + 4h + (j & 3)), and O^T's rescale by exp(m_old - m_new) is per lane too.
// Throughout: lane = 32 * hh + li; D is the head dim (64, 80 or 128), KS its k-steps, NF its 32-dim fragments of O^T; the
// `dim < D` guards exist only where NF * 32 != D (head dim 80).
#pragma once
#include <math.h>

#include "clm_internal.h"

namespace b2t {
namespace {

using f32x16 = float __attribute__((ext_vector_type(16)));
using f32x4 = float __attribute__((ext_vector_type(4)));
using half8 = _Float16 __attribute__((ext_vector_type(8)));

template <int D>
struct AttnDims {
  static constexpr int KS = D / 16, NF = (D + 31) / 32, VP = D + 8, PCS = D / 8, NIT = PCS / 2;
  static constexpr bool GUARD = NF * 32 != D;
  static_assert(32 * PCS == 64 * NIT, "a V block is a whole number of 16-byte pieces per lane");
};

// Where the V operand of a key block comes from.  at(key, dim): V[key of the block][dim] (key < 32).
// Global gather (the flat kernel): row k0 + key of Vb at pitch RS, zero beyond the sequence's L rows; nothing to wait for.
struct VGather {
  const _Float16* Vb; long long RS; int k0, L;
  __device__ __forceinline__ void ready() const {}
  __device__ __forceinline__ _Float16 at(int key, int dim) const {
    return k0 + key < L ? Vb[(long long)(k0 + key) * RS + dim] : (_Float16)0.f;
  }
};
// The wave's own LDS slab (the tree, cached and trunk kernels), staged by stage_v: row pitch VP = D + 8, so that the two lane
// halves, 4 keys apart, fall on disjoint banks.  The slab is private to the wave: a wave barrier orders its writes and reads.
template <int D>
struct VSlab {
  const _Float16* vs;
  __device__ __forceinline__ void ready() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the slab is written
  }
  __device__ __forceinline__ _Float16 at(int key, int dim) const { return vs[key * AttnDims<D>::VP + dim]; }
};

// Stage a 32 x D V block into the slab as whole 16-byte row pieces: piece p = 64 * it + lane is columns 8c .. 8c + 7 of block
// key p / PCS, whose V row is vrow(key); the rows of keys >= nvalid are zeroed (not read).
template <int D, class VRow>
__device__ __forceinline__ void stage_v(_Float16* vs, int lane, int nvalid, VRow&& vrow) {
  using A = AttnDims<D>;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();   // the previous block's reads of the slab are done
#pragma unroll
  for (int it = 0; it < A::NIT; ++it) {
    const int p = 64 * it + lane, key = p / A::PCS, c = p % A::PCS;
    const _Float16* row = vrow(key);
    half8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (_Float16)0.f;
    if (key < nvalid) v = *reinterpret_cast<const half8*>(row + 8 * c);
    *reinterpret_cast<half8*>(vs + key * A::VP + 8 * c) = v;
  }
}

// the lane's Q fragment: qp = the query row's head + 8 * hh
template <int D>
__device__ __forceinline__ void load_q(const _Float16* qp, half8* qf) {
#pragma unroll
  for (int ks = 0; ks < AttnDims<D>::KS; ++ks) qf[ks] = *reinterpret_cast<const half8*>(qp + 16 * ks);
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
// or the L keys; MASK false = no key of the block can be either), the per-lane state update, P rounded to fp16,
// O^T += V^T . P^T with V from `v`.
template <int D, bool MASK, class VSrc>
__device__ __forceinline__ void attn_block(const _Float16* kp, const half8* qf, const VSrc& v, int k0, int q, int L, int li,
                                           int hh, float& m, float& l, f32x16* o) {
  using A = AttnDims<D>;
  f32x16 sacc;
#pragma unroll
  for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < A::KS; ++ks)
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
  v.ready();
#pragma unroll
  for (int f = 0; f < A::NF; ++f) {
#pragma unroll
    for (int e = 0; e < 16; ++e) o[f][e] *= alpha;
    const int dim = 32 * f + li;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      half8 va;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = 16 * s2 + 8 * (j >> 2) + 4 * hh + (j & 3);
        va[j] = !A::GUARD || dim < D ? v.at(key, dim) : (_Float16)0.f;
      }
      o[f] = __builtin_amdgcn_mfma_f32_32x32x16_f16(va, pb[s2], o[f], 0, 0, 0);
    }
  }
}

// the lane's query row of the output, o * (1 / l) in the C / D layout: op = the output row's head
template <int D>
__device__ __forceinline__ void attn_store(_Float16* op, const f32x16* o, float l, int hh) {
  const float inv = 1.0f / l;
#pragma unroll
  for (int f = 0; f < AttnDims<D>::NF; ++f)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int dim = 32 * f + (e & 3) + 8 * (e >> 2) + 4 * hh;
      if (!AttnDims<D>::GUARD || dim < D) op[dim] = (_Float16)(o[f][e] * inv);
    }
}

}  // namespace
}  // namespace b2t
