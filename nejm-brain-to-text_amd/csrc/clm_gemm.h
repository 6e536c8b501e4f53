// clm_gemm.h — the 16-bit tile GEMM of the causal-LM forward with its fused epilogues (the design notes are in the header of
// causal_lm.hip).  A kernel template with internal linkage, on the tile, the epilogue and the element type E (_Float16 by
// default, __bf16: ClmElem of clm_internal.h; only the MFMA and the conversions of bias and out16 depend on it, the 16-byte
// global and LDS traffic does not): a translation unit instantiates what it launches -- causal_lm.hip the four epilogues of
// the OPT forward in fp16 (its launch_gemm serves the tree and cache paths too), causal_lm_llama.hip the two of the Llama
// family in fp16 (rotary embedding on q | k, SwiGLU), causal_lm_llama_bf16.hip the four of the Llama forward in bf16,
// causal_lm_qwen3.hip the one Qwen3 adds (EP_QKNORM_ROPE: the per-head q / k RMSNorm in front of the rotation) in both,
// causal_lm_gpt2.hip the one GPT-2 adds (EP_GELU: gelu_new where OPT's fc1 has ReLU) in fp16, causal_lm_neox.hip the two
// GPT-NeoX adds (EP_ROPE_PART: the rotation of only the first rotary_ndims dims of a head; EP_GELU_ERF) in fp16, causal_lm_olmo2.hip the two OLMo-2 adds
// (EP_F32 and EP_QKV_F32: fp32 stores for the norms over a whole output row) in both, causal_lm_mixtral.hip the grouped form of
// the tile (clm_gemm_grouped_kernel: one B matrix per expert) with EP_SWIGLU and EP_F32 in both, causal_lm_gemma2.hip the two
// Gemma-2 adds (EP_GEGLU: gelu_new where SwiGLU has silu; EP_HEAD_CAP: the fused head on soft-capped logits) in both,
// causal_lm_phi3.hip EP_QKV_F32 again in both (Phi-3's rotation reads the fp32 q | k columns in a kernel of its own),
// causal_lm_gptoss.hip the two gpt-oss adds to the grouped tile (EP_OSS_GLU, EP_F32_BIAS: per-expert biases) in both,
// causal_lm_gptoss_mx.hip those two on the packed form of the grouped tile (clm_gemm_grouped_mx_kernel: B in MXFP4),
// causal_lm_llama_fp8.hip the Llama and Qwen3 layers' four on the packed form of the plain tile (clm_gemm_fp8_kernel: B in
// block-scaled FP8) in both.  Which
// tile a GEMM gets is decided in one place, launch_gemm of causal_lm.hip, for either element type; clm_gemm_tiles below only
// launches it.
#pragma once
#include <math.h>

#include "clm_internal.h"

namespace b2t {
namespace {

constexpr int CK = 64, CPITCH = CK + 8;      // k tile; LDS row pitch in 2-byte elements (144 B)
constexpr int ROWPAD = CLM_ROWPAD;                  // A operands and weights are padded to this many rows

// ClmGemm (the GEMM's arguments) and the EP_* epilogue ids: clm_internal.h

__device__ __forceinline__ float warp32_max(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float warp32_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// gelu_new (GPT-2's tanh form): 0.5 v (1 + tanh(u)), u = sqrt(2 / pi) (v + 0.044715 v^3), in fp32.  tanh(u) is written
// 1 - 2 / (exp(2u) + 1): exp(2u) = inf gives 1 and exp(2u) = 0 gives -1, so a saturated pre-activation yields v or -0.0 / 0,
// never inf / inf; expf is the full-range one (no scratch, no call).
__device__ __forceinline__ float gelu_new(float v) {
  const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
  const float th = 1.0f - 2.0f / (expf(2.0f * u) + 1.0f);
  return 0.5f * v * (1.0f + th);
}

// the erf GELU (GPT-NeoX / Pythia's "gelu"): 0.5 v (1 + erf(v / sqrt 2)) in fp32.  erff saturates to +-1, so a saturated
// pre-activation yields v or -0.0 / 0, never NaN.
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.7071067811865476f)); }

// MXFP4 -> E: the eight values of 4 bytes of e2m1 nibbles (low nibble first: element 2i is byte i's low nibble) times
// 2^(sb - 127), sb the block's E8M0 scale byte, as eight E in element order -- the uint4 that the dense path loads from a matrix
// of (E)(float)(value * 2^(sb - 127)), rounded to nearest even.  No table in memory and no per-element branch: a byte permute
// looks the magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6 up as the high byte of an fp16 (the low byte is 0), four at a time; the sign
// bit is or-ed in; a second permute interleaves the even and the odd elements into four fp16 pairs.  Those pairs are exact,
// and one multiplication by a power of two, whose one rounding is the contract's, does the rest:
//   fp16  a packed fp16 multiply.  2^(sb - 127) is an fp16 only for sb in [103, 142], so the table holds the values times 2^-13
//         (sb <= 128; 0.5 * 2^-13 is the smallest normal) or times 4 (sb > 128) and the factor is 2^(sb - 114) or 2^(sb - 129),
//         a normal fp16 for 100 <= sb <= 144.  Below 100 the largest value, 6 * 2^-28, rounds to zero, and the factor is 0, which
//         keeps the signs; above 144 only zero nibbles are finite, and the factor stays 2^15.  The subnormal results (sb < 114)
//         are the multiplier's own rounding to nearest even (fp16 denormals are never flushed on this target).
//   bf16  the pair widened to fp32 (exact) times 2^(sb - 127) in fp32 (exact: at most two significant bits, and bf16 has fp32's
//         exponent range, its subnormals included), of which the upper halves are the bf16s.
// A scale byte of 255 (NaN) has no defined result: the loader refuses it.  The one definition: the packed grouped tile below
// and b2t_clm_mxfp4_unpack_f16 / _bf16 (causal_lm_gptoss_mx.hip) call it.
template <int REF>   // the table: values * 2^-13 (0), * 4 (1) or * 1 (2), as fp16 pairs (element 2i, element 2i + 1) of byte i
__device__ __forceinline__ void mxfp4_pairs_f16(unsigned q, unsigned (&p)[4], bool hi = false) {
  constexpr unsigned T0[3] = {0x0A080400u, 0x46444000u, 0x3E3C3800u}, T1[3] = {0x12100E0Cu, 0x4E4C4A48u, 0x46444240u};
  unsigned t0 = T0[REF], t1 = T1[REF];
  if (REF == 0 && hi) { t0 = T0[1]; t1 = T1[1]; }
  const unsigned ev = q & 0x0F0F0F0Fu, od = (q >> 4) & 0x0F0F0F0Fu;   // elements 0, 2, 4, 6 and 1, 3, 5, 7, one a byte
  const unsigned he = __builtin_amdgcn_perm(t1, t0, ev & 0x07070707u) | ((ev & 0x08080808u) << 4);
  const unsigned ho = __builtin_amdgcn_perm(t1, t0, od & 0x07070707u) | ((od & 0x08080808u) << 4);
  p[0] = __builtin_amdgcn_perm(ho, he, 0x040C000Cu); p[1] = __builtin_amdgcn_perm(ho, he, 0x050C010Cu);
  p[2] = __builtin_amdgcn_perm(ho, he, 0x060C020Cu); p[3] = __builtin_amdgcn_perm(ho, he, 0x070C030Cu);
}
template <class E>
__device__ __forceinline__ uint4 mxfp4_unpack8(unsigned q, unsigned sb);
template <>
__device__ __forceinline__ uint4 mxfp4_unpack8<_Float16>(unsigned q, unsigned sb) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const bool hi = sb > 128u;
  const unsigned ex = hi ? (sb < 144u ? sb : 144u) - 114u : (sb > 99u ? sb - 99u : 0u);   // the factor's exponent field
  const unsigned f = (ex << 10) * 0x10001u;
  unsigned p[4];
  mxfp4_pairs_f16<0>(q, p, hi);
  uint4 r;
  unsigned* o = &r.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const h2 v = __builtin_bit_cast(h2, p[i]) * __builtin_bit_cast(h2, f);
    o[i] = __builtin_bit_cast(unsigned, v);
  }
  return r;
}
template <>
__device__ __forceinline__ uint4 mxfp4_unpack8<__bf16>(unsigned q, unsigned sb) {
  typedef _Float16 h2 __attribute__((ext_vector_type(2)));
  const float f = __builtin_bit_cast(float, sb ? sb << 23 : 0x00400000u);   // 2^(sb - 127); 2^-127 is an fp32 subnormal
  unsigned p[4];
  mxfp4_pairs_f16<2>(q, p);
  uint4 r;
  unsigned* o = &r.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const h2 v = __builtin_bit_cast(h2, p[i]);
    const unsigned lo = __builtin_bit_cast(unsigned, (float)v[0] * f), up = __builtin_bit_cast(unsigned, (float)v[1] * f);
    o[i] = __builtin_amdgcn_perm(up, lo, 0x07060302u);
  }
  return r;
}

// FP8 -> E: the eight values of 8 bytes of OCP e4m3fn codes (element i is byte i; q.x holds elements 0..3) times the block's
// fp32 scale s, as eight E in element order -- the uint4 that the dense path loads from a matrix of (E)((float)code * s).  Two
// roundings, in the loader's order (llm_rescore.fp8_dequant, then the cast): the code widened to fp32 (exact, the e4m3
// subnormals included), one fp32 multiplication rounded to nearest even with subnormal products kept, one conversion to E
// rounded to nearest even with subnormal results kept (this target never flushes either).  Codes 0x7F and 0xFF (NaN) have no
// defined result: the loader refuses them; a product that is not finite in E is refused there too.  The one definition: the
// packed plain tile below and b2t_clm_fp8_unpack_f16 / _bf16 (causal_lm_llama_fp8.hip) call it.
template <class E>
__device__ __forceinline__ uint4 fp8_unpack8(uint2 q, float s) {
  typedef E e2 __attribute__((ext_vector_type(2)));
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 v[4] = {__builtin_amdgcn_cvt_pk_f32_fp8((int)q.x, false), __builtin_amdgcn_cvt_pk_f32_fp8((int)q.x, true),
                   __builtin_amdgcn_cvt_pk_f32_fp8((int)q.y, false), __builtin_amdgcn_cvt_pk_f32_fp8((int)q.y, true)};
  uint4 r;
  unsigned* o = &r.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    e2 p;
    p[0] = (E)(v[i][0] * s); p[1] = (E)(v[i][1] * s);
    o[i] = __builtin_bit_cast(unsigned, p);
  }
  return r;
}

// how a tile reads its B operand: 16-bit elements, MXFP4 (the grouped tile alone) or block-scaled FP8 (the plain tile alone)
enum { PK_DENSE = 0, PK_MXFP4 = 1, PK_FP8 = 2 };

// BM x BN block tile, WGM x WGN waves, each wave (BM / WGM) x 64 = FM x 2 fragments of 32 x 32.  E is the element type of
// A, B, bias and out16 (ClmElem, clm_internal.h).  This is the body of both kernels below.  GROUPED (routed experts,
// clm_moe.h): B is a stack of matrices b_stride elements apart and the rows of A are sorted by matrix in segments of whole
// 256-row blocks, so a tile of either size lies in one segment; it takes its matrix from blk_expert[m0 / 128] and returns, the
// whole workgroup alike and before any barrier, where that is negative (a block no row was routed to).  Nothing else
// differs: the k order and the arithmetic of an output element are those of the plain tile.  PK selects the form of B: PK_DENSE,
// 16-bit elements.  PK_MXFP4 (with GROUPED: gpt-oss experts kept in MXFP4) reads B packed: g.B holds K / 2 bytes of nibbles a row and g.b_scale K / 32 scale bytes a row, in the rows and
// the strides (b_stride, in elements) of the dense stack.  A thread fetches, where the dense tile fetches 16 bytes of B, the 4
// bytes that hold the same eight elements and their block's scale byte -- a thread's piece never crosses a row's end or a
// block of 32 -- and unpacks them (mxfp4_unpack8) into the uint4 the dense tile would have loaded, on its way into the same LDS
// layout: from the LDS reads on the kernel is the dense one, operand bits and k order included.  The unpacking of tile kt + 1 is
// spread over the last three of tile kt's four MFMA steps, so that its VALU work issues under the matrix pipe and not, with every
// wave of the workgroup at once, between the k loop's last MFMA and the barrier (in the last tile it expands stale registers,
// which nothing reads).  PK_FP8 (without GROUPED: the Llama family's projections kept in block-scaled FP8) does the same with one
// byte an element: g.B holds K e4m3fn codes a row in the rows of the dense matrix, g.b_scale fp32 [rows / 32][K / b_block_k], the
// scale of every 32 stored rows and b_block_k columns (a multiple of CK, so a k tile lies in one block column, and a thread's
// four pieces, RS rows apart, in block rows RS / 32 apart).  A thread fetches the 8 bytes that hold the dense piece's eight
// elements and their block's scale, and fp8_unpack8 makes the dense uint4 of them under the same MFMA steps.
template <int BM, int BN, int WGM, int WGN, int EP, class E = _Float16, bool GROUPED = false, int PK = PK_DENSE>
__device__ __forceinline__ void clm_gemm_tile(const ClmGemm& g) {
  static_assert(PK != PK_MXFP4 || GROUPED, "the MXFP4 B operand is the grouped tile's");
  static_assert(PK != PK_FP8 || !GROUPED, "the FP8 B operand is the plain tile's");
  constexpr bool MX = PK == PK_MXFP4, F8 = PK == PK_FP8;
  using vec8 = typename ClmElem<E>::v8;
  constexpr int T = 64 * WGM * WGN, WTM = BM / WGM, WTN = BN / WGN, FM = WTM / 32, FN = WTN / 32, RS = T / 8;
  static_assert(WTN == 64, "the head epilogue reduces over 64-column wave slices");
  static_assert(BM * 8 == 4 * T && BN * 8 == 4 * T, "four 16-byte loads per operand and thread per k tile");
  static_assert(RS % 32 == 0, "a thread's four pieces of B are whole scale rows of 32 apart");
  extern __shared__ __attribute__((aligned(16))) unsigned char clm_lds[];
  E* As = reinterpret_cast<E*>(clm_lds);
  E* Bs = As + 2 * BM * CPITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave / WGN, wn = wave % WGN;
  const int li = lane & 31, hh = lane >> 5;
  int m0, n0;
  {   // tiles column-major (consecutive tiles share the weight panel), a contiguous range of tiles per XCD
    const int mt = (g.M + BM - 1) / BM, nwg = gridDim.x, b = blockIdx.x, xcd = b & 7, qq = nwg >> 3, rr = nwg & 7;
    const int tile = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (b >> 3);
    m0 = (tile % mt) * BM; n0 = (tile / mt) * BN;
  }
  const int K = g.K, nk = K / CK;
  const E* ag = static_cast<const E*>(g.A) + (long long)(m0 + (tid >> 3)) * K + (tid & 7) * 8;
  const E* bg = static_cast<const E*>(g.B) + (long long)(n0 + (tid >> 3)) * K + (tid & 7) * 8;
  long long boff = (long long)(n0 + (tid >> 3)) * K + (tid & 7) * 8;   // MX: the element bg points at, counted from g.B
  int ex = 0;
  if (GROUPED) {
    ex = g.blk_expert[m0 / 128];   // one value per workgroup: m0 is a multiple of 128
    if (ex < 0) return;
    bg += (long long)ex * g.b_stride;
    boff += (long long)ex * g.b_stride;
  }
  const long long rstep = (long long)RS * K;
  uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
  // MX: element e of B is nibble e & 1 of byte e / 2 and belongs to scale byte e / 32; boff, rstep and k0 are multiples of 8
  const unsigned char* bq = static_cast<const unsigned char*>(g.B);
  const unsigned char* bs = static_cast<const unsigned char*>(g.b_scale);
  unsigned rq0, rq1, rq2, rq3, rs0, rs1, rs2, rs3;
#define CLM_FETCH_MX(rq, rs, e) rq = *reinterpret_cast<const unsigned*>(bq + ((e) >> 1)); rs = bs[(e) >> 5];
  // FP8: element e of B is byte e; the scales of the thread's first piece are row f8s, of piece i the row i * RS / 32 below
  // it, nkb = K / b_block_k to a row; f8kb is the block column of the k tile being fetched, f8in that tile's place in it
  const int nkb = F8 ? K / g.b_block_k : 0, f8tiles = F8 ? g.b_block_k / CK : 1;
  const float* f8s = static_cast<const float*>(g.b_scale) + (long long)((n0 + (tid >> 3)) >> 5) * nkb;
  int f8kb = 0, f8in = 0;
  uint2 rf0, rf1, rf2, rf3;
  float rc0, rc1, rc2, rc3;
#define CLM_FETCH_F8(rf, rc, i, k0) rf = *reinterpret_cast<const uint2*>(bq + boff + (i) * rstep + (k0)); rc = f8s[(i) * (RS / 32) * nkb + f8kb];
  // an empty statement that keeps an unpacked piece where it was computed: without it the compiler moves the unpacking, whose
  // results only the stash reads, behind the k tile's last MFMA
#define CLM_PIN(r) asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
#define CLM_FETCH(k0)                                                                                                   \
  ra0 = *reinterpret_cast<const uint4*>(ag + (k0)); ra1 = *reinterpret_cast<const uint4*>(ag + rstep + (k0));             \
  ra2 = *reinterpret_cast<const uint4*>(ag + 2 * rstep + (k0)); ra3 = *reinterpret_cast<const uint4*>(ag + 3 * rstep + (k0)); \
  if constexpr (MX) {                                                                                                   \
    CLM_FETCH_MX(rq0, rs0, boff + (k0)) CLM_FETCH_MX(rq1, rs1, boff + rstep + (k0))                                     \
    CLM_FETCH_MX(rq2, rs2, boff + 2 * rstep + (k0)) CLM_FETCH_MX(rq3, rs3, boff + 3 * rstep + (k0))                     \
  } else if constexpr (F8) {                                                                                            \
    CLM_FETCH_F8(rf0, rc0, 0, k0) CLM_FETCH_F8(rf1, rc1, 1, k0) CLM_FETCH_F8(rf2, rc2, 2, k0) CLM_FETCH_F8(rf3, rc3, 3, k0) \
  } else {                                                                                                              \
  rb0 = *reinterpret_cast<const uint4*>(bg + (k0)); rb1 = *reinterpret_cast<const uint4*>(bg + rstep + (k0));             \
  rb2 = *reinterpret_cast<const uint4*>(bg + 2 * rstep + (k0)); rb3 = *reinterpret_cast<const uint4*>(bg + 3 * rstep + (k0)); }
#define CLM_STASH(buf)                                                                                                  \
  { E* ad = As + (buf) * BM * CPITCH + (tid >> 3) * CPITCH + (tid & 7) * 8;                                      \
    E* bd = Bs + (buf) * BN * CPITCH + (tid >> 3) * CPITCH + (tid & 7) * 8;                                      \
    *reinterpret_cast<uint4*>(ad) = ra0; *reinterpret_cast<uint4*>(ad + RS * CPITCH) = ra1;                             \
    *reinterpret_cast<uint4*>(ad + 2 * RS * CPITCH) = ra2; *reinterpret_cast<uint4*>(ad + 3 * RS * CPITCH) = ra3;       \
    *reinterpret_cast<uint4*>(bd) = rb0; *reinterpret_cast<uint4*>(bd + RS * CPITCH) = rb1;                             \
    *reinterpret_cast<uint4*>(bd + 2 * RS * CPITCH) = rb2; *reinterpret_cast<uint4*>(bd + 3 * RS * CPITCH) = rb3; }
  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  CLM_FETCH(0)
  if constexpr (MX) {
    rb0 = mxfp4_unpack8<E>(rq0, rs0); rb1 = mxfp4_unpack8<E>(rq1, rs1);
    rb2 = mxfp4_unpack8<E>(rq2, rs2); rb3 = mxfp4_unpack8<E>(rq3, rs3);
  }
  if constexpr (F8) {
    rb0 = fp8_unpack8<E>(rf0, rc0); rb1 = fp8_unpack8<E>(rf1, rc1);
    rb2 = fp8_unpack8<E>(rf2, rc2); rb3 = fp8_unpack8<E>(rf3, rc3);
  }
  CLM_STASH(0)
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if constexpr (F8) {   // the block column of tile kt + 1
      if (++f8in == f8tiles) { f8in = 0; ++f8kb; }
    }
    if (kt + 1 < nk) { CLM_FETCH((kt + 1) * CK) }
    const E* ap = As + cur * BM * CPITCH + (wm * WTM + li) * CPITCH + 8 * hh;
    const E* bp = Bs + cur * BN * CPITCH + (wn * WTN + li) * CPITCH + 8 * hh;
#pragma unroll
    for (int kk = 0; kk < CK; kk += 16) {
      vec8 a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = *reinterpret_cast<const vec8*>(ap + i * 32 * CPITCH + kk);
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = *reinterpret_cast<const vec8*>(bp + j * 32 * CPITCH + kk);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = ClmElem<E>::mfma(a[i], b[j], acc[i][j]);
      if constexpr (MX) {   // the next tile's pieces are expanded between this tile's MFMAs, behind the step that hid their loads
        if (kk == 16) { rb0 = mxfp4_unpack8<E>(rq0, rs0); CLM_PIN(rb0) }
        if (kk == 32) { rb1 = mxfp4_unpack8<E>(rq1, rs1); CLM_PIN(rb1) }
        if (kk == 48) { rb2 = mxfp4_unpack8<E>(rq2, rs2); CLM_PIN(rb2) rb3 = mxfp4_unpack8<E>(rq3, rs3); CLM_PIN(rb3) }
      }
      if constexpr (F8) {   // the same places
        if (kk == 16) { rb0 = fp8_unpack8<E>(rf0, rc0); CLM_PIN(rb0) }
        if (kk == 32) { rb1 = fp8_unpack8<E>(rf1, rc1); CLM_PIN(rb1) }
        if (kk == 48) { rb2 = fp8_unpack8<E>(rf2, rc2); CLM_PIN(rb2) rb3 = fp8_unpack8<E>(rf3, rc3); CLM_PIN(rb3) }
      }
    }
    if (kt + 1 < nk) { CLM_STASH(cur ^ 1) }
    __syncthreads();
  }
#undef CLM_FETCH
#undef CLM_FETCH_MX
#undef CLM_FETCH_F8
#undef CLM_PIN
#undef CLM_STASH
  // epilogue: C/D layout of the 32x32 MFMAs: col = lane & 31, row = (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5)
  const int colw = n0 + wn * WTN;
  const E* bias = static_cast<const E*>(g.bias);
  if (GROUPED && (EP == EP_OSS_GLU || EP == EP_F32_BIAS)) bias += (long long)ex * g.bias_stride;   // the expert's bias
  E* out16 = static_cast<E*>(g.out16);
  if (EP == EP_HEAD || EP == EP_HEAD_CAP) {
    if (colw >= g.N) return;   // a 64-column group entirely beyond the vocabulary (wave-uniform)
    const int cg = colw / 64;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        float v[FN];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          float a = acc[i][j][e];
          if (EP == EP_HEAD_CAP) a = g.cap * (1.0f - 2.0f / (expf(2.0f * (a / g.cap)) + 1.0f));   // cap * tanh(a / cap)
          v[j] = colw + j * 32 + li < g.N ? a : -INFINITY;
          mx = fmaxf(mx, v[j]);
        }
        mx = warp32_max(mx);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < FN; ++j) s += __expf(v[j] - mx);
        s = warp32_sum(s);
        if (row < g.M) {
          if (li == 0) { g.pmax[(long long)row * g.ncg + cg] = mx; g.psum[(long long)row * g.ncg + cg] = s; }
          const int t = g.tgt[row];
#pragma unroll
          for (int j = 0; j < FN; ++j)
            if (colw + j * 32 + li == t) g.tlogit[row] = v[j];
        }
      }
    }
    return;
  }
  if (EP == EP_QKNORM_ROPE) {
    // EP_ROPE without a bias, behind an RMSNorm over each q and k head of a row (Qwen3), all on the fp32 accumulator.  A lane
    // holds columns colw + li and colw + 32 + li as below, so a head of 64 is the wave's slice: the sum of squares is a
    // butterfly over the 32 lanes of a half, which leaves the same bits in every lane.  A head of 128 is the slices of waves
    // `wave & ~1` and `wave | 1` of this workgroup (n0 and the head boundaries are multiples of 128): each writes its
    // per-row partial sums to LDS -- the operand tiles are dead after the k loop's last barrier -- and both add the two in one
    // order, lower 64 columns first, so the result depends neither on the wave nor on the tile.  The barrier is reached by
    // every wave of the workgroup, the v slices and the slices beyond N included: no wave returns before it.
    static_assert(FN == 2 && WGN % 2 == 0, "rotary pairs are the two fragments of a lane; a head of 128 is two neighbouring waves");
    const bool normed = colw < g.rope_cols;   // wave-uniform, and inside the matrix: rope_cols <= N
    float* part = reinterpret_cast<float*>(clm_lds);   // [waves][WTM]
    if (g.hd == 128) {
      if (normed) {
#pragma unroll
        for (int i = 0; i < FM; ++i) {
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const float ss = warp32_sum(__builtin_fmaf(acc[i][0][e], acc[i][0][e], acc[i][1][e] * acc[i][1][e]));
            if (li == 0) part[wave * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh] = ss;
          }
        }
      }
      __syncthreads();
    }
    if (colw >= g.N) return;
    const int c0 = colw + li, c1 = c0 + 32;
    const float sc = colw < g.qcols ? g.qscale : 1.f;
    const int half = g.hd >> 1, hc = colw % g.hd, fi = (hc >> 1) + li;
    const float inv_hd = 1.0f / (float)g.hd;
    float w0 = 1.f, w1 = 1.f;
    if (normed) {   // stored under the head's row order, like the rows they scale
      const E* nw = static_cast<const E*>(colw < g.qcols ? g.qnorm_w : g.knorm_w);
      w0 = (float)nw[hc + li]; w1 = (float)nw[hc + 32 + li];
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int lr = i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh, row = m0 + wm * WTM + lr;
        float x0 = acc[i][0][e], x1 = acc[i][1][e];
        float ss = 0.f;
        if (normed)
          ss = g.hd == 128 ? part[(wave & ~1) * WTM + lr] + part[(wave | 1) * WTM + lr]
                           : warp32_sum(__builtin_fmaf(x0, x0, x1 * x1));
        if (row >= g.M) continue;
        if (normed) {
          const float rstd = 1.0f / sqrtf(ss * inv_hd + g.rms_eps);
          x0 = x0 * rstd * w0; x1 = x1 * rstd * w1;
          const long long a = (long long)g.pos[row] * half + fi;
          const float cs = g.rope_cos[a], sn = g.rope_sin[a];
          const float y0 = x0 * cs - x1 * sn, y1 = x1 * cs + x0 * sn;
          x0 = y0; x1 = y1;
        }
        E* o = out16 + (long long)row * g.ldo;
        o[c0] = (E)(x0 * sc);
        o[c1] = (E)(x1 * sc);
      }
    }
    return;
  }
  if (EP == EP_ROPE || EP == EP_ROPE_PART || EP == EP_SWIGLU || EP == EP_GEGLU || EP == EP_OSS_GLU) {
    // a lane holds columns colw + li (fragment 0) and colw + 32 + li (fragment 1) of every row it owns: the two halves of a
    // rotary pair (head dims of 128 are stored [0..31, 64..95, 32..63, 96..127], and in general stored 32-block 2j holds dims
    // [32j, 32j + 32) and block 2j + 1 dims [hd / 2 + 32j, hd / 2 + 32j + 32), so their pairs are 32 columns apart as
    // well), and the gate and up values of one SwiGLU / GeGLU column (the weight's rows are interleaved in blocks of 32).  N is a
    // multiple of 64 here, so a wave's slice is inside the matrix or outside it as a whole.
    static_assert(FN == 2, "rotary pairs and gate / up pairs are the two fragments of a lane");
    if (colw >= g.N) return;
    const int c0 = colw + li, c1 = c0 + 32;
    if (EP == EP_OSS_GLU) {
      // gpt-oss: the two columns' biases, gate clamped from above and up on both sides, (up + 1) * gate * sigmoid(1.702 gate).
      // expf(-1.702 g) = inf (g far below 0) gives a factor 0 and so g * 0 = -0, never inf / inf.
      const int oc = (colw >> 1) + li;
      const float bg0 = (float)bias[c0], bu0 = (float)bias[c1], lim = g.glu_limit;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (row >= g.M) continue;
          const float gt = fminf(acc[i][0][e] + bg0, lim), up = fminf(fmaxf(acc[i][1][e] + bu0, -lim), lim);
          out16[(long long)row * g.ldo + oc] = (E)((up + 1.0f) * gt * (1.0f / (1.0f + expf(-1.702f * gt))));
        }
      }
      return;
    }
    if (EP == EP_SWIGLU || EP == EP_GEGLU) {
      const int oc = (colw >> 1) + li;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (row >= g.M) continue;
          const float gt = acc[i][0][e], up = acc[i][1][e];
          if (EP == EP_GEGLU) out16[(long long)row * g.ldo + oc] = (E)(gelu_new(gt) * up);
          else out16[(long long)row * g.ldo + oc] = (E)(gt / (1.0f + __expf(-gt)) * up);
        }
      }
      return;
    }
    const float b0 = bias ? (float)bias[c0] : 0.f, b1 = bias ? (float)bias[c1] : 0.f;
    const float sc = colw < g.qcols ? g.qscale : 1.f;
    // EP_ROPE: wave-uniform (q | k | v boundaries are multiples of the head dim).  EP_ROPE_PART (GPT-NeoX's partial rotary):
    // the table has rope_half columns, and of the slice at (colw % hd) / 2 = 32 j of them the lanes below rope_half - 32 j
    // hold a rotary pair; the other lanes' two columns pass through (llm_rescore.neox_head_perm stores the heads so).
    const bool rot = colw < g.rope_cols && (EP != EP_ROPE_PART || ((colw % g.hd) >> 1) + li < g.rope_half);
    const int half = EP == EP_ROPE_PART ? g.rope_half : g.hd >> 1, fi = ((colw % g.hd) >> 1) + li;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (row >= g.M) continue;
        float x0 = acc[i][0][e] + b0, x1 = acc[i][1][e] + b1;
        if (rot) {
          const long long a = (long long)g.pos[row] * half + fi;
          const float cs = g.rope_cos[a], sn = g.rope_sin[a];
          const float y0 = x0 * cs - x1 * sn, y1 = x1 * cs + x0 * sn;
          x0 = y0; x1 = y1;
        }
        E* o = out16 + (long long)row * g.ldo;
        o[c0] = (E)(x0 * sc);
        o[c1] = (E)(x1 * sc);
      }
    }
    return;
  }
  if (EP == EP_F32_BIAS) {
    // gpt-oss: EP_F32 with the (expert's) bias on the accumulator
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = colw + j * 32 + li;
      if (col >= g.N) continue;
      const float bv = (float)bias[col];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (row >= g.M) continue;
          g.resid[(long long)row * g.ldo + col] = acc[i][j][e] + bv;
        }
      }
    }
    return;
  }
  if (EP == EP_F32 || EP == EP_QKV_F32) {
    // OLMo-2: the accumulator itself, unrounded, for a norm over the whole output row in a pass of its own.  EP_QKV_F32 keeps
    // only the q | k columns in fp32 (pitch rope_cols) and rounds the v columns once, where the attention reads them.
    const int pitch = EP == EP_F32 ? g.ldo : g.rope_cols;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = colw + j * 32 + li;
      if (col >= g.N) continue;
      const bool f32 = EP == EP_F32 || col < g.rope_cols;
#pragma unroll
      for (int i = 0; i < FM; ++i) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
          if (row >= g.M) continue;
          if (f32) g.resid[(long long)row * pitch + col] = acc[i][j][e];
          else out16[(long long)row * g.ldo + col] = (E)acc[i][j][e];
        }
      }
    }
    return;
  }
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int col = colw + j * 32 + li;
    if (col >= g.N) continue;
    const float bv = bias ? (float)bias[col] : 0.f;
    const float sc = col < g.qcols ? g.qscale : 1.f;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = m0 + wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (row >= g.M) continue;
        float v = acc[i][j][e] + bv;
        const long long off = (long long)row * g.ldo + col;
        if (EP == EP_RESID) {
          g.resid[off] += v;
        } else {
          if (EP == EP_RELU) v = fmaxf(v, 0.f);
          else if (EP == EP_GELU) v = gelu_new(v);
          else if (EP == EP_GELU_ERF) v = gelu_erf(v);
          else v *= sc;
          out16[off] = (E)v;
        }
      }
    }
  }
}

// The tile as a kernel of its own: the plain GEMM, and the grouped one of the routed experts.
template <int BM, int BN, int WGM, int WGN, int EP, class E = _Float16>
__global__ __launch_bounds__(64 * WGM * WGN) void clm_gemm_kernel(ClmGemm g) {
  clm_gemm_tile<BM, BN, WGM, WGN, EP, E>(g);
}
template <int BM, int BN, int WGM, int WGN, int EP, class E = _Float16>
__global__ __launch_bounds__(64 * WGM * WGN) void clm_gemm_grouped_kernel(ClmGemm g) {
  clm_gemm_tile<BM, BN, WGM, WGN, EP, E, true>(g);
}

// the grouped tile over experts kept in MXFP4 (ClmGemm::b_scale)
template <int BM, int BN, int WGM, int WGN, int EP, class E = _Float16>
__global__ __launch_bounds__(64 * WGM * WGN) void clm_gemm_grouped_mx_kernel(ClmGemm g) {
  clm_gemm_tile<BM, BN, WGM, WGN, EP, E, true, PK_MXFP4>(g);
}

// the plain tile over a matrix kept in block-scaled FP8 (ClmGemm::b_scale, b_block_k)
template <int BM, int BN, int WGM, int WGN, int EP, class E = _Float16>
__global__ __launch_bounds__(64 * WGM * WGN) void clm_gemm_fp8_kernel(ClmGemm g) {
  clm_gemm_tile<BM, BN, WGM, WGN, EP, E, false, PK_FP8>(g);
}

template <int BM, int BN, int WGM, int WGN, int EP, class E, bool GROUPED, int PK = PK_DENSE>
constexpr auto clm_gemm_entry() {
  if constexpr (PK == PK_MXFP4) return &clm_gemm_grouped_mx_kernel<BM, BN, WGM, WGN, EP, E>;
  else if constexpr (PK == PK_FP8) return &clm_gemm_fp8_kernel<BM, BN, WGM, WGN, EP, E>;
  else if constexpr (GROUPED) return &clm_gemm_grouped_kernel<BM, BN, WGM, WGN, EP, E>;
  else return &clm_gemm_kernel<BM, BN, WGM, WGN, EP, E>;
}

constexpr size_t lds_bytes(int bm, int bn) { return (size_t)2 * (bm + bn) * CPITCH * 2; }   // 2-byte elements

// The launch of one GEMM on the tile the rule chose (ClmGemmTiles of clm_internal.h); GROUPED launches the grouped kernel on
// the same grid (M is then the sorted rows S, a multiple of 256), PK the packed form of either.
template <int EP, class E = _Float16, bool GROUPED = false, int PK = PK_DENSE>
int clm_gemm_tiles(const ClmGemm& g, hipStream_t s, bool use256) {
  if (use256) {   // one 8-wave workgroup per CU
    const auto kern = clm_gemm_entry<256, 256, 2, 4, EP, E, GROUPED, PK>();
    const int m256 = (g.M + 255) / 256, n256 = (g.N + 255) / 256;
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(256, 256));
    B2T_REQUIRE(attr == hipSuccess, "b2t_clm_score_f16: %zu bytes of LDS refused", lds_bytes(256, 256));
    hipLaunchKernelGGL(kern, dim3(m256 * n256), dim3(512), lds_bytes(256, 256), s, g);
  } else {
    const auto kern = clm_gemm_entry<128, 128, 2, 2, EP, E, GROUPED, PK>();
    static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes(128, 128));
    B2T_REQUIRE(attr == hipSuccess, "b2t_clm_score_f16: %zu bytes of LDS refused", lds_bytes(128, 128));
    const int m128 = (g.M + 127) / 128, n128 = (g.N + 127) / 128;
    hipLaunchKernelGGL(kern, dim3(m128 * n128), dim3(256), lds_bytes(128, 128), s, g);
  }
  B2T_CHECK_LAUNCH("clm_gemm_kernel");
  return 0;
}

}  // namespace
}  // namespace b2t
