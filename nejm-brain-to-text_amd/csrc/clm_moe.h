// clm_moe.h — the routed-experts MLP of a sparse mixture-of-experts layer (Mixtral; causal_lm_mixtral.hip's header has the
// contract), written once for both element types: the four small kernels around the grouped GEMM, the workspace region, the
// launches of one layer's MLP (moe_mlp) and MixtralFamily, which hands layout, refusals and forward to the entry-point bodies
// and the size rules of clm_internal.h.  A policy P of this forward is LlamaShared<E> (everything the Llama layer launches) plus
//   P::gemm_experts_swiglu, P::gemm_experts_f32 (g, s)   the two grouped GEMMs, each through the one tile rule launch_gemm
//   P::route, P::gather                                   the launches of the two kernels below that depend on E (MoeOps<E>)
//
// The rule of the layout: the host knows every size before the first launch and never reads routing back.  With n = rows * top_k
// routed (row, choice) entries, S = round_up(n, 256) + 256 * n_experts sorted rows always suffice, because every expert's
// segment is padded to whole 256-row blocks (sum over experts of round_up(count, 256) <= n + 255 * n_experts).  The grouped GEMM
// runs over all S rows on either tile; a tile whose 128-row block no expert owns returns at once.
#pragma once
#include <limits.h>

#include "clm_llama.h"

namespace b2t {
namespace {

constexpr int MOE_MAX_EXPERTS = 64, MOE_MAX_TOPK = 8;

// One row: the router's logits l[e] = sum_c x[c] Wg[e][c] (16-bit operands widened, fp32 sums in the order of
// clm_llama_rmsnorm_kernel's statistic: the strided loop and block_sum256, so they depend on the row alone), the choice of k
// experts by repeated argmax with a strict `>` over the experts not yet taken (ties go to the lower index; a comparison with a
// NaN is false, so whatever the logits hold the ids are k distinct values in [0, ne)), and the weights
// w[j] = exp(l[e_j] - l[e_0]) / sum_i exp(l[e_i] - l[e_0]) in fp32, in order of choice.  route_e / route_w: [rows][k];
// route_out (optional): the ids once more, for the caller.
template <class E>
__global__ __launch_bounds__(256) void clm_moe_route_kernel(const E* x, const E* wg, int d, int ne, int k, int* route_e,
                                                            float* route_w, int* route_out) {
  __shared__ float red[4];
  __shared__ float lg[MOE_MAX_EXPERTS];
  __shared__ float we[MOE_MAX_TOPK];
  const int r = blockIdx.x;
  const E* xr = x + (long long)r * d;
  for (int e = 0; e < ne; ++e) {
    const E* w = wg + (long long)e * d;
    float v = 0.f;
    for (int c = threadIdx.x; c < d; c += 256) v += (float)xr[c] * (float)w[c];
    const float l = block_sum256(v, red);
    if (threadIdx.x == 0) lg[e] = l;
  }
  if (threadIdx.x != 0) return;   // thread 0 wrote lg and we and is their only reader
  unsigned long long taken = 0;
  float l0 = 0.f, sum = 0.f;
  for (int j = 0; j < k; ++j) {
    int best = -1;
    for (int e = 0; e < ne; ++e) {
      if ((taken >> e) & 1) continue;
      if (best < 0 || lg[e] > lg[best]) best = e;
    }
    taken |= 1ull << best;          // k <= ne: an expert is left
    if (j == 0) l0 = lg[best];
    const float ex = expf(lg[best] - l0);
    we[j] = ex;
    sum += ex;
    route_e[(long long)r * k + j] = best;
    if (route_out) route_out[(long long)r * k + j] = best;
  }
  for (int j = 0; j < k; ++j) route_w[(long long)r * k + j] = we[j] / sum;
}

// A single workgroup: sorts the n = rows * k entries (entry i = row i / k, choice i % k) by expert, in entry order inside an
// expert, into segments of whole 256-row blocks.  Thread t owns the entries [t * chunk, (t + 1) * chunk); per expert the
// threads count theirs, an exclusive scan over the block gives each thread its first slot, and the segment's start is the sum
// of the segments before it: no atomics, so the slots do not depend on timing.  Writes perm[S] (slot -> source row, -1 for
// padding), slot_of[n] (entry -> slot) and blk_expert[S / 128] (-1 behind the last segment).
__global__ __launch_bounds__(256) void clm_moe_plan_kernel(const int* route_e, int n, int k, int ne, int S, int* perm, int* slot_of,
                                                           int* blk_expert) {
  __shared__ int wsum[4];
  const int t = threadIdx.x, lane = t & 63, chunk = (n + 255) / 256;
  const int i0 = min(t * chunk, n), i1 = min(i0 + chunk, n);
  int base = 0;
  for (int e = 0; e < ne; ++e) {
    int c = 0;
    for (int i = i0; i < i1; ++i) c += route_e[i] == e;
    int inc = c;
    for (int o = 1; o < 64; o <<= 1) {
      const int u = __shfl_up(inc, o);
      if (lane >= o) inc += u;
    }
    __syncthreads();                 // the expert before is done with wsum
    if (lane == 63) wsum[t >> 6] = inc;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < (t >> 6); ++w) before += wsum[w];
    const int total = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]), seg = (total + 255) / 256 * 256;
    int slot = base + before + inc - c;
    for (int i = i0; i < i1; ++i)
      if (route_e[i] == e) {
        slot_of[i] = slot;
        perm[slot++] = i / k;
      }
    for (int p = base + total + t; p < base + seg; p += 256) perm[p] = -1;
    for (int b = base / 128 + t; b < (base + seg) / 128; b += 256) blk_expert[b] = e;
    base += seg;
  }
  for (int p = base + t; p < S; p += 256) perm[p] = -1;
  for (int b = base / 128 + t; b < S / 128; b += 256) blk_expert[b] = -1;
}

// xs[slot] = x[perm[slot]] in 16-byte pieces (d / 8 per row), zeros where perm[slot] < 0: every one of the S sorted rows is
// written, so no tile reads an operand nobody wrote.
template <class E>
__global__ __launch_bounds__(256) void clm_moe_gather_kernel(const E* x, const int* perm, E* xs, int d, long long pieces) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pieces) return;
  const int per = d >> 3;
  const long long slot = i / per;
  const int c = (int)(i % per) * 8, src = perm[slot];
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (src >= 0) v = *reinterpret_cast<const uint4*>(x + (long long)src * d + c);
  *reinterpret_cast<uint4*>(xs + slot * d + c) = v;
}

// resid[r][c] += ((w[0] ys[slot_of[r][0]][c] + w[1] ys[slot_of[r][1]][c]) + ...) in fp32, in order of choice; one thread per
// element, no atomics.
__global__ __launch_bounds__(256) void clm_moe_combine_kernel(const float* ys, const int* slot_of, const float* route_w, int k,
                                                              float* resid, int d, long long elems) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= elems) return;
  const long long r = i / d;
  const int c = (int)(i % d);
  float acc = route_w[r * k] * ys[(long long)slot_of[r * k] * d + c];
  for (int j = 1; j < k; ++j) acc = acc + route_w[r * k + j] * ys[(long long)slot_of[r * k + j] * d + c];
  resid[i] += acc;
}

// the launches that depend on the element type (a policy's route and gather)
template <class El>
struct MoeOps {
  static int route(const El* x, const El* wg, int d, int ne, int k, int* route_e, float* route_w, int* route_out, long long rows,
                   hipStream_t s) {
    hipLaunchKernelGGL(clm_moe_route_kernel<El>, dim3((unsigned)rows), dim3(256), 0, s, x, wg, d, ne, k, route_e, route_w, route_out);
    B2T_CHECK_LAUNCH("clm_moe_route_kernel");
    return 0;
  }
  static int gather(const El* x, const int* perm, El* xs, int d, long long S, hipStream_t s) {
    const long long pieces = S * (d >> 3);
    hipLaunchKernelGGL(clm_moe_gather_kernel<El>, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, x, perm, xs, d, pieces);
    B2T_CHECK_LAUNCH("clm_moe_gather_kernel");
    return 0;
  }
};

// The region behind the Llama layout for a forward over `rows` rows: the route arrays, the plan arrays, and the sorted operand
// xs[S][d], the experts' hidden rows hs[S][F] and outputs ys[S][d] (fp32).  Offsets are from the region's start.
struct MoeRegion {
  long long S;
  size_t route_e, route_w, slot_of, perm, blk_expert, xs, hs, ys, bytes;
};
inline MoeRegion moe_region(const b2t_clm_llama_t* m, const b2t_clm_moe_t* moe, long long rows) {
  MoeRegion R{};
  const long long n = rows * moe->top_k;
  R.S = rup(n, 256) + 256LL * moe->n_experts;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += al256(bytes); return at; };
  R.route_e = take(sizeof(int) * (size_t)n);
  R.route_w = take(sizeof(float) * (size_t)n);
  R.slot_of = take(sizeof(int) * (size_t)n);
  R.perm = take(sizeof(int) * (size_t)R.S);
  R.blk_expert = take(sizeof(int) * (size_t)(R.S / 128));
  R.xs = take(2 * (size_t)R.S * m->d_model);
  R.hs = take(2 * (size_t)R.S * m->ffn_dim);
  R.ys = take(sizeof(float) * (size_t)R.S * m->d_model);
  R.bytes = o;
  return R;
}
inline bool moe_dims_ok(const b2t_clm_moe_t* moe) {
  return moe && moe->n_experts >= 1 && moe->n_experts <= MOE_MAX_EXPERTS && moe->top_k >= 1 && moe->top_k <= MOE_MAX_TOPK &&
         moe->top_k <= moe->n_experts;
}
// The Llama layout plus the region behind its total, as olmo2_layout; a cached call's state goes behind the new total.  The
// dense MLP's hidden rows (hbuf) get no bytes: the experts' hidden rows are hs in the region.
inline ClmLayout mixtral_layout(const b2t_clm_llama_t* m, const b2t_clm_moe_t* moe, long long rows, long long hrows, size_t ints) {
  const long long qw = (long long)(m->n_heads + 2 * m->n_kv_heads) * (m->d_model / m->n_heads);
  ClmLayout L = clm_layout(m->d_model, qw, 0, m->vocab, rows, hrows, ints);
  L.total += moe_region(m, moe, rows).bytes;
  return L;
}

// One layer's MLP over r.rows rows: resid += sum_j w[j] down_{e_j}(silu(x gate_{e_j}) * (x up_{e_j})), x16 the operand.
template <class P>
int moe_mlp(const b2t_clm_llama_t& m, const b2t_clm_moe_t& moe, int l, long long rows, const ClmLayout& L, char* base,
            const typename P::E* x16, float* resid, hipStream_t s) {
  using E = typename P::E;
  const int d = m.d_model, F = m.ffn_dim, ne = moe.n_experts, k = moe.top_k;
  const MoeRegion R = moe_region(&m, &moe, rows);
  B2T_REQUIRE(R.S <= INT_MAX, "b2t_clm_mixtral: %lld sorted rows do not fit an int", R.S);
  char* reg = base + L.total - R.bytes;
  int* route_e = reinterpret_cast<int*>(reg + R.route_e);
  float* route_w = reinterpret_cast<float*>(reg + R.route_w);
  int* slot_of = reinterpret_cast<int*>(reg + R.slot_of);
  int* perm = reinterpret_cast<int*>(reg + R.perm);
  int* blk_expert = reinterpret_cast<int*>(reg + R.blk_expert);
  E* xs = reinterpret_cast<E*>(reg + R.xs);
  E* hs = reinterpret_cast<E*>(reg + R.hs);
  float* ys = reinterpret_cast<float*>(reg + R.ys);
  const b2t_clm_llama_layer_t& w = m.layers_host[l];
  int* route_out = moe.route_out ? moe.route_out + (long long)l * rows * k : nullptr;
  if (int rc = P::route(x16, static_cast<const E*>(moe.router_w_host[l]), d, ne, k, route_e, route_w, route_out, rows, s)) return rc;
  hipLaunchKernelGGL(clm_moe_plan_kernel, dim3(1), dim3(256), 0, s, route_e, (int)(rows * k), k, ne, (int)R.S, perm, slot_of,
                     blk_expert);
  B2T_CHECK_LAUNCH("clm_moe_plan_kernel");
  if (int rc = P::gather(x16, perm, xs, d, R.S, s)) return rc;
  ClmGemm g{};
  g.A = xs; g.B = w.gate_up_w; g.M = (int)R.S; g.N = 2 * F; g.K = d; g.out16 = hs; g.ldo = F;
  g.blk_expert = blk_expert; g.b_stride = moe.gate_up_stride * d;
  if (int rc = P::gemm_experts_swiglu(g, s)) return rc;
  g = ClmGemm{};
  g.A = hs; g.B = w.down_w; g.M = (int)R.S; g.N = d; g.K = F; g.resid = ys; g.ldo = d;
  g.blk_expert = blk_expert; g.b_stride = moe.down_stride * F;
  if (int rc = P::gemm_experts_f32(g, s)) return rc;
  const long long elems = rows * d;
  hipLaunchKernelGGL(clm_moe_combine_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, s, ys, slot_of, route_w, k, resid,
                     d, elems);
  B2T_CHECK_LAUNCH("clm_moe_combine_kernel");
  return 0;
}

// the Llama forward with the routed MLP in the dense one's place
template <class P, class Attn>
int mixtral_forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                    const b2t_clm_moe_t* moe) {
  using E = typename P::E;
  auto mlp = [&](int l, const E* x16, float* resid) { return moe_mlp<P>(m, *moe, l, r.rows, L, base, x16, resid, s); };
  return llama_forward_mlp<P>(m, r, L, base, attn, s, nullptr, mlp);
}

// The MoE descriptor of a checked model for the entry point `who`: refused are a null descriptor, router array or entry,
// expert counts outside the limits, a stride that does not hold a padded matrix (zero included), and q / k / v biases
// (Mixtral has none).
inline int clm_mixtral_check(const char* who, const b2t_clm_llama_t& m, const b2t_clm_moe_t* moe) {
  B2T_REQUIRE(moe, "%s: null moe descriptor", who);
  B2T_REQUIRE(moe->n_experts >= 1 && moe->n_experts <= MOE_MAX_EXPERTS, "%s: n_experts %d outside [1, %d]", who, moe->n_experts,
              MOE_MAX_EXPERTS);
  B2T_REQUIRE(moe->top_k >= 1 && moe->top_k <= MOE_MAX_TOPK && moe->top_k <= moe->n_experts, "%s: top_k %d outside [1, min(%d, n_experts %d)]",
              who, moe->top_k, MOE_MAX_TOPK, moe->n_experts);
  B2T_REQUIRE(moe->gate_up_stride >= rup(2LL * m.ffn_dim, ROWPAD) && moe->down_stride >= rup(m.d_model, ROWPAD),
              "%s: expert strides %lld / %lld rows below round_up(2 ffn_dim, 256) = %lld / round_up(d_model, 256) = %lld", who,
              moe->gate_up_stride, moe->down_stride, rup(2LL * m.ffn_dim, ROWPAD), rup(m.d_model, ROWPAD));
  B2T_REQUIRE(m.n_layers == 0 || moe->router_w_host, "%s: null router_w_host", who);
  for (int l = 0; l < m.n_layers; ++l) {
    B2T_REQUIRE(moe->router_w_host[l], "%s: null router weight in layer %d", who, l);
    B2T_REQUIRE(!m.layers_host[l].qkv_b, "%s: layer %d has q / k / v biases (qkv_b), which Mixtral does not", who, l);
  }
  return 0;
}

// what the entry-point bodies and the size rules of clm_internal.h take from this family
struct MixtralFamily : LlamaFamilyBase {
  static ClmLayout layout(const b2t_clm_llama_t* m, long long rows, long long hrows, size_t ints, const b2t_clm_moe_t* moe) {
    return mixtral_layout(m, moe, rows, hrows, ints);
  }
  static bool dims_ok(const b2t_clm_llama_t* m, const b2t_clm_moe_t* moe) {
    return LlamaFamilyBase::dims_ok(m, moe) && moe_dims_ok(moe);
  }
  template <class P>
  static int check(const char* who, const b2t_clm_llama_t* m, const b2t_clm_moe_t* moe) {
    if (int rc = clm_llama_check_model(m)) return rc;
    return clm_mixtral_check(who, *m, moe);
  }
  template <class P, class Attn>
  static int forward(const b2t_clm_llama_t& m, const ClmRun& r, const ClmLayout& L, char* base, Attn&& attn, hipStream_t s,
                     const b2t_clm_moe_t* moe) {
    return mixtral_forward<P>(m, r, L, base, attn, s, moe);
  }
};

}  // namespace
}  // namespace b2t
