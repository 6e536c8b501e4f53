// wfst_prune.hip -- FinalizeDecoding and PruneActiveTokens of the WFST decoder (see wfst.hip): prune_frame and the one-workgroup
// kernels, the cluster kernels and the walk pieces they share, b2t_wfst_finalize / b2t_wfst_prune.
#include "wfst_internal.h"

namespace b2t {
namespace {
// PruneForwardLinks (:297-374) / PruneForwardLinksFinal (:380-470) for ONE frame f, by one workgroup.
// extra_cost(t) = min over the surviving forward links of t of (extra_cost(dst) + link cost - cost gap), plus, on the last
// frame of a finished utterance, the final-cost term.  The emitting links of f end in frame f + 1, whose values are final:
// ONE pass over them gives each token a base value (and prunes the links beyond lattice_beam).  The epsilon links stay
// inside the frame and form chains a few arcs deep: they are relaxed IN PLACE from above (atomicMin, Bellman-Ford) until
// nothing moves -- a few passes over a few thousand links instead of over all ~25 k links of the frame each time --, and one
// more pass then prunes the epsilon links beyond the beam with the converged values.  (Pruning while the values are still
// upper bounds would remove links that belong in the lattice.)
// keep_all: the frame's tokens are never removed and count with extra cost 0 (the newest frame in PruneActiveTokens).
// Returns through *flags: [0] scratch, [1] |= an extra cost moved by more than delta (vs tok_prev = its old value: the
// reference's extra_costs_changed, which alone sends PruneActiveTokens one frame further back, :528-531), [2] |= a link was pruned.
#ifdef B2T_FIN_TIMING
__device__ unsigned long long fin_t[8];   // [0..4] cycles in: token init, emitting links, epsilon sweeps, epsilon prune, token pass; [5] sweeps; [6] frames
#define FT(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); fin_t[i] += now_ - ft_; ft_ = now_; } } while (0)
#else
#define FT(i) do {} while (0)
#endif
constexpr int PRUNE_LDS_WORDS = 36000;   // dynamic LDS of the finalize / prune kernels (144 000 B of the CU's 160 KB)
// (l, g, o BY VALUE, and the kernels below hold their Lay as a by-value copy: with a reference to the struct the compiler kept
//  all 25 array pointers in scratch memory, reloaded them around every barrier and -- their address space lost on the way
//  through memory -- turned every access into a FLAT instruction, which also waits on the LDS counter)
__device__ __forceinline__ void prune_frame(const Lay l, const Graph g, const Opts o, int f, int F, bool final_frame, int has_final, float final_best,
                            float delta, int* flags, unsigned* lds) {
#ifdef B2T_FIN_TIMING
  unsigned long long ft_ = __builtin_amdgcn_s_memtime();
  if (blockIdx.x == 0 && threadIdx.x == 0) ++fin_t[6];
#endif
  const int a0 = l.tok_off[f], a1 = l.tok_off[f + 1];
  const int e0 = f == 0 ? 0 : l.link_off[2 * f], e1 = l.link_off[2 * f + 1];                 // eps links of frame f
  const int m0 = f < F ? l.link_off[2 * f + 1] : 0, m1 = f < F ? l.link_off[2 * f + 2] : 0;   // emitting f -> f+1
  // The pass is bound by ONE CU's rate of random gathers (64 cache lines per wave instruction): per emitting link the costs of
  // its two tokens, the extra cost of its destination, and an atomic on the extra cost of its source (62 % of finalize's
  // time).  A frame's tokens are contiguous, so the three arrays that are hit at random -- extra costs of frame f (atomics),
  // costs and extra costs of frame f + 1 -- are staged in LDS when they fit (a frame holds ~8 k tokens: 100 KB); the source
  // costs stay in memory (links are created token by token: a wave's sources share a few lines).
  const int b0 = a1, b1 = f < F ? l.tok_off[f + 2] : a1;
  const int nA = a1 - a0, nB = b1 - b0;
  if (lds != nullptr && nA + 2 * nB <= PRUNE_LDS_WORDS) {
    unsigned* xA = lds; unsigned* cB = lds + nA; unsigned* xB = cB + nB;
    // (four tokens per thread and trip, a trip's loads before its stores: tok_prev / tok_extra may alias for all the compiler
    //  knows, so a one-token loop waits out a memory round trip per token)
    for (int tb = a0; tb < a1; tb += 4 * NT) {
      unsigned ex[4]; float base[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = tb + k * NT + (int)threadIdx.x, q = t < a1 ? t : a1 - 1;
        ex[k] = l.tok_extra[q];
        base[k] = INFINITY;
        if (final_frame) {
          const float fc = has_final ? g.final_cost[l.tok_state[q]] : 0.f;
          base[k] = fmaxf(o2f(l.tok_cost[q]) + fc - final_best, 0.f);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = tb + k * NT + (int)threadIdx.x;
        if (t < a1) { l.tok_prev[t] = ex[k]; xA[t - a0] = __float_as_uint(base[k]); }
      }
    }
    for (int tb = b0; tb < b1; tb += 4 * NT) {
      unsigned c4[4], x4[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int t = tb + k * NT + (int)threadIdx.x, q = t < b1 ? t : b1 - 1; c4[k] = l.tok_cost[q]; x4[k] = l.tok_extra[q]; }
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int t = tb + k * NT + (int)threadIdx.x; if (t < b1) { cB[t - b0] = c4[k]; xB[t - b0] = x4[k]; } }
    }
    __syncthreads();
    FT(0);
    // A frame has ~22 k emitting links (up to 54 k).  What bounds the pass on ONE CU is the address path of the vector memory
    // unit: a wave's load instruction costs it 16 clocks whatever its width, and a link read field by field is six of them
    // (measured 1.5 clocks per link = 6 x 16 / 64).  So a thread takes FOUR CONSECUTIVE links: one 16-byte load per field, the
    // four alive bytes as one word, and only the source costs remain single gathers; dead links are marked by rewriting that
    // word once.  A trip is still two dependent round trips (links, then source costs), and the marks may alias anything for
    // all the compiler knows, so three trips are kept in flight by hand: trip i + 2 loads its links, trip i + 1 gathers its
    // source costs, trip i is evaluated (LDS reads, LDS atomics, marks).
    const int mb = m0 & ~3;                                   // quads are 16-byte aligned in every link array
    const int n_trips = (m1 - mb + 4 * NT - 1) / (4 * NT);
    const int q_last = m1 > mb ? (m1 - 1 - mb) / 4 : 0;
    int4 srcA, dstA; float4 acA, grA; unsigned alA;
    int4 srcB, dstB; float4 acB, grB; unsigned alB; unsigned csB[4];
#define B2T_LOAD_A(trip)                                                                                                  \
    {                                                                                                                       \
      int q_ = (trip) * NT + (int)threadIdx.x; if (q_ > q_last) q_ = q_last;                                                \
      const int i_ = mb + 4 * q_;                                                                                           \
      alA = *reinterpret_cast<const unsigned*>(l.link_alive + i_);                                                          \
      srcA = *reinterpret_cast<const int4*>(l.link_src + i_); dstA = *reinterpret_cast<const int4*>(l.link_dst + i_);       \
      acA = *reinterpret_cast<const float4*>(l.link_ac + i_); grA = *reinterpret_cast<const float4*>(l.link_graph + i_);    \
    }
#define B2T_A_TO_B(trip)                                                                                                  \
    {                                                                                                                       \
      alB = alA; srcB = srcA; dstB = dstA; acB = acA; grB = grA;                                                            \
      const int i_ = mb + 4 * ((trip) * NT + (int)threadIdx.x);                                                             \
      const int s_[4] = {srcA.x, srcA.y, srcA.z, srcA.w};                                                                   \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) csB[k] = (i_ + k >= m0 && i_ + k < m1) ? l.tok_cost[s_[k]] : 0u;        \
    }
    if (n_trips > 0) {
      B2T_LOAD_A(0);
      B2T_A_TO_B(0);
      if (n_trips > 1) { B2T_LOAD_A(1); }
    }
    for (int tr = 0; tr < n_trips; ++tr) {
      const int4 srcC = srcB, dstC = dstB; const float4 acC = acB, grC = grB; const unsigned alC = alB;
      unsigned csC[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) csC[k] = csB[k];
      if (tr + 1 < n_trips) { B2T_A_TO_B(tr + 1); }
      if (tr + 2 < n_trips) { B2T_LOAD_A(tr + 2); }
      const int i0 = mb + 4 * (tr * NT + (int)threadIdx.x);
      const int s4[4] = {srcC.x, srcC.y, srcC.z, srcC.w}, d4[4] = {dstC.x, dstC.y, dstC.z, dstC.w};
      const float a4[4] = {acC.x, acC.y, acC.z, acC.w}, g4[4] = {grC.x, grC.y, grC.z, grC.w};
      unsigned al_new = alC;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int li = i0 + k;
        if (li < m0 || li >= m1 || !((alC >> (8 * k)) & 0xffu)) continue;
        const float lec = link_extra_lds(xB, cB, d4[k] - b0, csC[k], a4[k], g4[k]);
        if (lec > o.lattice_beam) { al_new &= ~(0xffu << (8 * k)); continue; }
        atomicMin(&xA[s4[k] - a0], extra_bits(lec));
      }
      // (the word's other bytes, if any, are links of neighbouring segments: finished, or not started before the next barrier)
      if (al_new != alC) { *reinterpret_cast<unsigned*>(l.link_alive + i0) = al_new; flags[2] = 1; }
    }
#undef B2T_LOAD_A
#undef B2T_A_TO_B
    __syncthreads();
    FT(1);
    for (int iter = 0; iter < 4096 && e1 > e0; ++iter) {
      if (threadIdx.x == 0) flags[0] = 0;
      __syncthreads();
      for (int li = e1 - 1 - (int)threadIdx.x; li >= e0; li -= NT) {
        if (!l.link_alive[li]) continue;
        const int src = l.link_src[li], dst = l.link_dst[li];
        const unsigned de = __hip_atomic_load(&xA[dst - a0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const float lec = link_extra_at(l, li, src, dst, __uint_as_float(de));
        if (!(lec <= o.lattice_beam)) continue;
        const unsigned nb = extra_bits(lec);
        if (nb < atomicMin(&xA[src - a0], nb)) flags[0] = 1;
      }
      __syncthreads();
#ifdef B2T_FIN_TIMING
      if (blockIdx.x == 0 && threadIdx.x == 0) ++fin_t[5];
#endif
      if (!flags[0]) break;
      __syncthreads();
    }
    FT(2);
    for (int li = e0 + threadIdx.x; li < e1; li += NT) {
      if (!l.link_alive[li]) continue;
      const int src = l.link_src[li], dst = l.link_dst[li];
      const float lec = link_extra_at(l, li, src, dst, __uint_as_float(xA[dst - a0]));
      if (lec > o.lattice_beam) { l.link_alive[li] = 0; flags[2] = 1; }
    }
    __syncthreads();
    FT(3);
    for (int t = a0 + threadIdx.x; t < a1; t += NT) {
      unsigned nv = xA[t - a0];
      if (final_frame && __uint_as_float(nv) > o.lattice_beam) nv = INF_BITS;
      l.tok_extra[t] = nv;
      const unsigned ov = l.tok_prev[t];
      if (extra_moved(nv, ov, delta)) flags[1] = 1;
    }
    __syncthreads();
    FT(4);
    return;
  }
  for (int t = a0 + threadIdx.x; t < a1; t += NT) {
    float base = INFINITY;
    if (final_frame) {
      const float fc = has_final ? g.final_cost[l.tok_state[t]] : 0.f;
      base = o2f(l.tok_cost[t]) + fc - final_best;
      if (base < 0.f) base = 0.f;
    }
    l.tok_prev[t] = l.tok_extra[t];
    l.tok_extra[t] = __float_as_uint(base);
  }
  __syncthreads();
  FT(0);
  // (4 links per thread and trip, every load of the four issued before the first use: the pass is a chain of dependent
  //  gathers -- link -> its two tokens -> their costs -- and one workgroup has to hide their latency by itself)
  for (int base = m0; base < m1; base += 4 * NT) {
    int li[4], src[4], dst[4]; unsigned char al[4]; float ac[4], gr[4], cs[4], cd[4], xd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      li[k] = base + k * NT + (int)threadIdx.x;
      const int q = li[k] < m1 ? li[k] : m1 - 1;
      al[k] = l.link_alive[q]; src[k] = l.link_src[q]; dst[k] = l.link_dst[q]; ac[k] = l.link_ac[q]; gr[k] = l.link_graph[q];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { cs[k] = o2f(l.tok_cost[src[k]]); cd[k] = o2f(l.tok_cost[dst[k]]); xd[k] = __uint_as_float(l.tok_extra[dst[k]]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (li[k] >= m1 || !al[k]) continue;
      const float lec = link_extra(xd[k], cs[k], ac[k], gr[k], cd[k]);
      if (lec > o.lattice_beam) { l.link_alive[li[k]] = 0; flags[2] = 1; continue; }
      atomicMin(&l.tok_extra[src[k]], extra_bits(lec));
    }
  }
  __syncthreads();
  FT(1);
  // (the relaxation sweeps stay one link per thread and trip: batching four links' loads ahead of their updates doubled the
  //  kernel's time -- a sweep then propagates through fewer links of a chain and more sweeps are needed)
  for (int iter = 0; iter < 4096 && e1 > e0; ++iter) {
    if (threadIdx.x == 0) flags[0] = 0;
    __syncthreads();
    // newest links first: the closure appends the links of deeper tokens later, and extra costs flow from a link's destination
    // to its source, so a sweep in creation order needs one pass per level of the closure and a backward sweep about one in all
    for (int li = e1 - 1 - (int)threadIdx.x; li >= e0; li -= NT) {
      if (!l.link_alive[li]) continue;
      const int src = l.link_src[li], dst = l.link_dst[li];
      const unsigned de = __hip_atomic_load(&l.tok_extra[dst], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      const float lec = link_extra_at(l, li, src, dst, __uint_as_float(de));
      if (!(lec <= o.lattice_beam)) continue;        // cannot survive, and cannot lower anything below the beam
      const unsigned nb = extra_bits(lec);
      if (nb < atomicMin(&l.tok_extra[src], nb)) flags[0] = 1;
    }
    __syncthreads();
#ifdef B2T_FIN_TIMING
    if (blockIdx.x == 0 && threadIdx.x == 0) ++fin_t[5];
#endif
    if (!flags[0]) break;
    __syncthreads();
  }
  FT(2);
  for (int li = e0 + threadIdx.x; li < e1; li += NT) {
    if (!l.link_alive[li]) continue;
    const int src = l.link_src[li], dst = l.link_dst[li];
    const float lec = link_extra_at(l, li, src, dst, __uint_as_float(l.tok_extra[dst]));
    if (lec > o.lattice_beam) { l.link_alive[li] = 0; flags[2] = 1; }
  }
  __syncthreads();
  FT(3);
  for (int t = a0 + threadIdx.x; t < a1; t += NT) {
    unsigned nv = l.tok_extra[t];
    if (final_frame && __uint_as_float(nv) > o.lattice_beam) { nv = INF_BITS; l.tok_extra[t] = nv; }
    const unsigned ov = l.tok_prev[t];
    if (extra_moved(nv, ov, delta)) flags[1] = 1;
  }
  __syncthreads();
  FT(4);
}

// ---- The per-frame walk of the two cluster pruning kernels below: PruneForwardLinks over one frame by the whole cluster, the extra
// costs minima taken with L2 atomics, the other members' values read with L1-bypassing loads.  FIN = FinalizeDecoding's rules: every
// link's alive byte is WRITTEN, exactly once, and never read; otherwise (PruneActiveTokens) dead links are skipped and only deaths
// are written.  The callers place the cluster barriers between the pieces and say where the frame's offsets come from.
// Emitting links [m0, m1) of frame f -> f + 1 (their destinations' extras are final).  into_last: the destinations are the last
// frame's tokens, whose marks (extra = inf beyond the beam) FinalizeDecoding applies on the fly.
template <bool FIN>
__device__ __forceinline__ void cwalk_emitting(const Lay l, int m0, int m1, int gtid, int gthreads, float beam, bool into_last) {
  for (int li = m0 + gtid; li < m1; li += gthreads) {
    if (!FIN && !ldub(&l.link_alive[li])) continue;
    const int src = l.link_src[li], dst = l.link_dst[li];
    float xd = __uint_as_float(ldu(&l.tok_extra[dst]));
    if (into_last && xd > beam) xd = INFINITY;          // (the mark PruneForwardLinksFinal has left on the last frame by now)
    const float lec = link_extra_at(l, li, src, dst, xd);
    if (lec > beam) { l.link_alive[li] = 0; continue; }
    if (FIN) l.link_alive[li] = 1;
    atomicMin(&l.tok_extra[src], extra_bits(lec));
  }
}
// Epsilon links [e0, e1) inside a frame: relaxation sweeps (newest links first, as prune_frame) until nothing moves, one cluster
// barrier per round.  `it` counts the rounds of the whole launch: round `it` reports through cl->changed[it & 7] (a rotating set
// of 'something moved' words in L2, no barrier to reset one).  Returns false when a barrier timed out.
template <bool FIN>
__device__ __forceinline__ bool cwalk_eps_relax(CCtx& c, const Lay l, int e0, int e1, float beam, int& it) {
  Clu* cl = c.cl;
  bool ok = true;
  for (int iter = 0; iter < 4096 && e1 > e0; ++iter) {
    const int w = it & 7;
    if (c.gtid == 0) cl->changed[(it + 1) & 7] = 0;       // (last read seven sweeps ago; the next sweep writes it behind this sweep's barrier)
    int moved = 0;
    // (two relaxation sweeps per meeting: the atomics of one member are in L2 for the others' next loads at once, so values travel
    //  two links further per barrier; a round in which NOBODY lowered anything read only final values: the fixpoint)
    for (int rep = 0; rep < 2; ++rep)
    for (int li = e1 - 1 - c.gtid; li >= e0; li -= c.gthreads) {
      if (!FIN && !ldub(&l.link_alive[li])) continue;
      const int src = l.link_src[li], dst = l.link_dst[li];
      const float lec = link_extra_at(l, li, src, dst, __uint_as_float(ldu(&l.tok_extra[dst])));
      if (!(lec <= beam)) continue;
      const unsigned nb = extra_bits(lec);
      if (nb < atomicMin(&l.tok_extra[src], nb)) moved = 1;
    }
    if (moved) cl->changed[w] = 1;
    ok = cbar(c);
    ++it;
    if (!ok || !ldi(&cl->changed[w])) break;
  }
  return ok;
}
// Epsilon links [q0, q1) of a frame whose sweeps have converged: the ones beyond the beam die.
template <bool FIN>
__device__ __forceinline__ void cwalk_eps_prune(const Lay l, int q0, int q1, int gtid, int gthreads, float beam) {
  for (int li = q0 + gtid; li < q1; li += gthreads) {
    if (!FIN && !ldub(&l.link_alive[li])) continue;
    const int src = l.link_src[li], dst = l.link_dst[li];
    const float lec = link_extra_at(l, li, src, dst, __uint_as_float(ldu(&l.tok_extra[dst])));
    if (FIN) l.link_alive[li] = lec > beam ? 0 : 1;
    else if (lec > beam) l.link_alive[li] = 0;
  }
}

// The header after a PruneActiveTokens pass (one thread): T0 = the first token that could move.
__device__ __forceinline__ void prune_account(const Lay l, int T0, int n_tok, int n_link, int n_tok_new, int n_link_new) {
  if (T0 == 0) l.tok_best[0] = -1;
  Hdr* h = l.h;
  h->peak_tok = max(h->peak_tok, n_tok); h->peak_link = max(h->peak_link, n_link);
  h->removed_tok += n_tok - n_tok_new; h->removed_link += n_link - n_link_new;
  h->n_tok = n_tok_new; h->n_link = n_link_new; h->links_marked = n_link_new; h->n_prunes += 1;
}
}  // namespace

// FinalizeDecoding (:632-647): PruneForwardLinksFinal on the last frame, then PruneForwardLinks(delta = 0) +
// PruneTokensForFrame backwards.  Marks link_alive; tok_extra = inf for tokens that leave the lattice.
__global__ __launch_bounds__(NT) void wfst_finalize_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                            int max_tok, int max_link, int hash) {
  __shared__ float redf[NT / 64];
  extern __shared__ unsigned prune_lds[];          // PRUNE_LDS_WORDS words (prune_frame's staging area)
  const int u = blockIdx.x;
  Lay l;
  layout(state + (size_t)u * state_bytes, max_frames, max_tok, max_link, hash, &l);
  const int F = l.h->n_frames;
  // ComputeFinalCosts (:547-590)
  const int t0 = l.tok_off[F], t1 = l.tok_off[F + 1];
  float b = INFINITY, bf = INFINITY;
  for (int t = t0 + threadIdx.x; t < t1; t += NT) {
    const float cst = o2f(l.tok_cost[t]);
    b = fminf(b, cst); bf = fminf(bf, cst + g.final_cost[l.tok_state[t]]);
  }
  b = block_min(redf, b); bf = block_min(redf, bf);
  const int has_final = bf != INFINITY;
  const float final_best = has_final ? bf : b;
  if (threadIdx.x == 0) { l.h->final_best = final_best; l.h->has_final = has_final; l.h->finalized = 1; }
  for (int li = threadIdx.x; li < min(l.h->n_link, max_link); li += NT) l.link_alive[li] = 1;
  __syncthreads();
  __shared__ int flags[3];
  for (int f = F; f >= 0; --f) prune_frame(l, g, o, f, F, f == F, has_final, final_best, 0.f, flags, prune_lds);
#ifdef B2T_FIN_TIMING
  if (blockIdx.x == 0 && threadIdx.x == 0)
    printf("finalize (utterance 0, 100 MHz ticks): tokens-init %llu, emitting %llu, eps sweeps %llu (%llu sweeps), eps prune %llu, tokens %llu, frames %llu\n",
           fin_t[0], fin_t[1], fin_t[2], fin_t[5], fin_t[3], fin_t[4], fin_t[6]);
#endif
}

// FinalizeDecoding by the utterance's CLUSTER (round 5; verdict item 4): the G workgroups that searched the utterance, behind one
// XCD's L2, instead of one workgroup on one of 256 CUs (5.7 ms for 32 utterances of 111 frames, a third of a pipelined batch).
// The same fixpoints as prune_frame -- extra costs are minima, a link lives iff its converged link-extra-cost is within the
// lattice beam -- so link_alive / tok_extra equal the single-workgroup kernel's bit for bit (tested).  What changes is where the
// minima are taken (L2 atomics on tok_extra instead of LDS) and how often the members meet: tokens of ALL frames are initialised
// up front (FinalizeDecoding walks every frame), then per frame ONE cluster barrier behind the emitting links f -> f + 1 (the
// epsilon links of frame f + 1 are pruned in the same phase: their extras have converged) and one per epsilon sweep of frame f
// (a rotating set of 'something moved' words in L2, no barrier to reset one).  Every link's alive byte is written exactly once.
// The final frame's tokens beyond the beam are marked (extra = inf) at the very end; the one phase that must see the marks
// (the emitting links F - 1 -> F) applies the rule on the fly, the phases that must not (epsilon sweeps / prune of frame F) run
// before anything is marked -- the order of PruneForwardLinksFinal (:380-470).
__global__ __launch_bounds__(NT) void wfst_finalize_cluster_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                                    int max_tok, int max_link, int hash, int G, int U) {
  __shared__ float redf[NT / 64];
  __shared__ int lsh[8];
  CCtx c = cluster_ctx(g, o, state, state_bytes, max_frames, max_tok, max_link, hash, G, U, lsh);   // (the search's mapping: the members of an utterance share one XCD)
  if (c.u >= U) return;
  __syncthreads();
  const Lay l = c.l;          // a copy, not a reference: see prune_frame
  Clu* cl = c.cl;
  Hdr* h = l.h;
  const int F = h->n_frames;
  const float beam = o.lattice_beam;
  // ComputeFinalCosts (:547-590): every member reduces the whole last frame itself (a few thousand tokens: cheaper than a barrier)
  const int tF0 = l.tok_off[F], tF1 = min(l.tok_off[F + 1], max_tok);
  float bb = INFINITY, bf = INFINITY;
  for (int t = tF0 + (int)threadIdx.x; t < tF1; t += NT) {
    const float cst = o2f(l.tok_cost[t]);
    bb = fminf(bb, cst); bf = fminf(bf, cst + g.final_cost[l.tok_state[t]]);
  }
  bb = block_min(redf, bb); bf = block_min(redf, bf);
  const int has_final = bf != INFINITY;
  const float final_best = has_final ? bf : bb;
  if (c.gtid == 0) {
    cl->overflow = h->overflow;
    for (int k = 0; k < 8; ++k) cl->changed[k] = 0;
  }
  // extra costs of every frame's tokens: inf, the last frame's from the final costs
  for (int t = c.gtid; t < tF1; t += c.gthreads) {
    unsigned v = INF_BITS;
    if (t >= tF0) {
      const float fc = has_final ? g.final_cost[l.tok_state[t]] : 0.f;
      v = __float_as_uint(fmaxf(o2f(l.tok_cost[t]) + fc - final_best, 0.f));
    }
    l.tok_extra[t] = v;
  }
  bool ok = cbar(c);
  int it = 0;                  // epsilon sweeps so far (all frames): sweep `it` reports through cl->changed[it & 7]
  for (int f = F; f >= 0 && ok; --f) {
    // ---- emitting links f -> f + 1 (their destinations' extras are final) ...
    if (f < F) {
      cwalk_emitting<true>(l, l.link_off[2 * f + 1], min(l.link_off[2 * f + 2], max_link), c.gtid, c.gthreads, beam, f + 1 == F);
      // ... and the epsilon links of frame f + 1, whose sweeps have converged: pruned against the (unmarked) extras
      cwalk_eps_prune<true>(l, l.link_off[2 * (f + 1)], min(l.link_off[2 * (f + 1) + 1], max_link), c.gtid, c.gthreads, beam);
      ok = cbar(c);
      if (!ok) break;
    }
    // ---- epsilon links inside frame f
    ok = cwalk_eps_relax<true>(c, l, f == 0 ? 0 : l.link_off[2 * f], min(l.link_off[2 * f + 1], max_link), beam, it);
  }
  if (ok) {
    // epsilon links of frame 0, then the marks on the last frame (nothing reads its extras any more)
    cwalk_eps_prune<true>(l, 0, min(l.link_off[1], max_link), c.gtid, c.gthreads, beam);
    ok = cbar(c);                // (frame 0 may BE the last frame: its prune reads the unmarked extras)
    if (ok)
      for (int t = tF0 + c.gtid; t < tF1; t += c.gthreads)
        if (__uint_as_float(ldu(&l.tok_extra[t])) > beam) l.tok_extra[t] = INF_BITS;
  }
  __syncthreads();
  if (c.gtid == 0) {
    h->final_best = final_best; h->has_final = has_final; h->finalized = 1;
    cluster_leave(c, h);
  }
}

// PruneActiveTokens (lattice-faster-decoder.cc:516-545, called every prune_interval frames at :592-630) as a pass of its own
// between two search calls: PruneForwardLinks (:297-374) on the frames F-1 .. 0 -- the tokens of the newest frame F are
// never pruned and count with extra_cost 0 --, going back only as far as something still changes, then PruneTokensForFrame
// (:489-514) as a stable in-place COMPACTION of the token and link arrays (the reference frees list nodes; here the arrays
// of the state block shrink, so a streamed utterance holds its pruned lattice plus at most prune_interval raw frames).
// Extra costs computed against the best path SO FAR are lower bounds of the final ones, so this removes only what
// FinalizeDecoding would remove: the final lattice is the same with or without these passes (tested).
__global__ __launch_bounds__(NT) void wfst_prune_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                         int max_tok, int max_link, int hash, float delta, float min_fill) {
  extern __shared__ unsigned prune_lds[];          // PRUNE_LDS_WORDS words (prune_frame's staging area)
  const int u = blockIdx.x;
  Lay l0;
  layout(state + (size_t)u * state_bytes, max_frames, max_tok, max_link, hash, &l0);
  const Lay l = l0;         // a copy, not a reference: see prune_frame
  const int F = l.h->n_frames;
  if (F < 2 || l.h->overflow || l.h->finalized) return;
  // memory-pressure policy (min_fill > 0): the pass only exists to bound memory, so an utterance whose arrays are still
  // mostly empty skips it (min_fill = 0: every call prunes, the reference's fixed prune_interval)
  if ((float)l.h->n_tok < min_fill * (float)max_tok && (float)l.h->n_link < min_fill * (float)max_link) return;
  const int n_tok = min(l.h->n_tok, max_tok), n_link = min(l.h->n_link, max_link);
  for (int li = l.h->links_marked + (int)threadIdx.x; li < n_link; li += NT) l.link_alive[li] = 1;
  __syncthreads();
  // ---- PruneForwardLinks, frames F-1 .. 0, stopping at the first frame where nothing moved by more than delta
  __shared__ int flags[3];
#ifdef B2T_WFST_TIMING
  unsigned long long tp0 = __builtin_amdgcn_s_memtime(), tp1, tp2, tp3, tp4;
#endif
  int f_stop = -1;
  for (int f = F - 1; f >= 0; --f) {
    __syncthreads();
    if (threadIdx.x == 0) flags[1] = 0;
    __syncthreads();
    prune_frame(l, g, o, f, F, false, 0, 0.f, delta, flags, prune_lds);
    if (!flags[1]) { f_stop = f; break; }
  }
  // ---- compaction of the tokens of frames f_stop+1 .. F-1 and of every link that starts in frame f_stop or later.
  // Stable and in place, one array SEGMENT at a time (a frame's tokens; a frame's epsilon links; its emitting links), each in
  // chunks of 4 x NT elements: 4 flags per thread, ONE barrier per chunk (scan4).  The first
  // version scanned NT elements per chunk with four barriers and a serial boundary loop: 18 ms per pass, mostly barriers.
#ifdef B2T_WFST_TIMING
  tp1 = __builtin_amdgcn_s_memtime();
#endif
  const int T0 = l.tok_off[f_stop + 1];
  const int TF = l.tok_off[F];                      // tokens of the newest frame always stay
  // (epsilon links of the stop frame that were pruned just now stay behind as dead entries -- link_alive 0 --: the stop frame's
  //  tokens keep their ids and their backpointers into that range; FinalizeDecoding prunes them again)
  const int L0 = f_stop >= 0 ? l.link_off[2 * f_stop + 1] : 0;
  int* excl = reinterpret_cast<int*>(l.tok_prev);   // [t] = new id of token t (or -1)
  __shared__ int wtot[2][4][NT / 64];
  int flip = 0;
  auto tok_alive = [&](int t) { return t >= TF || l.tok_extra[t] != INF_BITS; };
  // pass 1: new token ids frame by frame; tok_off rewritten as the frames are finished
  int run_t = T0;
  {
    int seg0 = T0;
    for (int fb = f_stop + 1; fb <= F; ++fb) {
      const int seg1 = min(l.tok_off[fb + 1], n_tok);       // (old value: rewritten below, after everyone has read it)
      for (int base = seg0; base < seg1; base += 4 * NT) {
        int fl[4], pos[4], tot;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int t = base + k * NT + (int)threadIdx.x; fl[k] = t < seg1 ? (int)tok_alive(t) : 0; }
        scan4(wtot, flip, fl, pos, tot);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int t = base + k * NT + (int)threadIdx.x; if (t < seg1) excl[t] = fl[k] ? run_t + pos[k] : -1; }
        run_t += tot;
      }
      __syncthreads();
      if (threadIdx.x == 0) l.tok_off[fb + 1] = run_t;
      seg0 = seg1;
    }
  }
  const int n_tok_new = run_t;
  __syncthreads();
#ifdef B2T_WFST_TIMING
  tp2 = __builtin_amdgcn_s_memtime();
#endif
  // pass 2: links -- drop, remap, move; link_off rewritten segment by segment
  int run_l = L0;
  {
    int seg0 = L0;
    for (int jb = (f_stop >= 0 ? 2 * f_stop + 1 : 0); jb <= 2 * F; ++jb) {
      const int seg1 = min(l.link_off[jb + 1], n_link);
      for (int base = seg0; base < seg1; base += 4 * NT) {
        int fl[4], pos[4], tot, src[4], dst[4], arc[4]; float ac[4], gr[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int li = base + k * NT + (int)threadIdx.x;
          fl[k] = 0;
          if (li < seg1) {
            src[k] = l.link_src[li]; dst[k] = l.link_dst[li]; arc[k] = l.link_arc[li]; ac[k] = l.link_ac[li]; gr[k] = l.link_graph[li];
            if (l.link_alive[li]) {
              if (src[k] >= T0) src[k] = excl[src[k]];
              if (dst[k] >= T0) dst[k] = excl[dst[k]];
              fl[k] = src[k] >= 0 && dst[k] >= 0;
            }
          }
        }
        scan4(wtot, flip, fl, pos, tot);                               // (its barrier: every read of this chunk is done)
#pragma unroll
        for (int k = 0; k < 4; ++k) if (fl[k]) {
          const int q = run_l + pos[k];                    // q <= li
          l.link_src[q] = src[k]; l.link_dst[q] = dst[k]; l.link_arc[q] = arc[k]; l.link_ac[q] = ac[k]; l.link_graph[q] = gr[k]; l.link_alive[q] = 1;
        }
        run_l += tot;
      }
      __syncthreads();
      if (threadIdx.x == 0) l.link_off[jb + 1] = run_l;
      seg0 = seg1;
    }
  }
  const int n_link_new = run_l;
  __syncthreads();
#ifdef B2T_WFST_TIMING
  tp3 = __builtin_amdgcn_s_memtime();
#endif
  // pass 3: move the surviving tokens (ids only go down; a chunk's reads are done before its writes)
  for (int base = T0; base < n_tok; base += 4 * NT) {
    int k2[4], st[4]; unsigned cs[4], ex[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int t = base + k * NT + (int)threadIdx.x;
      k2[k] = -1;
      if (t < n_tok) { k2[k] = excl[t]; st[k] = l.tok_state[t]; cs[k] = l.tok_cost[t]; ex[k] = l.tok_extra[t]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k2[k] >= 0) { l.tok_state[k2[k]] = st[k]; l.tok_cost[k2[k]] = cs[k]; l.tok_extra[k2[k]] = ex[k]; l.tok_best[k2[k]] = BEST_UNSET; }
    __syncthreads();
  }
  // backpointers of the moved tokens: the first surviving link whose cost equals the token's (best_links' rule)
  for (int li = L0 + (int)threadIdx.x; li < n_link_new; li += NT) {
    const int src = l.link_src[li], dst = l.link_dst[li];
    if (dst >= T0) best_link<false>(l, li, src, dst);
  }
  __syncthreads();
#ifdef B2T_WFST_TIMING
  tp4 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0 && u == 0) printf("wfst prune u0: F %d f_stop %d | sweeps %llu | tok ids %llu | links %llu | tok move + best %llu | tokens %d -> %d, links %d -> %d\n",
                                         F, f_stop, tp1 - tp0, tp2 - tp1, tp3 - tp2, tp4 - tp3, n_tok, n_tok_new, n_link, n_link_new);
#endif
  if (threadIdx.x == 0) prune_account(l, T0, n_tok, n_link, n_tok_new, n_link_new);
}

// PruneActiveTokens by the utterance's CLUSTER (round 5; verdict item 4).  The one-workgroup pass above takes 3.9 ms for 32 utterances
// (more than the 25 frames of search between two passes): ~30 frames of prune_frame on one CU, then a stable compaction that meets
// at a barrier every 4096 elements.  Here the G workgroups that search the utterance share the pass:
//   * PruneForwardLinks per frame as in wfst_finalize_cluster_kernel (L2 atomics on the extra costs), with the pass's own rules:
//     a frame's tokens are re-initialised when its turn comes (the walk stops at the first frame where nothing moved by more than
//     delta), so per frame: emitting links | barrier | epsilon sweeps (one barrier each) | epsilon prune + the 'moved' test +
//     the NEXT frame's initialisation | barrier.  The speculative initialisation of frame f_stop - 1 is undone when the walk stops.
//   * the compaction meets once per 8 x 4096 elements: every member scans its 4096-element share, publishes one total, and after the
//     barrier knows its base; tokens get their new ids from per-member prefix counts (one barrier for the whole range).
// Same surviving set, same order, same ids as the one-workgroup pass (tested array by array on the same state).
// Scratch: the epsilon work list (rebuilt by every frame of the search) for flags and totals; old frame offsets in LDS.
__global__ __launch_bounds__(NT) void wfst_prune_cluster_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                                 int max_tok, int max_link, int hash, float delta, float min_fill, int G, int U) {
  __shared__ int lsh[8], wtot[2][4][NT / 64], tots[80];     // tots[0 .. G]: token bases; tots[40 .. 40 + G]: a link chunk's bases
  extern __shared__ int old_off[];                 // [max_frames + 3] tok_off, then [2 (max_frames + 3)] link_off, as the pass found them
  CCtx c = cluster_ctx(g, o, state, state_bytes, max_frames, max_tok, max_link, hash, G, U, lsh);
  if (c.u >= U) return;
  const int j = c.j;
  __syncthreads();
  const Lay l = c.l;
  Clu* cl = c.cl;
  Hdr* h = l.h;
  const int F = h->n_frames;
  // (every member reads the same header, written by the previous launch: the same decision, before any barrier)
  if (F < 2 || h->overflow || h->finalized) return;
  if ((float)h->n_tok < min_fill * (float)max_tok && (float)h->n_link < min_fill * (float)max_link) return;
  const float beam = o.lattice_beam;
  const int n_tok = min(h->n_tok, max_tok), n_link = min(h->n_link, max_link);
  int* scr = l.wlg;                                  // [0, 8): 'moved' per frame (mod 8); [64 + 32 (chunk mod 8) + member]: chunk totals; [512 + member]: token totals
  int* tok_off_old = old_off;
  int* link_off_old = old_off + (max_frames + 3);
  for (int i = threadIdx.x; i <= F + 1; i += NT) tok_off_old[i] = l.tok_off[i];
  for (int i = threadIdx.x; i <= 2 * F + 2; i += NT) link_off_old[i] = l.link_off[i];
  if (c.gtid == 0) {
    cl->overflow = h->overflow;
    for (int k = 0; k < 8; ++k) { cl->changed[k] = 0; scr[k] = 0; }
  }
  for (int li = h->links_marked + c.gtid; li < n_link; li += c.gthreads) l.link_alive[li] = 1;
  auto init_frame = [&](int f) {                     // tok_prev = the old extra cost, extra = inf (prune_frame's first pass)
    const int a0 = tok_off_old[f], a1 = tok_off_old[f + 1];
    for (int t = a0 + c.gtid; t < a1; t += c.gthreads) { l.tok_prev[t] = ldu(&l.tok_extra[t]); l.tok_extra[t] = INF_BITS; }
  };
  __syncthreads();
  init_frame(F - 1);
  bool ok = cbar(c);
  int it = 0, f_stop = -1;
  for (int f = F - 1; f >= 0 && ok; --f) {
    const int a0 = tok_off_old[f], a1 = tok_off_old[f + 1];
    cwalk_emitting<false>(l, link_off_old[2 * f + 1], min(link_off_old[2 * f + 2], max_link), c.gtid, c.gthreads, beam, false);
    ok = cbar(c);
    if (!ok) break;
    const int e0 = f == 0 ? 0 : link_off_old[2 * f], e1 = min(link_off_old[2 * f + 1], max_link);
    ok = cwalk_eps_relax<false>(c, l, e0, e1, beam, it);
    if (!ok) break;
    // epsilon links beyond the beam; did an extra cost of this frame move by more than delta?; the next frame's initialisation
    cwalk_eps_prune<false>(l, e0, e1, c.gtid, c.gthreads, beam);
    {
      int mv = 0;
      for (int t = a0 + c.gtid; t < a1; t += c.gthreads) {
        const unsigned nv = ldu(&l.tok_extra[t]), ov = ldu(&l.tok_prev[t]);
        if (extra_moved(nv, ov, delta)) mv = 1;
      }
      if (mv) scr[f & 7] = 1;
      if (c.gtid == 0) scr[(f + 6) & 7] = 0;           // the word of frame f - 2 (last read two frames ago, by frame f + 6's test)
    }
    if (f > 0) init_frame(f - 1);
    ok = cbar(c);
    if (!ok) break;
    if (!ldi(&scr[f & 7])) { f_stop = f; break; }
  }
  if (ok && f_stop > 0) {                              // the walk stopped: frame f_stop - 1 keeps its old extra costs
    const int a0 = tok_off_old[f_stop - 1], a1 = tok_off_old[f_stop];
    for (int t = a0 + c.gtid; t < a1; t += c.gthreads) l.tok_extra[t] = ldu(&l.tok_prev[t]);
  }
  // ---- compaction: tokens of frames f_stop + 1 .. F - 1 (the newest frame's always stay), links from frame f_stop's emitting ones on
  const int T0 = tok_off_old[f_stop + 1], TF = tok_off_old[F];
  const int L0 = f_stop >= 0 ? link_off_old[2 * f_stop + 1] : 0;
  int* excl = reinterpret_cast<int*>(l.tok_prev);      // alive: number of survivors before t in its member's block; dead: the complement of that
  int flip = 0;
  // tokens: member j scans the j-th of G equal blocks of [T0, n_tok)
  const int ntok_span = n_tok - T0;
  const int tblk = max(4, ((ntok_span + G - 1) / G + 3) & ~3);
  int n_tok_new = T0;
  if (ok) {
    ok = cbar(c);                                      // the undo's loads of tok_prev are done everywhere before tok_prev becomes excl; the last marks are in L2
  }
  if (ok) {
    const int tb0 = T0 + j * tblk, tb1 = min(tb0 + tblk, n_tok);
    int run = 0;
    for (int base = tb0; base < tb1; base += 4 * NT) {
      int fl[4], pos[4], tot;
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int t = base + k * NT + (int)threadIdx.x; fl[k] = t < tb1 ? (int)(t >= TF || ldu(&l.tok_extra[t]) != INF_BITS) : 0; }
      scan4(wtot, flip, fl, pos, tot);
#pragma unroll
      for (int k = 0; k < 4; ++k) { const int t = base + k * NT + (int)threadIdx.x; if (t < tb1) excl[t] = fl[k] ? run + pos[k] : ~(run + pos[k]); }
      run += tot;
    }
    if (threadIdx.x == 0) scr[512 + j] = run;
    ok = cbar(c);
  }
  if (ok) {
    if ((int)threadIdx.x <= G) {                       // tots[m] = survivors in the blocks before member m; tots[G] = all
      int sum = 0;
      for (int m = 0; m < (int)threadIdx.x; ++m) sum += ldi(&scr[512 + m]);
      tots[threadIdx.x] = sum;
    }
    __syncthreads();
    n_tok_new = T0 + tots[G];
  }
  auto count_before = [&](int p) {                     // survivors in [T0, p)
    if (p >= n_tok) return tots[G];
    const int v = ldi(&excl[p]);
    return tots[(p - T0) / tblk] + (v < 0 ? ~v : v);
  };
  auto new_id = [&](int t) {                           // t >= T0: its id after the pass, or -1
    const int v = ldi(&excl[t]);
    return v < 0 ? -1 : T0 + tots[(t - T0) / tblk] + v;
  };
  if (ok) {
    for (int fb = f_stop + 1 + c.gtid; fb <= F; fb += c.gthreads) l.tok_off[fb + 1] = T0 + count_before(min(tok_off_old[fb + 1], n_tok));
  }
  // links: chunks of G x 4 NT over [L0, n_link), member j takes the j-th 4 NT of a chunk; ONE barrier per chunk.  The segment offsets
  // (a frame's epsilon links, its emitting links) come out on the way: link_off[jb + 1] = L0 + survivors before its old value p, which
  // the thread holding element p knows once the members' totals are in (the first version walked segment by segment: a barrier per
  // segment, ~60 of the pass's ~75 compaction barriers)
  int run_l = L0, cc = 0;
  if (ok) {
    int jb = f_stop >= 0 ? 2 * f_stop + 1 : 0;         // the next segment end to place (offsets are sorted)
    for (int cb = L0; cb < n_link && ok; cb += G * 4 * NT, ++cc) {
      const int base = cb + j * 4 * NT;
      int fl[4], pos[4], tot, src[4], dst[4], arc[4]; float ac[4], gr[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int li = base + k * NT + (int)threadIdx.x;
        fl[k] = 0;
        if (li < n_link) {
          src[k] = l.link_src[li]; dst[k] = l.link_dst[li]; arc[k] = l.link_arc[li]; ac[k] = l.link_ac[li]; gr[k] = l.link_graph[li];
          if (ldub(&l.link_alive[li])) {
            if (src[k] >= T0) src[k] = new_id(src[k]);
            if (dst[k] >= T0) dst[k] = new_id(dst[k]);
            fl[k] = src[k] >= 0 && dst[k] >= 0;
          }
        }
      }
      scan4(wtot, flip, fl, pos, tot);
      if (threadIdx.x == 0) scr[64 + 32 * (cc & 7) + j] = tot;
      ok = cbar(c);                                    // every read of this chunk is done, every member's total is out
      if (!ok) break;
      if ((int)threadIdx.x <= G) {
        int sum = 0;
        for (int m = 0; m < (int)threadIdx.x; ++m) sum += ldi(&scr[64 + 32 * (cc & 7) + m]);
        tots[40 + threadIdx.x] = sum;                  // (tots[0 .. G] keep the token bases)
      }
      __syncthreads();
      const int mybase = run_l + tots[40 + j];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (fl[k]) {
        const int q = mybase + pos[k];                 // q <= li
        l.link_src[q] = src[k]; l.link_dst[q] = dst[k]; l.link_arc[q] = arc[k]; l.link_ac[q] = ac[k]; l.link_graph[q] = gr[k]; l.link_alive[q] = 1;
      }
      // segment ends inside this chunk
      const int cend = cb + G * 4 * NT;
      while (jb <= 2 * F && link_off_old[jb + 1] < cend && link_off_old[jb + 1] < n_link) {
        const int p = link_off_old[jb + 1], e = p - base;          // (p >= cb: the ends are sorted and the earlier ones are placed)
        if (e >= 0 && e < 4 * NT && (e & (NT - 1)) == (int)threadIdx.x) {
          const int k = e / NT;
          l.link_off[jb + 1] = mybase + (k == 0 ? pos[0] : k == 1 ? pos[1] : k == 2 ? pos[2] : pos[3]);
        }
        ++jb;
      }
      run_l += tots[40 + G];
      __syncthreads();                                 // tots[40 ..] are rewritten by the next chunk
    }
    if (ok) for (int q = jb + c.gtid; q <= 2 * F; q += c.gthreads) l.link_off[q + 1] = run_l;      // ends at (or clamped to) the last link
  }
  const int n_link_new = run_l;
  // tokens move down: chunks of G x 4 NT, reads and writes of a chunk separated by a barrier (ids only go down)
  if (ok) {
    for (int cb = T0; cb < n_tok && ok; cb += G * 4 * NT) {
      const int base = cb + j * 4 * NT;
      int k2[4], st[4]; unsigned cs[4], ex[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int t = base + k * NT + (int)threadIdx.x;
        k2[k] = -1;
        if (t < n_tok) { k2[k] = new_id(t); st[k] = l.tok_state[t]; cs[k] = l.tok_cost[t]; ex[k] = ldu(&l.tok_extra[t]); }
      }
      ok = cbar(c);
      if (!ok) break;
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k2[k] >= 0) { l.tok_state[k2[k]] = st[k]; l.tok_cost[k2[k]] = cs[k]; l.tok_extra[k2[k]] = ex[k]; l.tok_best[k2[k]] = BEST_UNSET; }
    }
  }
  if (ok) ok = cbar(c);
  if (ok) {
    // backpointers of the moved tokens: the first surviving link whose cost equals the token's (best_links' rule)
    for (int li = L0 + c.gtid; li < n_link_new; li += c.gthreads) {
      const int src = ldi(&l.link_src[li]), dst = ldi(&l.link_dst[li]);
      if (dst >= T0) best_link<true>(l, li, src, dst);
    }
  }
  __syncthreads();
  if (c.gtid == 0) {
    if (ok) prune_account(l, T0, n_tok, n_link, n_tok_new, n_link_new);
    cluster_leave(c, h);
  }
}

}  // namespace b2t

using namespace b2t;

extern "C" int b2t_wfst_finalize(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, int U, void* stream) {
  { int rc = check_args(g, o, state, U, "wfst_finalize"); if (rc) return rc; }
  const size_t sb = state_bytes(o);
  {   // the utterance's cluster finalizes where the cluster searched (B2T_WFST_FIN_CLUSTER=0, read per call: one workgroup per utterance)
    const char* e = getenv("B2T_WFST_FIN_CLUSTER");
    const int G = (e && atoi(e) == 0) ? 1 : b2t_wfst_cluster_size(U);
    // (cluster kernels spin on L2 barriers: the launch must be fully resident.  b2t_wfst_cluster_size sizes clusters for ONE cluster
    //  kernel on the device at a time -- search, prune and finalize launches of decode streams that run concurrently must be
    //  serialised by the caller (WfstSearch does: one stream per searcher, passes behind the search) or take B2T_WFST_*_CLUSTER=0;
    //  a partly resident launch ends in CBAR_SPIN_LIMIT with overflow | 32, never in a hang)
    B2T_REQUIRE(G <= 32, "wfst_finalize: clusters of at most 32 workgroups (scratch layout), got %d", G);
    if (G > 1) {
      const int grid = cluster_grid(U, G);
      hipLaunchKernelGGL(wfst_finalize_cluster_kernel, dim3(grid), dim3(NT), 0, as_stream(stream), to_graph(g), (char*)state, sb, to_opts(o),
                         o->max_frames, o->max_tokens, o->max_links, o->hash_size, G, U);
      B2T_CHECK_LAUNCH("b2t_wfst_finalize (cluster)");
      return 0;
    }
  }
  allow_lds(wfst_finalize_kernel, PRUNE_LDS_WORDS * sizeof(unsigned));
  hipLaunchKernelGGL(wfst_finalize_kernel, dim3(U), dim3(NT), PRUNE_LDS_WORDS * sizeof(unsigned), as_stream(stream), to_graph(g), (char*)state,
                     sb, to_opts(o), o->max_frames, o->max_tokens, o->max_links, o->hash_size);
  B2T_CHECK_LAUNCH("b2t_wfst_finalize");
  return 0;
}

extern "C" int b2t_wfst_prune(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, int U, float delta, float min_fill,
                              void* stream) {
  { int rc = check_args(g, o, state, U, "wfst_prune"); if (rc) return rc; }
  B2T_REQUIRE(delta >= 0.f && min_fill >= 0.f && min_fill <= 1.f, "wfst_prune: bad delta / min_fill");
  const size_t sb = state_bytes(o);
  {   // the utterance's cluster prunes where the cluster searches (B2T_WFST_PRUNE_CLUSTER=0, read per call: one workgroup per utterance)
    const char* e = getenv("B2T_WFST_PRUNE_CLUSTER");
    const int G = (e && atoi(e) == 0) ? 1 : b2t_wfst_cluster_size(U);
    const size_t lds = (size_t)3 * (o->max_frames + 3) * sizeof(int);
    B2T_REQUIRE(G <= 32, "wfst_prune: clusters of at most 32 workgroups (tots[80] / scratch layout), got %d", G);
    static_assert(WLG_CAP >= 64 + 32 * 8 + 32, "the cluster compaction's per-member scratch lives in the work list");
    if (G > 1 && lds <= 96 * 1024) {
      const int grid = cluster_grid(U, G);
      allow_lds(wfst_prune_cluster_kernel, lds);
      hipLaunchKernelGGL(wfst_prune_cluster_kernel, dim3(grid), dim3(NT), lds, as_stream(stream), to_graph(g), (char*)state, sb, to_opts(o),
                         o->max_frames, o->max_tokens, o->max_links, o->hash_size, delta, min_fill, G, U);
      B2T_CHECK_LAUNCH("b2t_wfst_prune (cluster)");
      return 0;
    }
  }
  allow_lds(wfst_prune_kernel, PRUNE_LDS_WORDS * sizeof(unsigned));
  hipLaunchKernelGGL(wfst_prune_kernel, dim3(U), dim3(NT), PRUNE_LDS_WORDS * sizeof(unsigned), as_stream(stream), to_graph(g), (char*)state, sb,
                     to_opts(o), o->max_frames, o->max_tokens, o->max_links, o->hash_size, delta, min_fill);
  B2T_CHECK_LAUNCH("b2t_wfst_prune");
  return 0;
}
