// wfst_cluster.hip -- the cluster searcher of the WFST decoder (see wfst.hip for the algorithm and the one-workgroup searcher).
// =====================================================================================================================
// CLUSTER search: G workgroups (G = 2, 4 or 8) per utterance instead of one, so that 32 utterances use the whole chip
// instead of 32 of its 256 CUs.  The G workgroups of an utterance are placed on ONE XCD (block b runs on XCD b % 8; checked
// at run time through XCC_ID), i.e. behind one L2:
//   * the frame's token hash, the tokens, the links and a handful of counters live in the utterance's state block and are
//     shared through that L2: plain stores (write-through the CU's vector cache into L2), L2 atomics (hash CAS, cost
//     atomicMin, counters) and L1-bypassing sc1 loads for everything another workgroup may have written;
//   * a frame is a sequence of phases separated by CLUSTER barriers (a monotonic arrival counter in L2, one lane per
//     workgroup arrives and polls) -- 6 per frame, + 4 when max_active binds -- instead of the ~45 workgroup barriers of the
//     single-workgroup kernel: claim and relax are ONE phase (the claim's winner publishes the token id AFTER the token's
//     fields have reached L2; a loser polls the slot), the epsilon work list is appended to by whoever creates a token, the
//     frame's best cost is kept by atomicMin while costs are written, two hashes alternate so that clearing one hides
//     under pass A, and the backpointer pass of a frame runs inside pass A of the next.
// Same arithmetic and the same results as wfst_search_kernel (tests/test_gpu_wfst.py runs both against the oracle).
// =====================================================================================================================
#include "wfst_internal.h"

namespace b2t {
namespace {

#ifndef B2T_CHASE_DEPTH
#define B2T_CHASE_DEPTH 4     // (-DB2T_CHASE_DEPTH=1 builds a library whose closure overflows all the time: the fallback rounds under test)
#endif
constexpr int CHASE_DEPTH = B2T_CHASE_DEPTH;    // tokens a thread of the epsilon closure may have pending (lowered, arcs not yet relaxed)

#ifdef B2T_WFST_TIMING
#define CT(i) { if (c.gtid == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); c.tacc[i] += now_ - c.tprev; c.tprev = now_; } }
#else
#define CT(i)
#endif

// k-th smallest cost of the tokens [t0, t1): the radix select of kth_cost with the histogram of a round summed over the
// cluster in L2 (every member then picks the digit from the same 256 numbers): one cluster barrier per round.
__device__ float ckth_cost(CCtx& c, int t0, int t1, int k, int set, bool& ok) {
  int* hist = c.redi + 64;
  int* res = c.redi + 320;
  unsigned prefix = 0u;
  int rank = k;
  for (int round = 0; round < 4; ++round) {
    radix_count<true>(hist, c.l.tok_cost, t0 + c.j * NT, t1, c.gthreads, round, prefix);
    if (threadIdx.x < 256 && hist[threadIdx.x]) atomicAdd(&c.cl->hist[set][round][threadIdx.x], hist[threadIdx.x]);
    if (!cbar(c)) { ok = false; return 0.f; }
    radix_pick<true>(res, rank, c.cl->hist[set][round]);
    prefix |= (unsigned)res[0] << (24 - 8 * round);
    rank = res[1];
    __syncthreads();
  }
  return o2f(prefix);
}

// The claim's winner creates the token: its fields, its place in the epsilon work list if its state has epsilon arcs, and -- before
// the caller publishes the id -- all of that in L2.  Returns the id, or -1 when the token capacity is exhausted.
__device__ __forceinline__ int cnew_token(CCtx& c, int state) {
  int id = wave_alloc(&c.cl->n_tok);
  if (id < c.max_tok) {
    c.l.tok_state[id] = state; c.l.tok_cost[id] = UMAX; c.l.tok_best[id] = BEST_UNSET; c.l.tok_extra[id] = 0u;
    if (c.g.n_eps[state] > 0) {
      const int w = wave_alloc(&c.cl->wl_n);
      if (w < WLG_CAP) c.l.wlg[w] = id; else atomicOr(&c.cl->overflow, 16);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  } else {
    atomicOr(&c.cl->overflow, 1); id = -1;
  }
  return id;
}

// FindOrAddToken across the cluster: returns the token id of `state` in the frame being built (-1: hash or token capacity
// exhausted).  A hash slot is ONE 8-byte word {state, token id} (the two int arrays of the layout are contiguous), so the
// common case -- the token exists -- is a single L1-bypassing 8-byte load.  The CAS (on the state half) winner allocates the
// token, writes its fields, waits until they are in L2 and only then publishes the id in the other half; everyone else polls
// the word.  A new token whose state has epsilon arcs joins the work list.
template <bool ST>   // ST: frame-stamped slots (compile-time: both claim paths in one kernel spilled 536 B per lane to scratch, 13.6 -> 21.7 ms)
__device__ __forceinline__ int cclaim(CCtx& c, int state) {
  const int mask = c.hash - 1;
  unsigned s = hash_of(state, mask);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(c.key);
  if constexpr (ST) {
    const unsigned want = (c.stamp << 27) | (unsigned)state;
    for (int probe = 0; probe < c.hash; ++probe, s = (s + 1) & mask) {
      unsigned long long v = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        const unsigned k = (unsigned)(v & 0xffffffffull);
        if ((k >> 27) != c.stamp) {               // not of this frame: empty.  ONE 64-bit CAS takes the slot and unsets the stale id with it
          const unsigned long long mine = ((unsigned long long)(unsigned)UNSET << 32) | want;
          const unsigned long long seen = atomicCAS(&slots[s], v, mine);   // (the value-returning form: taking &v for the builtin's `expected` put the loop's state into scratch memory, 13.6 -> 21.7 ms)
          const bool won = seen == v;
          v = seen;
          if (won) {
            const int id = cnew_token(c, state);
            __hip_atomic_store(reinterpret_cast<int*>(&slots[s]) + 1, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return id;
          }
          continue;                                 // lost the race: v holds what is there now, look at it again
        }
        if (k == want) {
          int id = (int)(unsigned)(v >> 32), spins = 0;
          while (id == UNSET) {
            if (++spins > (1 << 24)) { atomicOr(&c.cl->overflow, 32); return -1; }
            id = (int)(unsigned)(__hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
          }
          return id;
        }
        break;                                      // another state of this frame: next slot
      }
    }
    atomicOr(&c.cl->overflow, 4);
    return -1;
  }
  for (int probe = 0; probe < c.hash; ++probe, s = (s + 1) & mask) {
    unsigned long long v = __hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int k = (int)(unsigned)(v & 0xffffffffull);
    if (k == -1) {
      int* kp = reinterpret_cast<int*>(&slots[s]);
      int expected = -1;
      if (__hip_atomic_compare_exchange_strong(kp, &expected, state, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        const int id = cnew_token(c, state);
        __hip_atomic_store(kp + 1, id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return id;
      }
      k = expected;
      v = ((unsigned long long)(unsigned)UNSET << 32) | (unsigned)k;
    }
    if (k == state) {
      int id = (int)(unsigned)(v >> 32), spins = 0;
      while (id == UNSET) {
        if (++spins > (1 << 24)) { atomicOr(&c.cl->overflow, 32); return -1; }
        id = (int)(unsigned)(__hip_atomic_load(&slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32);
      }
      return id;
    }
  }
  atomicOr(&c.cl->overflow, 4);
  return -1;
}

// best_links over the links [l0, l1) (deferred: runs in pass A of the next frame / at the end of the launch)
__device__ __forceinline__ void cbest_links(CCtx& c, int l0, int l1) {
  for (int li = l0 + c.gtid; li < l1; li += c.gthreads) best_link<true>(c.l, li, ldi(&c.l.link_src[li]), ldi(&c.l.link_dst[li]));
}

struct CFrame { int f, t0, t1, pl0, pl1; };   // decoded frames so far, tokens of the newest frame, links awaiting best_links

// One AdvanceDecoding(.., 1) by the whole cluster.  fr is cluster-uniform private state, updated on success.
template <bool ST, bool CP>
__device__ bool cadvance(CCtx& c, CFrame& fr) {
  const Graph& g = c.g;
  Clu* cl = c.cl;
  const int f = fr.f, t0 = fr.t0, t1 = fr.t1, par = f & 1, npar = par ^ 1;
  if (f >= c.max_frames) { if (c.gtid == 0) atomicOr(&cl->overflow, 8); return cbar(c) && false; }
  CT(0)
  // ---- GetCutoff (:650-720): the frame's best cost was kept by atomicMin while the costs were written
  const float best = o2f(ldu(&cl->best[par]));
  const int n = t1 - t0;
  const float beam_cutoff = best + c.o.beam;
  float cur_cutoff = beam_cutoff, adaptive = c.o.beam;
  {
    bool ok = true;
    float max_cut = INFINITY, min_cut = INFINITY;
    if (n > c.o.max_active) { max_cut = ckth_cost(c, t0, t1, c.o.max_active, 0, ok); if (!ok) return false; }
    if (max_cut < beam_cutoff) {
      cur_cutoff = max_cut; adaptive = max_cut - best + c.o.beam_delta;
    } else {
      if (n > c.o.min_active) {
        if (c.o.min_active == 0) min_cut = best;
        else { min_cut = ckth_cost(c, t0, t1, c.o.min_active, 1, ok); if (!ok) return false; }
      }
      if (min_cut > beam_cutoff) { cur_cutoff = min_cut; adaptive = min_cut - best + c.o.beam_delta; }
    }
  }
  CT(1)   // cutoff (k-th cost)
  const float cost_offset = -best;
  const float lp = c.o.length_penalty;
  auto arc_cost = [&](float cur, int s, int a, float& ac, float& gc) {
    ac = cost_offset - c.ll[g_il_t<CP>(g, a) - 1];
    gc = g_w_t<CP>(g, a);
    if (lp != 0.f && g.next[a] != s) gc += lp;
    return cur + ac + gc;
  };
  const int lane = threadIdx.x & 63;
  int narcs = 0;
  // Work distribution.  Out-degrees are bimodal: ~3 arcs inside a word, hundreds at the word-boundary states of L o G, and
  // the word-boundary tokens sit together at the end of a frame's token range (the epsilon closure creates them last).
  //   light tokens (<= HEAVY_DEG arcs): 64-token blocks dealt round-robin over ALL waves of the cluster (block q -> member
  //     q % G), arcs flattened inside the wave as in the single-workgroup kernel;
  //   heavy tokens: pass A's light walk lists them CHUNK by chunk (64 arcs, up to 16 chunks; longer rows get wider chunks),
  //     then one wave per chunk, round-robin: a 400-arc token is seven waves' work, not seven trips of one wave while its
  //     neighbours idle (~66 heavy tokens per frame for 128 waves).
  // (With the blocks dealt member by member the members that got the frame's last blocks took 3-4x as long as the others.)
  const int gwave = (int)(threadIdx.x >> 6) * c.G + c.j, nwaves = c.G * (NT / 64);
  auto walk_light = [&](bool collect, auto&& visit) {
    for (int base = t0 + gwave * 64; base < t1; base += nwaves * 64) {    // wave-uniform
      const int t = base + lane;
      float cur = INFINITY; int s = 0, a0 = 0, deg = 0;
      if (t < t1) {
        cur = o2f(ldu(&c.l.tok_cost[t]));
        if (cur <= cur_cutoff) { s = ldi(&c.l.tok_state[t]); a0 = g.row[s] + g.n_eps[s]; deg = g.row[s + 1] - a0; }
      }
      narcs += deg;
      int nch = 0, sh = 0;
      if (deg > HEAVY_DEG) {
        if (collect) {                             // chunks of 64 << sh arcs, at most 16 per token
          while (((deg - 1) >> (6 + sh)) >= 16) ++sh;
          nch = ((deg - 1) >> (6 + sh)) + 1;
        }
        deg = 0;
      }
      if (collect && __ballot(nch > 0)) {          // wave-uniform: one counter atomic per wave for all its chunks
        int ci = nch;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(ci, off, 64); if (lane >= off) ci += v; }
        const int ctot = __shfl(ci, 63, 64);
        int cb = 0;
        if (lane == 0) cb = atomicAdd(&cl->n_heavy, ctot);
        cb = __shfl(cb, 0, 64) + ci - nch;
        // (an entry carries everything a walk needs -- the token's cost is final by now --: the walks below go from the entry
        //  straight to the arcs, two dependent round trips fewer than through tok_cost / tok_state / row)
        const int hspan = 64 << sh, ha0 = a0, hdeg = g.row[s + 1] - a0;
        for (int k = 0; k < nch; ++k) {
          if (cb + k < HEAVY_CAP) {
            const int ab = ha0 + k * hspan, ae = ha0 + min(hdeg, (k + 1) * hspan);
            c.l.heavy[2 * (cb + k)] = ((unsigned long long)__float_as_uint(cur) << 32) | (unsigned)t;
            c.l.heavy[2 * (cb + k) + 1] = ((unsigned long long)(unsigned)ae << 32) | (unsigned)ab;
          } else {
            atomicOr(&cl->overflow, 16);           // (128 k chunks in one frame: capacity error; every entry below the cap is written)
          }
        }
      }
      int incl = deg;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
      const int total = __shfl(incl, 63, 64), excl = incl - deg;
      for (int jb = 0; jb < total; jb += 64) {
        const int jj = jb + lane;
        int owner = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) { const int v = __shfl(incl, owner + step - 1, 64); if (v <= jj) owner += step; }
        owner = min(owner, 63);
        const int oa0 = __shfl(a0, owner, 64), oex = __shfl(excl, owner, 64), os = __shfl(s, owner, 64);
        const float ocur = __shfl(cur, owner, 64);
        if (jj < total) visit(base + owner, ocur, os, oa0 + (jj - oex));
      }
    }
  };
  auto walk_heavy = [&](auto&& visit) {
    const int nh = min(ldi(&cl->n_heavy), HEAVY_CAP);
#ifdef B2T_WFST_TIMING
    if (c.gtid == 0) { c.tacc[12] += nh; c.tacc[13] += 1; }
#endif
    for (int i = gwave; i < nh; i += nwaves) {
      const unsigned long long e0 = __hip_atomic_load(&c.l.heavy[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const unsigned long long e1 = __hip_atomic_load(&c.l.heavy[2 * i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int t = (int)(unsigned)(e0 & 0xffffffffull), ab = (int)(unsigned)(e1 & 0xffffffffull), ae = (int)(unsigned)(e1 >> 32);
      const float cur = __uint_as_float((unsigned)(e0 >> 32));
      const int s = lp != 0.f ? ldi(&c.l.tok_state[t]) : -1;      // (only the length penalty looks at the source state)
      for (int jb = ab; jb < ae; jb += 64) if (jb + lane < ae) visit(t, cur, s, jb + lane);
    }
  };
  // ---- pass A: the frame's cheapest candidate.  Under it: the previous frame's backpointers, the other hash cleared,
  //      the next parity's accumulators and the histograms reset.
  float mn = INFINITY;
  auto visit_a = [&](int, float cur, int s, int a) { float ac, gc; mn = fminf(mn, arc_cost(cur, s, a, ac, gc)); };
  walk_light(true, visit_a);
  CT(11)  // pass A, light tokens
  if (!cbar(c)) return false;                    // the heavy list is complete
  walk_heavy(visit_a);
  mn = block_min(c.redf, mn);
  narcs = block_sum(c.redi, narcs);
  if (threadIdx.x == 0) { atomicMin(&cl->cand_min[par], f2o(mn)); atomicAdd(&cl->narcs[par], narcs); }
  CT(2)   // pass A walk
  cbest_links(c, fr.pl0, fr.pl1);
  CT(3)   // deferred best links
  int* nkey = npar ? c.l.gkey2 : c.l.gkey;        // (key / idx arrays are adjacent: 8-byte slots)
  const unsigned use = (unsigned)(f + 1) >> 1;     // how often this hash has been used before (frame f + 1 is built in hash (f + 1) & 1)
  c.stamp = 1u + use % 30u;
  if (!ST || (c.stamp == 1u && use > 0u)) {   // stamped: only when the stamps wrap; InitDecoding left both hashes empty
    unsigned long long* ns = reinterpret_cast<unsigned long long*>(nkey);
    const unsigned long long empty = ((unsigned long long)(unsigned)UNSET << 32) | 0xffffffffull;
    for (int i = c.gtid; i < c.hash; i += c.gthreads) ns[i] = empty;
  }
  if (c.j == 0) {
    int* hz = &cl->hist[0][0][0];
    for (int i = threadIdx.x; i < 2 * 4 * 256; i += NT) hz[i] = 0;
    if (threadIdx.x < 8) cl->changed[threadIdx.x] = 0;
    if (threadIdx.x == 0) { cl->best[npar] = UMAX; cl->wl_n = 0; }
  }
  CT(4)   // clears
  if (!cbar(c)) return false;
  CT(5)   // barrier A
  c.key = nkey;
  const unsigned cmin = ldu(&cl->cand_min[par]);
  const float next_cutoff = (cmin == UMAX ? INFINITY : o2f(cmin)) + adaptive;
  const int n0 = ldi(&cl->n_tok), l0 = ldi(&cl->n_link);
  if (c.gtid == 0) {
    const unsigned na = (unsigned)ldi(&cl->narcs[par]);
    const unsigned lo = c.l.h->arcs_lo + na;
    if (lo < c.l.h->arcs_lo) c.l.h->arcs_hi += 1u;
    c.l.h->arcs_lo = lo;
  }
  // ---- pass B: claim + relax + link record in one walk
  auto visit_b = [&](int t, float cur, int s, int a) {
    float ac, gc;
    const float tot = arc_cost(cur, s, a, ac, gc);
    if (!(tot < next_cutoff)) return;
    const int id = cclaim<ST>(c, g.next[a]);
    if (id < 0) return;
    const unsigned nb = f2o(tot);
    atomicMin(&c.l.tok_cost[id], nb);
    const int li = wave_alloc(&cl->n_link);
    if (li < c.max_link) {
      c.l.link_src[li] = t; c.l.link_dst[li] = id; c.l.link_arc[li] = a; c.l.link_ac[li] = ac; c.l.link_graph[li] = gc;
    } else {
      atomicOr(&cl->overflow, 2);
    }
  };
  walk_light(false, visit_b);
  walk_heavy(visit_b);
  if (c.gtid == 0) { cl->cand_min[npar] = UMAX; cl->narcs[npar] = 0; }   // (read above by everyone, not needed before frame f + 1's pass A)
  CT(6)   // pass B walk
  if (!cbar(c)) return false;
  CT(7)   // barrier B
  const int lem = min(ldi(&cl->n_link), c.max_link);
  // ---- ProcessNonemitting.  One pass over the work list in which whoever LOWERS a token's cost goes on to relax that token's
  //      epsilon arcs itself, with the value it wrote (a small per-thread stack in LDS): every final cost was written by a
  //      thread that then relaxed the token's arcs with exactly that cost, so the pass ends at the fixed point and needs no
  //      second sweep to notice it -- one cluster barrier instead of one per level of the epsilon chains plus one (4-5 rounds
  //      of ~10 us each before).  Only a stack overflow (CHASE_DEPTH pending tokens in one thread) asks for another round.
  for (int round = 0;; ++round) {
    const int wn = min(ldi(&cl->wl_n), WLG_CAP);
    if (round > 0 && ldi(&cl->changed[(round - 1) & 7]) == 0) break;
    if (c.gtid == 0) cl->changed[(round + 2) & 7] = 0;
    for (int i = c.gtid; i < wn; i += c.gthreads) {
      // (the stack holds STATES and the costs written for them: relaxing a token's arcs needs nothing else, so a chased token
      //  costs no load of its own -- a level of the chain is row -> arc -> {hash slot, n_eps of the target} -> cost atomic)
      int sp = 1, pops = 0;
      {
        const int t = ldi(&c.l.wlg[i]);
        const unsigned c0 = ldu(&c.l.tok_cost[t]);
        c.stk_t[threadIdx.x] = ldi(&c.l.tok_state[t]);
        c.stk_c[threadIdx.x] = o2f(c0);
      }
      while (sp > 0) {
        if (++pops > (1 << 14)) { atomicOr(&cl->overflow, 32); break; }   // (an epsilon cycle of negative weight: refuse, do not hang)
        --sp;
        const int s = c.stk_t[sp * NT + threadIdx.x];
        const float cur = c.stk_c[sp * NT + threadIdx.x];
        if (!(cur < next_cutoff)) continue;
        const int a0 = g.row[s], ne = g.n_eps[s];
        for (int a = a0; a < a0 + ne; ++a) {
          const float tot = cur + g_w_t<CP>(g, a);
          if (tot < next_cutoff) {
            const int ns = g.next[a];
            const int nne = g.n_eps[ns];           // (in flight next to the claim's slot load)
            const int id = cclaim<ST>(c, ns);
            if (id < 0) continue;
            const unsigned nb = f2o(tot);
            const unsigned old = atomicMin(&c.l.tok_cost[id], nb);
            if (nb < old && nne > 0) {
              if (sp < CHASE_DEPTH) { c.stk_t[sp * NT + threadIdx.x] = ns; c.stk_c[sp * NT + threadIdx.x] = tot; ++sp; }
              else __hip_atomic_store(&cl->changed[round & 7], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
        }
      }
    }
    if (!cbar(c)) return false;
    if (round > 4096) { atomicOr(&cl->overflow, 32); break; }
  }
  CT(8)   // closure rounds incl. their barriers
  // ---- the epsilon links with the converged costs, and the new frame's best cost
  {
    const int wn = min(ldi(&cl->wl_n), WLG_CAP);
    for (int i = c.gtid; i < wn; i += c.gthreads) {
      const int t = ldi(&c.l.wlg[i]);
      const int s = ldi(&c.l.tok_state[t]);
      const float cur = o2f(ldu(&c.l.tok_cost[t]));
      if (!(cur < next_cutoff)) continue;
      const int a0 = g.row[s], ne = g.n_eps[s];
      for (int a = a0; a < a0 + ne; ++a) {
        const float tot = cur + g_w_t<CP>(g, a);
        if (tot < next_cutoff) {
          const int id = cclaim<ST>(c, g.next[a]);      // exists: the closure has converged
          if (id < 0) continue;
          const int li = wave_alloc(&cl->n_link);
          if (li < c.max_link) {
            c.l.link_src[li] = t; c.l.link_dst[li] = id; c.l.link_arc[li] = a; c.l.link_ac[li] = 0.f; c.l.link_graph[li] = g_w_t<CP>(g, a);
          } else {
            atomicOr(&cl->overflow, 2);
          }
        }
      }
    }
    if (c.gtid == 0) cl->n_heavy = 0;            // (last read in pass B; next written in the next frame's pass A)
    float b2 = INFINITY;
    const int n1 = min(ldi(&cl->n_tok), c.max_tok);
    for (int t = n0 + c.gtid; t < n1; t += c.gthreads) b2 = fminf(b2, o2f(ldu(&c.l.tok_cost[t])));
    b2 = block_min(c.redf, b2);
    if (threadIdx.x == 0 && b2 != INFINITY) atomicMin(&cl->best[npar], f2o(b2));
  }
  CT(9)   // epsilon links + best
  if (!cbar(c)) return false;
  CT(10)  // barrier end
  const int n1 = min(ldi(&cl->n_tok), c.max_tok), l1 = min(ldi(&cl->n_link), c.max_link);
  if (c.gtid == 0) {
    c.l.cost_offset[f] = cost_offset;
    c.l.link_off[2 * f + 2] = lem;
    c.l.tok_off[f + 2] = n1;
    c.l.link_off[2 * f + 3] = l1;
  }
  fr.f = f + 1; fr.t0 = n0; fr.t1 = n1; fr.pl0 = l0; fr.pl1 = l1;
  return true;
}

}  // namespace

template <bool ST, bool CP>
__global__ __launch_bounds__(NT) void wfst_cluster_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                           int max_tok, int max_link, int hash, int G, int U,
                                                           const float* __restrict__ logp, const int* __restrict__ lens, int T, int C) {
  __shared__ float ll[MAX_C], lastp[MAX_C], redf[NT];
  __shared__ int redi[NT], lsh[8], stk_t[CHASE_DEPTH * NT];
  __shared__ float stk_c[CHASE_DEPTH * NT];
  CCtx c = cluster_ctx(g, o, state, state_bytes, max_frames, max_tok, max_link, hash, G, U, lsh);
  if (c.u >= U) return;
  const int u = c.u, j = c.j;
  c.ll = ll; c.redf = redf; c.redi = redi; c.stk_t = stk_t; c.stk_c = stk_c;
  if ((int)threadIdx.x < MAX_C) lastp[threadIdx.x] = c.l.last_prob[threadIdx.x];   // every member keeps its own copy of the remembered blank frame
  __syncthreads();
  Clu* cl = c.cl;
  Hdr* h = c.l.h;
  // launch prologue: counters from the header, placement check, the newest frame's best cost
  int nf = h->n_frames, num_input = h->num_input, is_last_blank = h->is_last_blank, last_best = h->last_best;
  if (c.gtid == 0) { cl->n_tok = h->n_tok; cl->n_link = h->n_link; cl->overflow = h->overflow; cl->best[nf & 1] = UMAX; cl->cand_min[nf & 1] = UMAX; cl->narcs[nf & 1] = 0; cl->n_heavy = 0; }
  if (threadIdx.x == 0) cl->xcc[j] = (int)xcc_of();
  if (!cbar(c)) return;
  {
    int same = 1;
    for (int m = 1; m < G; ++m) same &= (ldi(&cl->xcc[m]) == ldi(&cl->xcc[0]));
    if (!same) {                               // not behind one L2: plain stores + sc1 loads would not be coherent
      if (c.gtid == 0) { h->overflow |= 64; cl->bar_base = c.bar_target; }
      return;
    }
  }
  CFrame fr;
  fr.f = nf; fr.t0 = c.l.tok_off[nf]; fr.t1 = c.l.tok_off[nf + 1];
  fr.pl0 = fr.pl1 = 0;
  {
    float b0 = INFINITY;
    for (int t = fr.t0 + c.gtid; t < fr.t1; t += c.gthreads) b0 = fminf(b0, o2f(c.l.tok_cost[t]));
    b0 = block_min(c.redf, b0);
    if (threadIdx.x == 0 && b0 != INFINITY) atomicMin(&cl->best[nf & 1], f2o(b0));
  }
  bool ok = cbar(c);
#ifdef B2T_WFST_TIMING
  c.tprev = __builtin_amdgcn_s_memtime();
#endif
  const int n = lens ? min(lens[u], T) : T;
  for (int i = 0; i < n && ok; ++i) {
    const float* row = logp + ((size_t)u * T + i) * C;
    // the blank-skipping decision (ctc_wfst_beam_search.cc:70-121) is taken by every member from the same numbers
    const int mode = frame_mode(row, C, o.blank_skip_thresh, is_last_blank, last_best);
    if (mode == 0) {                             // a blank frame: skipped, and remembered
      is_last_blank = 1;
      __syncthreads();
      if ((int)threadIdx.x < C) lastp[threadIdx.x] = row[threadIdx.x];
    }
    if (mode == 2) {
      __syncthreads();
      if ((int)threadIdx.x < C) ll[threadIdx.x] = o.acoustic_scale * lastp[threadIdx.x];
      if (c.gtid == 0 && fr.f < max_frames) c.l.mapping[fr.f] = num_input - 1;
      __syncthreads();
      ok = cadvance<ST, CP>(c, fr);
    }
    if (mode >= 1 && ok) {
      __syncthreads();
      if ((int)threadIdx.x < C) ll[threadIdx.x] = o.acoustic_scale * row[threadIdx.x];
      if (c.gtid == 0 && fr.f < max_frames) c.l.mapping[fr.f] = num_input;
      __syncthreads();
      ok = cadvance<ST, CP>(c, fr);
      is_last_blank = 0;
    }
    num_input += 1;
  }
  if (ok) {
    cbest_links(c, fr.pl0, fr.pl1);            // the last frame's backpointers
    ok = cbar(c);
  }
#ifdef B2T_WFST_TIMING
  if (c.gtid == 0 && u == 0)
    printf("wfst cluster u0 ticks: other %llu | cutoff %llu | passA light %llu | passA bar+heavy %llu | bestlinks %llu | clears %llu | barA %llu | passB %llu | barB %llu | closure %llu | epslinks %llu | barEnd %llu\n",
           c.tacc[0], c.tacc[1], c.tacc[11], c.tacc[2], c.tacc[3], c.tacc[4], c.tacc[5], c.tacc[6], c.tacc[7], c.tacc[8], c.tacc[9], c.tacc[10]);
  if (c.gtid == 0 && u == 0) printf("wfst cluster u0: heavy tokens %llu over %llu walks; frames %d, tokens %d, links %d, arcs %u\n", c.tacc[12], c.tacc[13], fr.f, ldi(&cl->n_tok), ldi(&cl->n_link), h->arcs_lo);
#endif
  __syncthreads();
  if (c.j == 0 && (int)threadIdx.x < MAX_C) c.l.last_prob[threadIdx.x] = lastp[threadIdx.x];
  if (c.gtid == 0) {
    h->n_frames = fr.f; h->num_input = num_input; h->is_last_blank = is_last_blank; h->last_best = last_best;
    h->n_tok = ldi(&cl->n_tok); h->n_link = ldi(&cl->n_link);
    cluster_leave(c, h);
  }
}

// (more utterances than clusters fit: still this kernel, with one member each -- see b2t_wfst_search_f32)
int wfst_cluster_search(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, const float* logp, const int32_t* lens,
                        int U, int T, int C, int G, hipStream_t stream) {
  static const bool no_stamp = getenv("B2T_WFST_STAMPED") && atoi(getenv("B2T_WFST_STAMPED")) == 0;   // A/B knob: clear a hash per frame (round 3)
  const bool stamped = !no_stamp && g->n_states < (1 << 27);
  // the slot format and the arc format are compile-time parameters of the kernel (see cclaim and g_il_t)
  const auto kernel = stamped ? (g->compact ? wfst_cluster_kernel<true, true> : wfst_cluster_kernel<true, false>)
                              : (g->compact ? wfst_cluster_kernel<false, true> : wfst_cluster_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3(cluster_grid(U, G)), dim3(NT), 0, stream, to_graph(g), (char*)state, state_bytes(o), to_opts(o),
                     o->max_frames, o->max_tokens, o->max_links, o->hash_size, G, U, logp, lens, T, C);
  B2T_CHECK_LAUNCH("b2t_wfst_search_f32 (cluster)");
  return 0;
}

}  // namespace b2t

