// wfst.hip (+ wfst_cluster.hip, wfst_prune.hip, wfst_lattice.hip; shared pieces in wfst_internal.h) — batched WFST token passing for gfx950: the search inner loop of the reference's LM decoder
// (language_model/runtime/core/kaldi/decoder/lattice-faster-decoder.cc: ProcessEmitting :722-824, ProcessNonemitting
// :839-909, GetCutoff :650-720, FindOrAddToken :250-295, PruneForwardLinks(Final) :297-470) under the frame loop of
// CtcWfstBeamSearch::Search (language_model/runtime/core/decoder/ctc_wfst_beam_search.cc:70-121).
//
// Two searchers with identical results (tests/test_gpu_wfst.py::test_cluster_search_equals_single_workgroup):
//   * wfst_search_kernel (this file): one workgroup per utterance; a frame's token hash (state -> token) lives in LDS when it fits
//     (<= 16384 slots = 128 KB);
//   * wfst_cluster_kernel (wfst_cluster.hip; the default when the XCD round-robin probe passes): 8 workgroups per utterance placed on one
//     XCD, sharing the frame through that XCD's L2 (hash, work lists, counters in HBM-backed scratch read with L1-bypassing
//     loads), a monotonic L2 counter as the cluster barrier.
// The decode graph (T o L o G as CSR arcs: nejm-brain-to-text_amd/wfst.py, csrc/graphc.cpp) lives in HBM and is shared by all
// utterances; tokens and forward links of every frame are appended to the utterance's state block in HBM (they ARE the lattice).
//
// What is data-parallel here and sequential in the reference:
//   * ProcessEmitting tightens `next_cutoff` while it walks the token list, so which over-the-cutoff dead-end tokens get
//     created depends on hash-list order.  Here the frame's minimum candidate cost is reduced first and every candidate
//     below min + adaptive_beam is kept -- the reference's FINAL cutoff.  Tokens the reference creates beyond it are never
//     expanded (ProcessNonemitting and the next frame's cutoff skip them) and disappear in FinalizeDecoding, so the
//     pruned lattice, best path and n-best are the same.  (Only GetCutoff's max_active / min_active COUNTS can see such
//     tokens: a difference exists only while max_active binds in consecutive frames.)
//   * ProcessNonemitting's work queue becomes Bellman-Ford sweeps over the frame's tokens until no cost changes (the
//     cluster search: one pass in which the thread that lowers a token's cost relaxes that token's arcs itself); forward
//     links are generated once, after convergence, with the final costs (what the queue leaves behind).
//   * PruneActiveTokens every prune_interval frames is a memory optimisation (it only removes what FinalizeDecoding would
//     remove as well: its extra_costs are lower bounds), so it is a pass of its own between search calls (wfst_prune_kernel,
//     b2t_wfst_prune) that shares prune_frame() with b2t_wfst_finalize; n-best lists are bit-identical with and without it.
// This file: the one-workgroup searcher (the fallback when the XCD probe fails, and the independent form the cluster searcher is
// tested against), the best-path kernel, the XCD probe and the cluster-size policy, and the entry points that are not a pass of
// their own (state_bytes / state_offsets, reset, set_cluster / cluster_size, search_f32, best_path).
#include "wfst_internal.h"

namespace b2t {
namespace {

#ifdef B2T_WFST_TIMING
#define WT(i) { if (threadIdx.x == 0) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); c.tacc[i] += now_ - c.tprev; c.tprev = now_; } }
#else
#define WT(i)
#endif

constexpr int WL_CAP = 4096;   // work-list capacity (a frame that has more tokens with epsilon arcs scans all its tokens, as before)

struct Ctx {
#ifdef B2T_WFST_TIMING
  unsigned long long tacc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
#endif
  Graph g; Lay l; Opts o;
  int max_frames, max_tok, max_link, hash;
  int* key; int* idx;          // the frame's hash (LDS or HBM)
  float* ll;                   // LDS: acoustic_scale * logp of the frame
  float* redf; int* redi;      // LDS reduction scratch [NT]
  int* sh;                     // LDS scalars: [0] n_tok, [1] n_link, [2] changed, [3] overflow, [4] work-list length, [5] tokens scanned so far, [6] work list overflowed
  int* wl;                     // LDS [WL_CAP]: the frame's tokens whose state has epsilon arcs (ProcessNonemitting's work list)
};

// k-th smallest (0-based) of the ordered cost keys of tokens [t0, t1): the radix select of wfst_internal.h with the histogram in LDS
__device__ float kth_cost(Ctx& c, int t0, int t1, int k) {
  int* hist = c.redi + 64;           // [256]; redi[0 .. 63] stay free for block_sum, redi[320 ..] hold the round's result
  int* res = c.redi + 320;           // [0] chosen digit, [1] rank inside the chosen bin
  unsigned prefix = 0u;
  int rank = k;
  for (int round = 0; round < 4; ++round) {
    radix_count<false>(hist, c.l.tok_cost, t0, t1, NT, round, prefix);
    radix_pick<false>(res, rank, hist);
    prefix |= (unsigned)res[0] << (24 - 8 * round);
    rank = res[1];
  }
  __syncthreads();
  return o2f(prefix);
}

// FindOrAddToken, claim phase: make sure `state` has a slot (and a token) in the frame being built; returns the slot
// (idx[slot] is valid after the next barrier) or -1 when the hash is full
__device__ __forceinline__ int claim(Ctx& c, int state) {
  const int mask = c.hash - 1;
  unsigned s = hash_of(state, mask);
  for (int probe = 0; probe < c.hash; ++probe, s = (s + 1) & mask) {
    const int k = __hip_atomic_load(&c.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (k == state) return (int)s;
    if (k == -1) {
      int expected = -1;
      if (__hip_atomic_compare_exchange_strong(&c.key[s], &expected, state, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) {
        const int id = atomicAdd(&c.sh[0], 1);
        if (id < c.max_tok) {
          c.idx[s] = id;
          c.l.tok_state[id] = state; c.l.tok_cost[id] = UMAX; c.l.tok_best[id] = BEST_UNSET; c.l.tok_extra[id] = 0u;
        } else {
          c.idx[s] = -1; atomicOr(&c.sh[3], 1);
        }
        return (int)s;
      }
      if (expected == state) return (int)s;
    }
  }
  atomicOr(&c.sh[3], 4);   // hash full
  return -1;
}
__device__ __forceinline__ int find(Ctx& c, int state) {
  const int mask = c.hash - 1;
  unsigned s = hash_of(state, mask);
  for (int probe = 0; probe < c.hash; ++probe, s = (s + 1) & mask) {
    const int k = c.key[s];
    if (k == state) return c.idx[s];
    if (k == -1) return -1;
  }
  return -1;
}

// ProcessNonemitting over the tokens [n0, ...) of the frame being built + generation of their epsilon links.
// Only the tokens of states WITH epsilon arcs matter (word ends: a few hundred of a frame's thousands), and the closure takes
// several Bellman-Ford rounds of two passes each: the tokens are classified once (token -> state -> n_eps, two dependent
// gathers) into an LDS work list that grows as the closure creates tokens; the rounds walk the list.
__device__ void nonemitting(Ctx& c, int n0, float cutoff) {
  const Graph& g = c.g;
  __syncthreads();
  if (threadIdx.x == 0) { c.sh[4] = 0; c.sh[5] = n0; c.sh[6] = 0; }
  auto extend = [&]() {                       // classify the tokens created since the last call (ends with a barrier)
    __syncthreads();
    const int from = c.sh[5], upto = min(c.sh[0], c.max_tok);
    for (int t = from + threadIdx.x; t < upto; t += NT) {
      if (g.n_eps[c.l.tok_state[t]] == 0) continue;
      const int i = atomicAdd(&c.sh[4], 1);
      if (i < WL_CAP) c.wl[i] = t; else c.sh[6] = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) c.sh[5] = upto;
    __syncthreads();
    return upto;
  };
  auto for_each = [&](int n_now, auto&& body) {   // body(t) for every token of [n0, n_now) whose state has epsilon arcs
    if (c.sh[6]) { for (int t = n0 + threadIdx.x; t < n_now; t += NT) body(t); }
    else { const int n = c.sh[4]; for (int i = threadIdx.x; i < n; i += NT) body(c.wl[i]); }
  };
  for (;;) {
    const int n_now = extend();
    if (threadIdx.x == 0) c.sh[2] = 0;
    __syncthreads();
    for (int phase = 0; phase < 2; ++phase) {
      for_each(n_now, [&](int t) {
        const int s = c.l.tok_state[t];
        const int ne = g.n_eps[s];
        if (ne == 0) return;
        const float cur = o2f(c.l.tok_cost[t]);
        if (!(cur < cutoff)) return;
        const int a0 = g.row[s];
        for (int a = a0; a < a0 + ne; ++a) {
          const float tot = cur + g_w(g, a);
          if (tot < cutoff) {
            if (phase == 0) {
              claim(c, g.next[a]);
            } else {
              const int id = find(c, g.next[a]);
              if (id >= 0) {
                const unsigned nb = f2o(tot);
                const unsigned old = atomicMin(&c.l.tok_cost[id], nb);
                if (nb < old) c.sh[2] = 1;
              }
            }
          }
        }
      });
      __syncthreads();
    }
    if (c.sh[2] == 0) break;
  }
  // forward links of the epsilon arcs, with the converged costs
  const int n_now = extend();
  for_each(n_now, [&](int t) {
    const int s = c.l.tok_state[t];
    const int ne = g.n_eps[s];
    if (ne == 0) return;
    const float cur = o2f(c.l.tok_cost[t]);
    if (!(cur < cutoff)) return;
    const int a0 = g.row[s];
    for (int a = a0; a < a0 + ne; ++a) {
      const float tot = cur + g_w(g, a);
      if (tot < cutoff) {
        const int id = find(c, g.next[a]);
        if (id < 0) continue;
        const int li = atomicAdd(&c.sh[1], 1);
        if (li < c.max_link) {
          c.l.link_src[li] = t; c.l.link_dst[li] = id; c.l.link_arc[li] = a; c.l.link_ac[li] = 0.f; c.l.link_graph[li] = g_w(g, a);
        } else {
          atomicOr(&c.sh[3], 2);
        }
      }
    }
  });
  __syncthreads();
}

// backpointers: among the links into the tokens of the new frame, the one whose cost equals the token's final cost
__device__ void best_links(Ctx& c, int l0, int l1) {
  for (int li = l0 + threadIdx.x; li < l1; li += NT) best_link<false>(c.l, li, c.l.link_src[li], c.l.link_dst[li]);
  __syncthreads();
}

__device__ void clear_hash(Ctx& c) {
  for (int i = threadIdx.x; i < c.hash; i += NT) c.key[i] = -1;
  __syncthreads();
}

// InitDecoding (:57-75)
__device__ void init_decoding(Ctx& c) {
  clear_hash(c);
  // the cluster search's scratch starts from zero whatever the caller's buffer held (its histograms are only re-zeroed AFTER a
  // frame's cut-off used them)
  for (int i = threadIdx.x; i < (int)(sizeof(Clu) / sizeof(int)); i += NT) reinterpret_cast<int*>(c.l.clu)[i] = 0;
  // ... and from two EMPTY frame hashes: the cluster search stamps its slots with the frame (below) instead of clearing a hash
  // per frame, so what an earlier utterance left in this state block must not look like a live entry of this one
  {
    unsigned long long* s0 = reinterpret_cast<unsigned long long*>(c.l.gkey);
    unsigned long long* s1 = reinterpret_cast<unsigned long long*>(c.l.gkey2);
    for (int i = threadIdx.x; i < c.hash; i += NT) { s0[i] = ~0ull; s1[i] = ~0ull; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Hdr* h = c.l.h;
    h->n_frames = 0; h->overflow = 0; h->num_input = 0; h->is_last_blank = 0; h->last_best = 0; h->finalized = 0;
    h->final_best = 0.f; h->has_final = 0; h->arcs_lo = 0u; h->arcs_hi = 0u;
    h->links_marked = 0; h->n_prunes = 0; h->peak_tok = 0; h->peak_link = 0; h->removed_tok = 0; h->removed_link = 0;
    c.l.clu->bar = 0u; c.l.clu->bar_base = 0u; c.l.clu->overflow = 0;
    c.sh[0] = 0; c.sh[1] = 0; c.sh[3] = 0;
    c.l.tok_off[0] = 0;
    c.l.link_off[0] = 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) claim(c, c.g.start);
  __syncthreads();
  if (threadIdx.x == 0) { c.l.tok_cost[0] = f2o(0.f); c.l.tok_best[0] = -1; }
  __syncthreads();
  nonemitting(c, 0, c.o.beam);
  best_links(c, 0, min(c.sh[1], c.max_link));
  if (threadIdx.x == 0) {
    c.l.tok_best[0] = -1;
    c.l.tok_off[1] = min(c.sh[0], c.max_tok);
    c.l.link_off[1] = min(c.sh[1], c.max_link);    // [eps links of frame 0]
    c.l.h->n_tok = c.sh[0]; c.l.h->n_link = c.sh[1]; c.l.h->overflow = c.sh[3];
  }
  __syncthreads();
}

// one AdvanceDecoding(.., 1): ProcessEmitting + ProcessNonemitting on the row `logp` (already in c.ll, scaled)
__device__ void advance(Ctx& c) {
  const Graph& g = c.g;
  const int f = c.l.h->n_frames;
  if (f >= c.max_frames) { if (threadIdx.x == 0) atomicOr(&c.sh[3], 8); __syncthreads(); return; }
  const int t0 = c.l.tok_off[f], t1 = c.l.tok_off[f + 1];
  WT(0)
  // ---- GetCutoff (:650-720)
  float best = INFINITY;
  for (int t = t0 + threadIdx.x; t < t1; t += NT) best = fminf(best, o2f(c.l.tok_cost[t]));
  best = block_min(c.redf, best);
  const int n = t1 - t0;
  const float beam_cutoff = best + c.o.beam;
  float cur_cutoff = beam_cutoff, adaptive = c.o.beam;
  {
    float max_cut = INFINITY, min_cut = INFINITY;
    if (n > c.o.max_active) max_cut = kth_cost(c, t0, t1, c.o.max_active);
    if (max_cut < beam_cutoff) {
      cur_cutoff = max_cut; adaptive = max_cut - best + c.o.beam_delta;
    } else {
      if (n > c.o.min_active) min_cut = c.o.min_active == 0 ? best : kth_cost(c, t0, t1, c.o.min_active);
      if (min_cut > beam_cutoff) { cur_cutoff = min_cut; adaptive = min_cut - best + c.o.beam_delta; }
    }
  }
  WT(1)   // best + k-th cost
  const float cost_offset = -best;
  const float lp = c.o.length_penalty;
  // ---- ProcessEmitting (:722-824).  Out-degrees are skewed (1-3 arcs inside a word, hundreds at the word-boundary states
  // of L o G, each arc a dependent chain of gathers + a hash probe), so a thread that owned a token would idle most of its
  // wave.  A wave takes 64 consecutive tokens, scans their degrees through lane permutes and walks the FLATTENED arc list 64
  // arcs at a time: arc j belongs to the first lane whose inclusive degree sum exceeds j (6-step search through permutes).
  float mn = INFINITY;
  int narcs = 0;
  auto arc_cost = [&](float cur, int s, int a, float& ac, float& gc) {
    ac = cost_offset - c.ll[g_il(g, a) - 1];
    gc = g_w(g, a);
    if (lp != 0.f && g.next[a] != s) gc += lp;     // (no gather of the destination when there is no length penalty)
    return cur + ac + gc;
  };
  const int lane = threadIdx.x & 63;
  auto walk = [&](auto&& visit) {          // visit(token, its cost, its state, arc) for every emitting arc of every token under the cutoff
    for (int base = t0 + (int)threadIdx.x - lane; base < t1; base += NT) {    // wave-uniform
      const int t = base + lane;
      float cur = INFINITY; int s = 0, a0 = 0, deg = 0;
      if (t < t1) {
        cur = o2f(c.l.tok_cost[t]);
        if (cur <= cur_cutoff) { s = c.l.tok_state[t]; a0 = g.row[s] + g.n_eps[s]; deg = g.row[s + 1] - a0; }
      }
      int incl = deg;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off, 64); if (lane >= off) incl += v; }
      const int total = __shfl(incl, 63, 64), excl = incl - deg;
      for (int jb = 0; jb < total; jb += 64) {
        const int jj = jb + lane;
        int owner = 0;                      // number of lanes whose inclusive sum is <= jj
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) { const int v = __shfl(incl, owner + step - 1, 64); if (v <= jj) owner += step; }
        owner = min(owner, 63);
        const int oa0 = __shfl(a0, owner, 64), oex = __shfl(excl, owner, 64), os = __shfl(s, owner, 64);
        const float ocur = __shfl(cur, owner, 64);
        if (jj < total) visit(base + owner, ocur, os, oa0 + (jj - oex));
      }
      narcs += deg;
    }
  };
  // Pass A: the frame's best candidate -> next_cutoff
  walk([&](int, float cur, int s, int a) { float ac, gc; mn = fminf(mn, arc_cost(cur, s, a, ac, gc)); });
  mn = block_min(c.redf, mn);
  narcs = block_sum(c.redi, narcs);
  if (threadIdx.x == 0) {
    const unsigned lo = c.l.h->arcs_lo + (unsigned)narcs;
    if (lo < c.l.h->arcs_lo) c.l.h->arcs_hi += 1u;
    c.l.h->arcs_lo = lo;
  }
  const float next_cutoff = mn + adaptive;
  WT(2)   // pass A
  clear_hash(c);
  WT(3)   // clear hash
  const int n0 = min(c.sh[0], c.max_tok), l0 = min(c.sh[1], c.max_link);
  // pass B.  Phase 0 walks the arcs once: every surviving arc claims its destination's hash slot and is recorded as a
  // forward link that still names the SLOT (token ids are handed out by the claim's winner and are only safe to read after
  // a barrier).  Phase 1 is a flat, perfectly balanced loop over those links: slot -> token id, cost minimisation.
  {
    auto visit = [&](int t, float cur, int s, int a) {
      float ac, gc;
      const float tot = arc_cost(cur, s, a, ac, gc);
      if (!(tot < next_cutoff)) return;
      const int slot = claim(c, g.next[a]);
      if (slot < 0) return;
      const int li = atomicAdd(&c.sh[1], 1);
      if (li < c.max_link) {
        c.l.link_src[li] = t; c.l.link_dst[li] = slot; c.l.link_arc[li] = a; c.l.link_ac[li] = ac; c.l.link_graph[li] = gc;
      } else {
        atomicOr(&c.sh[3], 2);
      }
    };
    { const int keep = narcs; walk(visit); narcs = keep; }
    __syncthreads();
    WT(4)   // pass B: arc walk (claim + link records)
    const int l1 = min(c.sh[1], c.max_link);
    for (int li = l0 + threadIdx.x; li < l1; li += NT) {
      int id = c.idx[c.l.link_dst[li]];
      if (id < 0) id = 0;                  // token capacity exceeded: the overflow bit is set and the caller discards the result
      const float tot = o2f(c.l.tok_cost[c.l.link_src[li]]) + c.l.link_ac[li] + c.l.link_graph[li];
      c.l.link_dst[li] = id;
      atomicMin(&c.l.tok_cost[id], f2o(tot));
    }
    __syncthreads();
    WT(5)   // pass B: link walk (token ids, costs)
  }
  if (threadIdx.x == 0) c.l.link_off[2 * f + 2] = min(c.sh[1], c.max_link);   // [emitting links f -> f+1]
  __syncthreads();
  nonemitting(c, n0, next_cutoff);
  WT(6)   // epsilon closure + links
  best_links(c, l0, min(c.sh[1], c.max_link));
  WT(7)   // best links
  if (threadIdx.x == 0) {
    c.l.cost_offset[f] = cost_offset;
    c.l.tok_off[f + 2] = min(c.sh[0], c.max_tok);
    c.l.link_off[2 * f + 3] = min(c.sh[1], c.max_link);                       // [eps links of frame f+1]
    c.l.h->n_frames = f + 1;
    c.l.h->n_tok = c.sh[0]; c.l.h->n_link = c.sh[1]; c.l.h->overflow = c.sh[3];
  }
  __syncthreads();
}

__device__ void setup(Ctx& c, const Graph& g, char* state, int u, size_t state_bytes, const Opts& o, int max_frames, int max_tok,
                      int max_link, int hash, int* smem_hash, float* ll, float* redf, int* redi, int* sh, int* wl) {
  c.g = g; c.o = o; c.max_frames = max_frames; c.max_tok = max_tok; c.max_link = max_link; c.hash = hash;
  layout(state + (size_t)u * state_bytes, max_frames, max_tok, max_link, hash, &c.l);
  if (smem_hash) { c.key = smem_hash; c.idx = smem_hash + hash; } else { c.key = c.l.gkey; c.idx = c.l.gidx; }
  c.ll = ll; c.redf = redf; c.redi = redi; c.sh = sh; c.wl = wl;
}

}  // namespace

__global__ __launch_bounds__(NT) void wfst_reset_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                         int max_tok, int max_link, int hash, int use_lds) {
  extern __shared__ int dyn[];
  __shared__ float ll[MAX_C], redf[NT];
  __shared__ int redi[NT], sh[8], wl[WL_CAP];
  Ctx c;
  setup(c, g, state, blockIdx.x, state_bytes, o, max_frames, max_tok, max_link, hash, use_lds ? dyn : nullptr, ll, redf, redi, sh, wl);
  init_decoding(c);
}

// CtcWfstBeamSearch::Search (ctc_wfst_beam_search.cc:70-121) over rows [0, lens[u]) of logp[u]
__global__ __launch_bounds__(NT) void wfst_search_kernel(Graph g, char* state, size_t state_bytes, Opts o, int max_frames,
                                                          int max_tok, int max_link, int hash, int use_lds,
                                                          const float* __restrict__ logp, const int* __restrict__ lens, int T, int C) {
  extern __shared__ int dyn[];
  __shared__ float ll[MAX_C], redf[NT];
  __shared__ int redi[NT], sh[8], wl[WL_CAP];
  __shared__ int dec[2];
  Ctx c;
  const int u = blockIdx.x;
  setup(c, g, state, u, state_bytes, o, max_frames, max_tok, max_link, hash, use_lds ? dyn : nullptr, ll, redf, redi, sh, wl);
  if (threadIdx.x == 0) { sh[0] = c.l.h->n_tok; sh[1] = c.l.h->n_link; sh[2] = 0; sh[3] = c.l.h->overflow; }
  __syncthreads();
  const int n = lens ? min(lens[u], T) : T;
  for (int i = 0; i < n; ++i) {
    const float* row = logp + ((size_t)u * T + i) * C;
    if (threadIdx.x == 0) {
      Hdr* h = c.l.h;
      int last_best = h->last_best;
      const int mode = frame_mode(row, C, o.blank_skip_thresh, h->is_last_blank, last_best);
      if (mode == 0) {                   // a blank frame: skipped, and remembered
        h->is_last_blank = 1;
        for (int k = 0; k < C; ++k) c.l.last_prob[k] = row[k];
      } else {
        h->last_best = last_best;
      }
      dec[0] = mode;
    }
    __syncthreads();
    const int mode = dec[0];
    if (mode == 2) {
      if ((int)threadIdx.x < C) ll[threadIdx.x] = o.acoustic_scale * c.l.last_prob[threadIdx.x];
      if (threadIdx.x == 0 && c.l.h->n_frames < max_frames) c.l.mapping[c.l.h->n_frames] = c.l.h->num_input - 1;
      __syncthreads();
      advance(c);
    }
    if (mode >= 1) {
      if ((int)threadIdx.x < C) ll[threadIdx.x] = o.acoustic_scale * row[threadIdx.x];
      if (threadIdx.x == 0 && c.l.h->n_frames < max_frames) c.l.mapping[c.l.h->n_frames] = c.l.h->num_input;
      __syncthreads();
      advance(c);
      if (threadIdx.x == 0) c.l.h->is_last_blank = 0;
    }
    if (threadIdx.x == 0) c.l.h->num_input += 1;
    __syncthreads();
  }
#ifdef B2T_WFST_TIMING
  if (threadIdx.x == 0 && blockIdx.x == 0)
    printf("wfst u0 cycles: other %llu | cutoff %llu | passA %llu | clear %llu | claim %llu | relax %llu | eps %llu | best_links %llu\n", c.tacc[0], c.tacc[1],
           c.tacc[2], c.tacc[3], c.tacc[4], c.tacc[5], c.tacc[6], c.tacc[7]);
#endif
}

constexpr int BP_NT = 256;   // threads of the best-path kernel (parallel argmin over the last frame; the backtrace: a serial chain walk + parallel gathers)
constexpr int BP_CAP = 1024;  // links of the best path handled per round of the backtrace
// Best path by backpointers (lattice-faster-online-decoder.cc:58-150): alignment (ilabels), words (olabels), costs.
// use_final: 0 = partial result (any token of the last frame), 1 = with final costs (after b2t_wfst_finalize).
__global__ void wfst_best_path_kernel(Graph g, char* state, size_t state_bytes, int max_frames, int max_tok, int max_link, int hash,
                                      int use_final, int max_len, int* ali, int* ali_frame, int* n_ali, int* words, int* n_words,
                                      float* costs) {
  const int u = blockIdx.x;
  Lay l;
  layout(state + (size_t)u * state_bytes, max_frames, max_tok, max_link, hash, &l);
  const int F = l.h->n_frames;
  if (threadIdx.x == 0) { n_ali[u] = 0; n_words[u] = 0; costs[2 * u] = 0.f; costs[2 * u + 1] = 0.f; }
  if (F == 0) return;
  // the cheapest token of the last frame (first one among equals, as a serial scan finds it): all threads, then a reduction
  __shared__ float r_cost[BP_NT], r_fc[BP_NT];
  __shared__ int r_tok[BP_NT];
  const int t0 = l.tok_off[F], t1 = l.tok_off[F + 1];
  float best = INFINITY, best_fc = 0.f; int bt = -1;
  const bool with_final = use_final && l.h->has_final;
  for (int t = t0 + (int)threadIdx.x; t < t1; t += BP_NT) {
    float cost = o2f(l.tok_cost[t]), fc = 0.f;
    if (with_final) {
      fc = g.final_cost[l.tok_state[t]];
      cost = fc == INFINITY ? INFINITY : cost + fc;
    }
    if (cost < best) { best = cost; bt = t; best_fc = fc; }
  }
  r_cost[threadIdx.x] = best; r_fc[threadIdx.x] = best_fc; r_tok[threadIdx.x] = bt;
  __syncthreads();
  for (int sft = BP_NT / 2; sft > 0; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
      const float oc = r_cost[threadIdx.x + sft]; const int ot = r_tok[threadIdx.x + sft];
      const float mc = r_cost[threadIdx.x]; const int mt = r_tok[threadIdx.x];
      if (ot >= 0 && (mt < 0 || oc < mc || (oc == mc && ot < mt))) {
        r_cost[threadIdx.x] = oc; r_tok[threadIdx.x] = ot; r_fc[threadIdx.x] = r_fc[threadIdx.x + sft];
      }
    }
    __syncthreads();
  }
  best = r_cost[0]; bt = r_tok[0]; best_fc = r_fc[0];
  (void)best;
  if (bt < 0) return;
  // Walk back.  The chain itself -- token -> {its best link, that link's source token} -- is ONE dependent load per hop and is
  // all thread 0 does per hop (the link ids go to LDS); what a link contributes (labels, costs, the frame it belongs to, that
  // frame's cost offset and input frame) is then fetched by all threads at once, frames from a prefix count of the emitting
  // links, and thread 0 only sums and emits from LDS, in walk order (the sums are the serial walk's, bit for bit).  The
  // first version did everything inside the chain: four dependent loads and a branch per hop, ~1.2 us per decoded frame, a
  // quarter of a streamed frame's latency at 100 frames.  Results are written from the end of the buffers, then moved up.
  __shared__ int s_li[BP_CAP], s_il[BP_CAP], s_ol[BP_CAP], s_map[BP_CAP], s_ctl[4], s_cnt[BP_NT];
  __shared__ float s_gc[BP_CAP], s_ac[BP_CAP];
  int na = 0, nw = 0, frame = F - 1;
  float gc = best_fc, ac = 0.f;
  int* a_out = ali + (size_t)u * max_len; int* f_out = ali_frame + (size_t)u * max_len; int* w_out = words + (size_t)u * max_len;
  if (threadIdx.x == 0) { s_ctl[0] = bt; s_ctl[2] = 0; }
  __syncthreads();
  for (;;) {
    if (threadIdx.x == 0) {
      int t = s_ctl[0], n = 0, done = 0;
      while (n < BP_CAP) {
        const long long bw = l.tok_best[t];
        if (bw < 0 || bw == BEST_UNSET) { done = 1; break; }
        s_li[n++] = (int)(bw >> 32);
        t = (int)(unsigned)(bw & 0xffffffffLL);
      }
      s_ctl[0] = t; s_ctl[1] = n; s_ctl[2] = done;
    }
    __syncthreads();
    const int n = s_ctl[1], done = s_ctl[2];
    constexpr int PER = BP_CAP / BP_NT;            // consecutive entries per thread (the prefix count below)
    const int i0 = (int)threadIdx.x * PER;
    int emit = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = i0 + k;
      if (i < n) {
        const int li = s_li[i], a = l.link_arc[li];
        const int il = g_il(g, a);
        s_il[i] = il; s_ol[i] = g_ol(g, a); s_gc[i] = l.link_graph[li]; s_ac[i] = l.link_ac[li];
        emit += il != 0;
      }
    }
    s_cnt[threadIdx.x] = emit;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < BP_NT; ++w) { const int v = s_cnt[w]; if (w < (int)threadIdx.x) before += v; total += v; }
    {
      int fr = frame - before;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int i = i0 + k;
        if (i < n && s_il[i] != 0) { s_ac[i] -= l.cost_offset[fr]; s_map[i] = l.mapping[fr]; --fr; }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int i = 0; i < n; ++i) {
        gc += s_gc[i];
        if (s_il[i] != 0) {
          ac += s_ac[i];
          if (na < max_len) { a_out[max_len - 1 - na] = s_il[i]; f_out[max_len - 1 - na] = s_map[i]; }
          ++na;
        }
        if (s_ol[i] != 0) { if (nw < max_len) w_out[max_len - 1 - nw] = s_ol[i]; ++nw; }
      }
      s_ctl[3] = na; s_cnt[0] = nw;
    }
    frame -= total;
    __syncthreads();
    if (done) break;
  }
  na = s_ctl[3]; nw = s_cnt[0];
  const int ka = min(na, max_len), kw = min(nw, max_len);
  // move up: chunk by chunk, a chunk's reads before its writes (its targets never reach a later chunk's sources)
  for (int base = 0; base < max(ka, kw); base += BP_NT) {
    const int i = base + (int)threadIdx.x;
    int va = 0, vf = 0, vw = 0;
    if (i < ka) { va = a_out[max_len - ka + i]; vf = f_out[max_len - ka + i]; }
    if (i < kw) vw = w_out[max_len - kw + i];
    __syncthreads();
    if (i < ka) { a_out[i] = va; f_out[i] = vf; }
    if (i < kw) w_out[i] = vw;
    __syncthreads();
  }
  if (threadIdx.x == 0) { n_ali[u] = ka; n_words[u] = kw; costs[2 * u] = gc; costs[2 * u + 1] = ac; }
}

}  // namespace b2t

using namespace b2t;

extern "C" size_t b2t_wfst_state_bytes(int max_frames, int max_tokens, int max_links, int hash_size) {
  return layout(nullptr, max_frames, max_tokens, max_links, hash_size, nullptr);
}

namespace {
size_t lds_hash_bytes(const b2t_wfst_opts_t* o) { return o->hash_size <= 16384 ? (size_t)o->hash_size * 2 * sizeof(int) : 0; }   // <= 128 KB of the CU's 160 KB
}  // namespace

extern "C" int b2t_wfst_reset(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, int U, void* stream) {
  { int rc = check_args(g, o, state, U, "wfst_reset"); if (rc) return rc; }
  const size_t sb = state_bytes(o), lds = lds_hash_bytes(o);
  allow_lds(wfst_reset_kernel, lds);
  hipLaunchKernelGGL(wfst_reset_kernel, dim3(U), dim3(NT), lds, as_stream(stream), to_graph(g), (char*)state, sb, to_opts(o),
                     o->max_frames, o->max_tokens, o->max_links, o->hash_size, lds ? 1 : 0);
  B2T_CHECK_LAUNCH("b2t_wfst_reset");
  return 0;
}

// Workgroups per utterance of the search: the largest of 8 / 4 / 2 / 1 that keeps every cluster resident (one 1024-thread
// workgroup per CU, 256 CUs); B2T_WFST_CLUSTER overrides (1 = the single-workgroup kernel with its LDS hash).
// The clusters assume what the hardware does in this partition mode: workgroup b of a launch runs on XCD b % 8.  Probed once
// per process (256 one-wave workgroups report their XCC_ID): if blocks with equal b % 8 do not share an XCD, or the eight
// classes are not on eight different XCDs, the search falls back to one workgroup per utterance.  (The kernel checks again,
// per launch, and refuses to decode on a mismatch.)
__global__ void wfst_xcd_probe_kernel(unsigned* out) { if (threadIdx.x == 0) out[blockIdx.x] = xcc_of(); }
static bool wfst_xcd_roundrobin_ok() {
  static int ok = -1;
  if (ok >= 0) return ok == 1;
  ok = 0;
  unsigned* d = nullptr;
  unsigned h[256];
  if (hipMalloc(reinterpret_cast<void**>(&d), sizeof(h)) != hipSuccess) { (void)hipGetLastError(); return false; }
  hipLaunchKernelGGL(wfst_xcd_probe_kernel, dim3(256), dim3(64), 0, nullptr, d);
  const bool copied = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
  (void)hipFree(d);
  if (!copied) { (void)hipGetLastError(); return false; }
  unsigned seen = 0;
  for (int i = 0; i < 256; ++i) if (h[i] > 7u || h[i] != h[i & 7]) return false;
  for (int i = 0; i < 8; ++i) seen |= 1u << h[i];
  if (seen != 0xffu) return false;
  ok = 1;
  return true;
}

static int g_cluster_override = 0;
// 0 = automatic; 2 .. 32 = that many workgroups per utterance; 1 = the single-workgroup kernel (frame hash in LDS: round 2's
// search, kept as the reference the cluster search is tested against); -1 = the cluster kernel with ONE member
extern "C" int b2t_wfst_set_cluster(int G) { g_cluster_override = G < -1 ? 0 : G; return 0; }
static int wfst_forced_cluster() {
  static const int env = getenv("B2T_WFST_CLUSTER") ? atoi(getenv("B2T_WFST_CLUSTER")) : 0;
  return g_cluster_override ? g_cluster_override : env;
}
extern "C" int b2t_wfst_cluster_size(int U) {
  const int forced = wfst_forced_cluster();
  if (forced == -1) return 1;
  if (forced >= 1) return forced >= 32 ? 32 : forced >= 16 ? 16 : forced >= 8 ? 8 : forced >= 4 ? 4 : forced >= 2 ? 2 : 1;
  // 8 workgroups per utterance where they are all resident.  Larger clusters work (b2t_wfst_set_cluster(16 / 32): up to a whole
  // XCD per utterance, tested against the single-workgroup search) but buy nothing: one utterance takes 11.7 / 11.1 / 11.7 ms
  // with 8 / 16 / 32 workgroups, eight take 14.9 / 14.1 / 14.9 -- beyond 8 members a frame is its ~6 cluster barriers and the
  // chains of dependent L2 round trips between them (~100 us), not the walk over its tokens and arcs.
  // one workgroup (1024 threads) per CU: the members of every cluster must be co-resident (their barrier is an L2 spin counter),
  // so the slot count is the device's CU count, not a constant (a partition or a smaller part has fewer)
  static int slots = -1;
  if (slots < 0) {
    int dev = 0; hipDeviceProp_t p;
    slots = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
  }
  for (int G = 8; G > 1; G >>= 1) if ((U + 7) / 8 * 8 * G <= slots) return wfst_xcd_roundrobin_ok() ? G : 1;
  return 1;
}

extern "C" int b2t_wfst_search_f32(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, const float* logp,
                                   const int32_t* lens, int U, int T, int C, void* stream) {
  { int rc = check_args(g, o, state, U, "wfst_search"); if (rc) return rc; }
  B2T_REQUIRE(logp && T > 0 && C > 1 && C <= MAX_C, "wfst_search: bad logp shape T=%d C=%d", T, C);
  const size_t sb = state_bytes(o), lds = lds_hash_bytes(o);
  const int G = b2t_wfst_cluster_size(U);
  // More utterances than clusters fit: still the cluster kernel, with one member each (its barriers then cost an atomic, and
  // its one-pass epsilon closure and single claim-relax-link walk make it faster than the single-workgroup kernel with its
  // ~45 __syncthreads per frame: 55.4 against 63.1 ms for 256 utterances).
  if (G > 1 || wfst_forced_cluster() != 1) return wfst_cluster_search(g, o, state, logp, lens, U, T, C, G, as_stream(stream));
  allow_lds(wfst_search_kernel, lds);
  hipLaunchKernelGGL(wfst_search_kernel, dim3(U), dim3(NT), lds, as_stream(stream), to_graph(g), (char*)state, sb, to_opts(o),
                     o->max_frames, o->max_tokens, o->max_links, o->hash_size, lds ? 1 : 0, logp, lens, T, C);
  B2T_CHECK_LAUNCH("b2t_wfst_search_f32");
  return 0;
}

extern "C" int b2t_wfst_best_path(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, const void* state, int U, int use_final,
                                  int max_len, int32_t* alignment, int32_t* align_frame, int32_t* n_align, int32_t* words,
                                  int32_t* n_words, float* costs, void* stream) {
  { int rc = check_args(g, o, const_cast<void*>(state), U, "wfst_best_path"); if (rc) return rc; }
  B2T_REQUIRE(max_len > 0 && alignment && align_frame && n_align && words && n_words && costs, "wfst_best_path: null output");
  const size_t sb = state_bytes(o);
  hipLaunchKernelGGL(wfst_best_path_kernel, dim3(U), dim3(BP_NT), 0, as_stream(stream), to_graph(g), (char*)const_cast<void*>(state), sb,
                     o->max_frames, o->max_tokens, o->max_links, o->hash_size, use_final, max_len, alignment, align_frame, n_align,
                     words, n_words, costs);
  B2T_CHECK_LAUNCH("b2t_wfst_best_path");
  return 0;
}

// Host views into one utterance's state block (offsets in bytes from the block's start), for copying the lattice out.
extern "C" int b2t_wfst_state_offsets(int max_frames, int max_tokens, int max_links, int hash_size, long long* off16) {
  B2T_REQUIRE(off16 != nullptr, "wfst_state_offsets: null output");
  Lay l;
  char* base = reinterpret_cast<char*>(0x1000);   // any non-null base: only differences are used
  layout(base, max_frames, max_tokens, max_links, hash_size, &l);
  const char* ptrs[16] = {(char*)l.h, (char*)l.mapping, (char*)l.tok_off, (char*)l.link_off, (char*)l.cost_offset, (char*)l.tok_state,
                          (char*)l.tok_cost, (char*)l.tok_extra, (char*)l.link_src, (char*)l.link_dst, (char*)l.link_arc,
                          (char*)l.link_ac, (char*)l.link_graph, (char*)l.link_alive, (char*)l.tok_best, (char*)l.last_prob};
  for (int i = 0; i < 16; ++i) off16[i] = (long long)(ptrs[i] - base);
  return 0;
}
