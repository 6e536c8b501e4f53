// wfst_internal.h -- what the units of the WFST decoder share (wfst.hip: the one-workgroup searcher, best path, entry points;
// wfst_cluster.hip: the cluster searcher; wfst_prune.hip: FinalizeDecoding / PruneActiveTokens; wfst_lattice.hip: the lattice
// extraction): the state-block layout, the decode graph, the cluster context and barrier, and every device piece that more than
// one kernel family uses -- each written ONCE.  Everything lives in an anonymous namespace: each unit gets its own copy and no
// symbol crosses a unit, except the launcher declared at the end; a unit that does not use one of the non-inline functions
// (cbar, the host helpers: [[maybe_unused]]) simply drops it.
// Lay, Graph and Opts go into helpers BY VALUE (see prune_frame in wfst_prune.hip for what a reference cost).
#pragma once
#include <float.h>
#include <stdlib.h>
#include "common.h"

namespace b2t {
namespace {

constexpr int NT = 1024;   // one workgroup per utterance; a frame holds thousands of tokens, each a dependent chain of gathers
constexpr unsigned UMAX = 0xffffffffu;
constexpr int MAX_C = 64;

struct Graph {
  const int* row; const int* ilabel; const int* olabel; const float* weight; const int* next; const int* n_eps;
  const float* final_cost; int start;
  // compact arcs (round 4; b2t_wfst_graph_t.compact): 10 bytes per arc instead of 16 -- labels = ilabel | olabel << 7 (one
  // word), the weight as IEEE half (|error| <= 2^-11 relative), next as before; the full-width arrays are then not read
  const unsigned* labels; const _Float16* w16; int compact;
};
__device__ __forceinline__ int g_il(const Graph& g, int a) { return g.compact ? (int)(g.labels[a] & 127u) : g.ilabel[a]; }
__device__ __forceinline__ int g_ol(const Graph& g, int a) { return g.compact ? (int)(g.labels[a] >> 7) : g.olabel[a]; }
__device__ __forceinline__ float g_w(const Graph& g, int a) { return g.compact ? (float)g.w16[a] : g.weight[a]; }
// the same with the arc format known at compile time (the cluster search's inner loops: the run-time test cost 3.5 %)
template <bool CP> __device__ __forceinline__ int g_il_t(const Graph& g, int a) { if constexpr (CP) return (int)(g.labels[a] & 127u); else return g.ilabel[a]; }
template <bool CP> __device__ __forceinline__ float g_w_t(const Graph& g, int a) { if constexpr (CP) return (float)g.w16[a]; else return g.weight[a]; }

// state block of one utterance (HBM), carved by layout(): header words then arrays
struct Hdr {
  int n_frames;        // decoded frames (emitting steps taken)
  int n_tok;           // tokens so far (all frames)
  int n_link;          // links so far
  int overflow;        // capacity exhausted (bit 0 tokens, 1 links, 2 hash slots, 3 frames): results invalid
  int num_input;       // input frames seen (incl. skipped ones)
  int is_last_blank, last_best;
  int finalized;
  float final_best;    // best (cost + final cost) on the last frame
  int has_final;
  unsigned arcs_lo, arcs_hi;   // emitting arcs expanded so far (64-bit): 16 B of graph each, the algorithmic traffic of the search
  int links_marked;    // links [0, links_marked) survived the last PruneActiveTokens pass (link_alive valid, all 1)
  int n_prunes;        // PruneActiveTokens passes so far
  int peak_tok, peak_link;   // high-water marks of n_tok / n_link (before the passes compacted them)
  int removed_tok, removed_link;   // what the PruneActiveTokens passes removed so far (created = held + removed)
};

// Scratch of the CLUSTER search (several workgroups per utterance, wfst_cluster_kernel below): every word is written with L2
// atomics or plain stores and read with L1-bypassing (sc1) loads by the workgroups of one cluster, which share an XCD's L2.
constexpr int WLG_CAP = 1 << 19;   // epsilon work list of a frame (tokens whose state has input-epsilon arcs; 125 k-word graphs put > 65 k of them into peak frames)
constexpr int HEAVY_CAP = 1 << 17; // heavy-token list of a frame: one 16-byte entry {token, its cost, first arc, end arc} per CHUNK of a heavy token's arcs (below)
constexpr int HEAVY_DEG = 32;
struct Clu {
  unsigned bar, bar_base; int pad0[62];          // cluster barrier: monotonic arrival counter, its value when the last launch ended
  // the counters the single-workgroup kernel keeps in LDS -- each on a 256-byte block of its own: they take ~2500 atomics per
  // frame between them (one per wave and trip), and atomics on words of one cache line are served one after the other
  // (all four in one line: 14.8 ms for the 32-utterance search; apart: 13.5)
  int n_tok, padt[63];
  int n_link, padl[63];
  int wl_n, padw[63];
  int overflow, pado[63];
  unsigned best[2], cand_min[2]; int narcs[2];   // per frame parity: cheapest token of the frame, cheapest candidate, arcs walked
  int changed[8];                                // per closure round (mod 8): a cost went down
  int xcc[32];                                   // XCC_ID each member saw (placement check; up to 32 members: a whole XCD)
  int n_heavy, pad1[63];                         // chunks of the frame's tokens with more than HEAVY_DEG emitting arcs (word-boundary states)
  int hist[2][4][256];                           // radix-select histograms: [max_active / min_active][round][digit]
};

struct Lay {
  Hdr* h; float* last_prob; int* mapping; int* tok_off; int* link_off; float* cost_offset;
  int* tok_state; unsigned* tok_cost; long long* tok_best; unsigned* tok_extra; unsigned* tok_prev;   // tok_best: {best link (high word), its source token}
  int* link_src; int* link_dst; int* link_arc; float* link_ac; float* link_graph; unsigned char* link_alive;
  int* gkey; int* gidx;
  Clu* clu; int* wlg; int* gkey2; int* gidx2; unsigned long long* heavy;   // heavy: 2 words per entry
};

__host__ __device__ inline size_t al(size_t v) { return (v + 255) / 256 * 256; }

__host__ __device__ __forceinline__ size_t layout(char* base, int max_frames, int max_tok, int max_link, int hash, Lay* l) {
  size_t o = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + o : nullptr; o += al(bytes); return p; };
  Hdr* h = reinterpret_cast<Hdr*>(take(sizeof(Hdr)));
  float* lp = reinterpret_cast<float*>(take(sizeof(float) * MAX_C));
  int* mp = reinterpret_cast<int*>(take(sizeof(int) * (max_frames + 1)));
  int* to = reinterpret_cast<int*>(take(sizeof(int) * (max_frames + 3)));
  int* lo = reinterpret_cast<int*>(take(sizeof(int) * 2 * (max_frames + 3)));
  float* co = reinterpret_cast<float*>(take(sizeof(float) * (max_frames + 1)));
  int* ts = reinterpret_cast<int*>(take(sizeof(int) * max_tok));
  unsigned* tc = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * max_tok));
  long long* tb = reinterpret_cast<long long*>(take(sizeof(long long) * max_tok));
  unsigned* te = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * max_tok));
  unsigned* tp = reinterpret_cast<unsigned*>(take(sizeof(unsigned) * max_tok));
  int* ls = reinterpret_cast<int*>(take(sizeof(int) * max_link));
  int* ld = reinterpret_cast<int*>(take(sizeof(int) * max_link));
  int* la = reinterpret_cast<int*>(take(sizeof(int) * max_link));
  float* lac = reinterpret_cast<float*>(take(sizeof(float) * max_link));
  float* lg = reinterpret_cast<float*>(take(sizeof(float) * max_link));
  unsigned char* lv = reinterpret_cast<unsigned char*>(take(max_link));
  int* gk = reinterpret_cast<int*>(take(sizeof(int) * hash));
  int* gi = reinterpret_cast<int*>(take(sizeof(int) * hash));
  Clu* cl = reinterpret_cast<Clu*>(take(sizeof(Clu)));
  int* wg = reinterpret_cast<int*>(take(sizeof(int) * WLG_CAP));
  int* gk2 = reinterpret_cast<int*>(take(sizeof(int) * hash));
  int* gi2 = reinterpret_cast<int*>(take(sizeof(int) * hash));
  unsigned long long* hv = reinterpret_cast<unsigned long long*>(take(sizeof(unsigned long long) * 2 * HEAVY_CAP));
  if (l) *l = Lay{h, lp, mp, to, lo, co, ts, tc, tb, te, tp, ls, ld, la, lac, lg, lv, gk, gi, cl, wg, gk2, gi2, hv};
  return o;
}

// order-preserving float <-> unsigned (atomicMin on costs)
__device__ __forceinline__ unsigned f2o(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float o2f(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// A token's backpointer: the cheapest-arriving link with the smallest index (best_links' rule) AND that link's source token, one
// 8-byte word {link (high, signed), source token (low)} so that the best-path walk is ONE dependent load per hop; atomicMin on
// the word orders by link.  -1 = the start token, BEST_UNSET = not computed yet.
constexpr long long BEST_UNSET = 0x7fffffffffffffffLL;
__device__ __forceinline__ long long best_word(int li, int src) { return ((long long)li << 32) | (long long)(unsigned)src; }

struct Opts {
  float beam, lattice_beam, beam_delta, acoustic_scale, length_penalty, blank_skip_thresh;
  int max_active, min_active;
};

// ---- extra costs (PruneForwardLinks, lattice-faster-decoder.cc:297-374)
constexpr unsigned INF_BITS = 0x7f800000u;   // +inf: a token that has left the lattice
// The link's extra cost: the destination's extra cost + what the path through this link costs more than the destination's best.
// fp32: THIS parenthesisation is the result (every pruning kernel must agree bit for bit on which links survive).
__device__ __forceinline__ float link_extra(float xd, float cs, float ac, float gr, float cd) { return xd + ((cs + ac + gr) - cd); }
// ... with the link's costs and its tokens' costs read from the state block (xd: the destination's extra cost, as the caller read it)
__device__ __forceinline__ float link_extra_at(const Lay l, int li, int src, int dst, float xd) {
  return link_extra(xd, o2f(l.tok_cost[src]), l.link_ac[li], l.link_graph[li], o2f(l.tok_cost[dst]));
}
// ... with the destination frame's costs (cB) and extra costs (xB) staged in LDS; d: the destination's index in its frame
__device__ __forceinline__ float link_extra_lds(const unsigned* xB, const unsigned* cB, int d, unsigned cs, float ac, float gr) {
  return link_extra(__uint_as_float(xB[d]), o2f(cs), ac, gr, o2f(cB[d]));
}
// what a surviving link hands to its source: never below 0; as bits (non-negative floats order like unsigned: atomicMin)
__device__ __forceinline__ unsigned extra_bits(float lec) { if (lec < 0.f) lec = 0.f; return __float_as_uint(lec); }
// did an extra cost move by more than delta (the reference's extra_costs_changed, :528-531)?
__device__ __forceinline__ bool extra_moved(unsigned nv, unsigned ov, float delta) {
  return nv != ov && (nv == INF_BITS || ov == INF_BITS || fabsf(__uint_as_float(nv) - __uint_as_float(ov)) > delta);
}

// Block reductions: within a wave through lane permutes, across the NT / 64 waves through LDS (red: NT / 64 words) -- two
// barriers instead of the 2 log2(NT) of a tree over the whole block (a frame makes several of them on its serial path).
__device__ __forceinline__ float block_min(float* red, float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) r = fminf(r, red[w]);
  __syncthreads();
  return r;
}
__device__ __forceinline__ int block_sum(int* red, int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = red[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) r += red[w];
  __syncthreads();
  return r;
}

// a load that is L1-bypassing (L2 = true: another workgroup of the cluster may have written the word) or plain
template <bool L2, typename T> __device__ __forceinline__ T ldt(const T* p) {
  if constexpr (L2) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); else return *p;
}

// Radix select (std::nth_element's value over ordered cost keys): four rounds of 8 bits from the top -- a 256-bin histogram per
// round, the bin that holds rank k found by wave 0 with a lane prefix sum -- instead of a 32-step bisection with a pass over the
// tokens and a block reduction per step.  The two halves of a round; kth_cost (wfst.hip) and ckth_cost (wfst_cluster.hip) chain them.
// radix_count: this workgroup's histogram (LDS, [256]) of digit `round` over keys[first + threadIdx.x .. t1) in steps of
// `stride` that match `prefix` in the digits above; ends with a barrier.
template <bool L2>   // L2: the keys may have been written by another workgroup of the cluster
__device__ __forceinline__ void radix_count(int* hist, const unsigned* keys, int first, int t1, int stride, int round, unsigned prefix) {
  const int shift = 24 - 8 * round;
  if (threadIdx.x < 256) hist[threadIdx.x] = 0;
  __syncthreads();
  for (int tb = first; tb < t1; tb += stride) {
    const int t = tb + (int)threadIdx.x;
    const unsigned key = t < t1 ? ldt<L2>(&keys[t]) : 0u;
    const bool act = t < t1 && (round == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8)));
    const int d = (int)((key >> shift) & 255u);
    if (round < 2) {
      // the costs of a frame lie within a beam of each other: their top bits fall into a handful of bins, so the lanes
      // of a wave that share a digit send ONE LDS atomic
      unsigned long long todo = __ballot(act);
      while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int dl = __shfl(d, leader);
        const unsigned long long peers = __ballot(act && d == dl);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[dl], __popcll(peers));
        todo &= ~peers;
      }
    } else if (act) {
      atomicAdd(&hist[d], 1);
    }
  }
  __syncthreads();
}
// radix_pick: wave 0 finds the bin that holds `rank` among the 256 counts bins[i]: res[0] = the digit, res[1] = the rank
// inside that bin; ends with a barrier.
template <bool L2>   // L2: the counts are the cluster's, summed in L2
__device__ __forceinline__ void radix_pick(int* res, int rank, const int* bins) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int h0 = ldt<L2>(bins + 4 * lane), h1 = ldt<L2>(bins + 4 * lane + 1), h2 = ldt<L2>(bins + 4 * lane + 2), h3 = ldt<L2>(bins + 4 * lane + 3);
    const int mine = h0 + h1 + h2 + h3;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int up = __shfl_up(incl, o); if (lane >= o) incl += up; }
    const int excl = incl - mine;
    if (rank >= excl && rank < incl) {      // exactly one lane (0 <= rank < number of candidates)
      int r = rank - excl, d = 4 * lane;
      if (r >= h0) { r -= h0; ++d; if (r >= h1) { r -= h1; ++d; if (r >= h2) { r -= h2; ++d; } } }
      res[0] = d; res[1] = r;
    }
  }
  __syncthreads();
}

// Exclusive positions of 4 flags per thread (element e_k = base + k * NT + tid: coalesced) + the chunk's total: wave scans + the
// 4 x 16 wave totals read by everyone from a double-buffered LDS table (wtot, flip) -- ONE barrier per chunk, which also
// separates the chunk's reads from its writes.
__device__ __forceinline__ void scan4(int (*wtot)[4][NT / 64], int& flip, const int (&fl)[4], int (&pos)[4], int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int incl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int v = fl[k];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int x = __shfl_up(v, off, 64); if (lane >= off) v += x; }
    incl[k] = v;
    if (lane == 63) wtot[flip][k][w] = v;
  }
  __syncthreads();
  int run = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int before = 0, row = 0;
    for (int ww = 0; ww < NT / 64; ++ww) { const int v = wtot[flip][k][ww]; if (ww < w) before += v; row += v; }
    pos[k] = run + before + incl[k] - fl[k];
    run += row;
  }
  total = run;
  flip ^= 1;
}

__device__ __forceinline__ unsigned xcc_of() { unsigned x; asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x)); return x & 0xf; }
__device__ __forceinline__ unsigned hash_of(int state, int mask) { return ((unsigned)state * 2654435761u) & (unsigned)mask; }

// ---- the cluster (G workgroups per utterance behind one XCD's L2: wfst_cluster.hip has the whole story)
constexpr int UNSET = -2;                        // a hash slot's id half while the claim's winner is still writing the token
constexpr unsigned CBAR_SPIN_LIMIT = 1u << 22;

__device__ __forceinline__ int ldi(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ldu(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ldub(const unsigned char* p) { return (unsigned)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The backpointer rule (best_links): among the links into a token, the first (smallest index) whose cost equals the token's
// final cost.  One link src -> dst; atomicMin on the {link, source} word orders by link.
template <bool L2> __device__ __forceinline__ void best_link(const Lay l, int li, int src, int dst) {
  const float tot = o2f(ldt<L2>(&l.tok_cost[src])) + ldt<L2>(&l.link_ac[li]) + ldt<L2>(&l.link_graph[li]);
  if (f2o(tot) == ldt<L2>(&l.tok_cost[dst])) atomicMin(&l.tok_best[dst], best_word(li, src));
}

// The blank-skipping decision of CtcWfstBeamSearch::Search (ctc_wfst_beam_search.cc:70-121) for one row of log-probs:
// 0 = a blank frame: skip it (the caller remembers it), 1 = decode it, 2 = re-insert the remembered blank frame first.
// last_best is updated by every non-blank frame.
__device__ __forceinline__ int frame_mode(const float* row, int C, float thresh, int is_last_blank, int& last_best) {
  if (expf(row[0]) > thresh) return 0;
  int cur_best = 0; float bv = row[0];
  for (int k = 1; k < C; ++k) if (row[k] > bv) { bv = row[k]; cur_best = k; }
  const int mode = (cur_best != 0 && is_last_blank && cur_best == last_best) ? 2 : 1;
  last_best = cur_best;
  return mode;
}

struct CCtx {
#ifdef B2T_WFST_TIMING
  unsigned long long tacc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, tprev = 0;
#endif
  Graph g; Lay l; Opts o; Clu* cl;
  int max_frames, max_tok, max_link, hash;
  int G, u, j, gtid, gthreads;                   // cluster size, utterance, member, thread of the cluster, threads of the cluster
  unsigned bar_target;
  float* ll; float* redf; int* redi; int* lsh;   // LDS: frame log-likelihoods, reduction scratch, [0] dead flag, [1..] scalars
  int* key;                                      // hash of the frame being built (8-byte slots {key, token id})
  // Frame-stamped slots (round 4): the key half of a slot is stamp << 27 | state, a slot whose stamp is not the current frame's
  // reads as empty -- no hash is cleared per frame any more (0.42 GB of the 1.13 GB a 25-frame launch of 32 utterances wrote).
  // Stamps 1 .. 30 cycle over a hash's uses (0 = zeroed memory, 31 = cleared marker: never live), so a hash is cleared once per
  // 30 uses.  Needs states < 2^27; larger graphs (stamped = 0) clear per frame as before.
  unsigned stamp;
  int* stk_t; float* stk_c;                      // LDS: per-thread stack of the epsilon closure's chase ([CHASE_DEPTH][NT])
};

// Cluster barrier.  Every store this workgroup issued has reached L2 (vmcnt(0): stores are acknowledged by L2) before its
// arrival is counted; readers use sc1 loads, so nothing has to be invalidated.  Returns false after a timeout (a member is
// not resident or died): the overflow word gets bit 32 and every member leaves at its next barrier.
[[maybe_unused]] __device__ bool cbar(CCtx& c) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  c.bar_target += (unsigned)c.G;
  if (threadIdx.x == 0 && !c.lsh[0]) {
    __hip_atomic_fetch_add(&c.cl->bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while ((int)(ldu(&c.cl->bar) - c.bar_target) < 0) {
      if (++spins > CBAR_SPIN_LIMIT || ((spins & 1023u) == 0u && (ldi(&c.cl->overflow) & 32))) { atomicOr(&c.cl->overflow, 32); c.lsh[0] = 1; break; }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __syncthreads();
  return c.lsh[0] == 0;
}

// One slot per ACTIVE lane from a shared counter with ONE atomic per wave: a counter word in L2 serves ~90 atomics per
// microsecond, and a frame allocates ~50 k links and ~8 k tokens (one atomic each: 60 ms of the first version's 72).
__device__ __forceinline__ int wave_alloc(int* counter) {
  const unsigned long long m = __ballot(1);
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader, 64);
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

// What every cluster kernel starts with: block -> (utterance u, member j), the context, the dead flag and scalars zeroed (the
// caller's next __syncthreads publishes them), the barrier target where the previous launch left it (written before that
// launch ended: kernel boundary, visible).  Blocks beyond the last utterance (c.u >= U) touch nothing and must return at once.
// block b = (k / 8) * 8G + j * 8 + (k % 8): the G members of cluster (utterance) k all have b % 8 == k % 8, i.e. one XCD
__device__ __forceinline__ CCtx cluster_ctx(const Graph g, const Opts o, char* state, size_t state_bytes, int max_frames, int max_tok,
                                            int max_link, int hash, int G, int U, int* lsh) {
  CCtx c;
  const int b = blockIdx.x, grp = b / (8 * G), r = b % (8 * G);
  c.j = r / 8; c.u = grp * 8 + (r % 8);
  c.g = g; c.o = o; c.max_frames = max_frames; c.max_tok = max_tok; c.max_link = max_link; c.hash = hash;
  char* const base = state + (size_t)c.u * state_bytes;
  // layout() carves from a null base too (the host's size query) and so selects between null and the address for every array
  // pointer; not here: every entry point that launches a cluster kernel has refused a null `state` in check_args
  __builtin_assume(base != nullptr);
  layout(base, max_frames, max_tok, max_link, hash, &c.l);
  c.cl = c.l.clu; c.G = G; c.gtid = c.j * NT + (int)threadIdx.x; c.gthreads = G * NT;
  c.ll = nullptr; c.redf = nullptr; c.redi = nullptr; c.lsh = lsh; c.stk_t = nullptr; c.stk_c = nullptr;
  c.key = c.l.gkey; c.stamp = 0u;
  if (threadIdx.x < 8) lsh[threadIdx.x] = 0;
  c.bar_target = c.u < U ? c.cl->bar_base : 0u;
  return c;
}
// ... and ends with (one thread of the cluster): the overflow word back into the header, the barrier count for the next launch
__device__ __forceinline__ void cluster_leave(const CCtx& c, Hdr* h) {
  h->overflow = ldi(&c.cl->overflow);
  c.cl->bar_base = c.bar_target;
}

// ---- host side
[[maybe_unused]] int check_args(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, int U, const char* what) {
  B2T_REQUIRE(g && o && state && U > 0, "%s: null argument", what);
  B2T_REQUIRE(g->row && g->next && g->n_eps && g->final_cost && g->n_states > 0 &&
              (g->compact ? (g->labels && g->weight_f16) : (g->ilabel && g->olabel && g->weight)), "%s: incomplete graph", what);
  B2T_REQUIRE(o->hash_size >= 64 && (o->hash_size & (o->hash_size - 1)) == 0, "%s: hash_size must be a power of two >= 64", what);
  B2T_REQUIRE(o->max_frames > 0 && o->max_tokens > 0 && o->max_links > 0, "%s: bad capacities", what);
  B2T_REQUIRE(o->beam > 0.f && o->lattice_beam > 0.f && o->max_active > 1 && o->min_active >= 0 && o->min_active <= o->max_active,
              "%s: bad search options", what);
  return 0;
}
[[maybe_unused]] Graph to_graph(const b2t_wfst_graph_t* g) {
  return Graph{g->row, g->ilabel, g->olabel, g->weight, g->next, g->n_eps, g->final_cost, g->start,
               g->labels, reinterpret_cast<const _Float16*>(g->weight_f16), g->compact};
}
[[maybe_unused]] Opts to_opts(const b2t_wfst_opts_t* o) {
  return Opts{o->beam, o->lattice_beam, o->beam_delta, o->acoustic_scale, o->length_penalty, o->blank_skip_thresh, o->max_active, o->min_active};
}
template <typename K> void allow_lds(K kernel, size_t bytes) {
  if (bytes > 48 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
[[maybe_unused]] size_t state_bytes(const b2t_wfst_opts_t* o) { return layout(nullptr, o->max_frames, o->max_tokens, o->max_links, o->hash_size, nullptr); }
// a cluster launch: utterances in groups of 8 (one per XCD), G consecutive blocks of 8 per group
[[maybe_unused]] int cluster_grid(int U, int G) { return (U + 7) / 8 * 8 * G; }
}  // namespace

// wfst_cluster.hip: the cluster search over rows [0, lens[u]) of logp[u], G workgroups per utterance (arguments checked by the caller)
int wfst_cluster_search(const b2t_wfst_graph_t* g, const b2t_wfst_opts_t* o, void* state, const float* logp, const int32_t* lens,
                        int U, int T, int C, int G, hipStream_t stream);

}  // namespace b2t
