// exec.cpp — the model pass (GRUDecoder.forward, model_training/rnn_model.py:88-134, and its backward, rnn_trainer.py:547)
// issued from C++: every GEMM / sweep / reduction launch and every stream-event edge of the pipelined execution plan
// comes from here, so that one pass is ONE call across the C ABI instead of ~250 ctypes calls.
//
// Execution plan.  A GRU layer is a strictly serial chain over time and one layer's persistent sweep keeps only
// (H/16) x ceil(B/16) workgroups busy, each mostly waiting on the inter-workgroup hand-off.  The time axis is cut into
// chunks and the layers are software-pipelined over them: while layer l sweeps chunk c, layer l+1 runs its
// input-projection GEMM + sweep on chunk c-1; in the backward pass the weight-gradient GEMMs of layer l run while the
// layers below are still sweeping.  The pass is built as a task graph and list-scheduled onto FOUR in-order queues (the
// caller's stream + three workers on different command-processor pipes, see run_plan / choose_workers); dependencies
// that cross queues are HIP events; the caller's stream joins the workers before the function returns (nothing
// synchronises with the host).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <functional>
#include <atomic>
#include <chrono>
#include <vector>
#include <queue>
#include <algorithm>
#include <unordered_map>
#include <unordered_set>
#include "common.h"
#include "gru_cell.h"
#include "gemm_args.h"

namespace b2t {
namespace {

constexpr int MAXL = B2T_MAX_LAYERS;
constexpr int MAXC = 32;   // time chunks
constexpr int NPACK = 4;   // queues with a pack scratch of their own (caller's stream + 3 workers)

struct ProfRec { int kind; double flops; hipEvent_t e0, e1; };

}  // namespace
}  // namespace b2t

struct b2t_exec {
  int L = 0;
  std::vector<hipStream_t> phys;                    // worker queues (the caller's stream is queue 0 of a pass)
  int n_workers = 3;
  bool have_workers = false;
  hipStream_t workers_for = nullptr;                // the caller's stream the workers were chosen against
  float* scratch = nullptr;                         // 256 bytes of device memory for the calibration launches
  unsigned sweep_qmask = 0;                         // queues a sweep may be scheduled on
  std::vector<hipEvent_t> pool;   // ordering events (timing disabled), handed out round-robin within a pass
  size_t next_ev = 0;
  bool profile = false;
  std::vector<b2t::ProfRec> recs;
  std::vector<hipEvent_t> tpool;  // timing events
  size_t next_tev = 0;
  // Replayable passes (B2T_EXEC_GRAPH=1): a pass whose every argument repeats is built ONCE as a hipGraph from the plan's task
  // graph -- each task captured alone on a stream of its own into a child graph, the plan's edges as the graph's -- and replayed
  // with one hipGraphLaunch (run_plan_graph below).
  std::unordered_map<uint64_t, hipGraphExec_t> graphs;
  std::unordered_set<uint64_t> seen_keys;           // a key's first pass runs eagerly (lazy one-time initialisations happen there)
  hipStream_t cap[8] = {};                          // capture streams, one per queue of the plan
  bool graph_failed = false;
  long long graph_replays = 0, graph_builds = 0;
};

namespace b2t {
namespace {

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int out_T(const b2t_model_t* m, int T) { return m->patch > 0 ? (T - m->patch) / m->stride + 1 : T; }
int in0(const b2t_model_t* m) { return m->patch > 0 ? m->F * m->patch : m->F; }

// Number of K slices so that a weight-gradient GEMM (few 128x128 output tiles, very long K) fills the chip with ONE wave of
// resident workgroups (each slice at least 256 deep): 3 per CU for the fp32 tile kernel (768 blocks; C2 step 19.49 ms
// against 19.56 with 1024 and 19.72 with 512), 2 per CU for the packed bf16 kernel (512; C2 bf16 10.64 against 10.78 / 10.88).
// More slices only add slab traffic (the slabs are written and read once more by the reduction).
int splitk_target(bool bf16) {
  static const int env = getenv("B2T_SPLITK_TARGET") ? std::max(1, atoi(getenv("B2T_SPLITK_TARGET"))) : 0;
  return env ? env : (bf16 ? 512 : 768);
}
int splitk_for(int M, int N, long long K, int target_blocks) {
  const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
  long long v = std::min<long long>(target_blocks / std::max(1, tiles), K / 256);
  // multiples of 8 slices let the GEMM keep each slice on one XCD (gemm.hip: ks_xcd)
  if (v >= 8) v = v / 8 * 8;   // (rounding 7 up to 8 was measured at H = 768: 19.03 -> 19.31 ms, more than one wave of blocks)
  return (int)std::max<long long>(1, v);
}
int splitk_cap(int M, int N, long long K) {   // workspace sizing
  return std::max(splitk_for(M, N, K, splitk_target(false)), splitk_for(M, N, K, splitk_target(true)));
}

// Time chunks of the layer pipeline: `chunks` equal parts (at least 16 steps each).
int make_chunks(int Tp, int chunks, int (*out)[2]) {
  int n = std::max(1, std::min(std::min(chunks, MAXC), Tp / 16));
  const int ch = (Tp + n - 1) / n;
  int k = 0;
  for (int t0 = 0; t0 < Tp; t0 += ch) { out[k][0] = t0; out[k][1] = std::min(Tp, t0 + ch); ++k; }
  return k;
}

int chunk_len(int Tp, int chunks) {     // length of the longest chunk make_chunks cuts
  const int n = std::max(1, std::min(std::min(chunks, MAXC), Tp / 16));
  return (Tp + n - 1) / n;
}

// ---- workspace layout (deterministic in (model, pass): forward and backward carve the same addresses) --------------
struct Layout {
  float *U, *Ud, *out[MAXL], *outd[MAXL], *gi[MAXL], *res[MAXL], *slab_gi[MAXL];
  float *dY[MAXL], *dG[MAXL], *dh_init, *carry[MAXL], *scratch[MAXL], *whh_t[MAXL], *dU, *dV, *day_slab, *day_bslab;
  float *slab[MAXL], *slab_head, *s4[MAXL], *cs_layer[MAXL], *asum[MAXL], *cs_head, *cs_day, *cs_h0, *slab_dx;
  char* pack[NPACK];       // amp mode: per-queue scratch of the two-pass bf16 GEMM (packed operands)
  size_t pack_bytes;
  char *wpk_f[MAXL], *wpk_b[MAXL];   // amp mode: W_ih of every layer packed once per pass -- as the projection's B operand (forward), as the input gradient's (backward)
  float *slab_hh[MAXL], *asum_hh[MAXL];   // amp mode: split-K slab / per-slice sums of dW_hh when it runs as a task of its own next to dW_ih
  char* xpk_day;                     // amp mode: the A operands of the day layer's per-sentence weight gradients (x[b]^T, Z = B), packed when the backward pass starts
  char *xpk_hh[MAXL], *xpk_ih[MAXL]; // amp mode: the B operands of a layer's whole-sequence weight-gradient GEMMs (h_{t-1}^T, x^T: known when the backward pass starts), packed ahead of the tail
  // layer wavefront (round 6, gru_wave.hip): counters + hand-off rings of the forward / backward launch, W_ih^T of the layers >= 1
  unsigned *wv_cnt_f, *wv_cnt_b;
  char *wv_ring_f[MAXL], *wv_ringd_f[MAXL], *wv_ring_b[MAXL], *wv_ringx_b[MAXL];
  float* wih_t[MAXL];
  size_t bytes;
};

// The pass runs its sweeps as the layer wavefront: asked for by the caller (B2T_GRU_WAVE on a persistent bf16 sweep mode in the bf16
// GEMM regime) and a shape the kernels hold (all L x H / 16 workgroups resident).  Decided the same way by carve and by both passes.
bool wave_pass(const b2t_model_t* m, const b2t_pass_t* p, int mode) {
  const int Tp = m->patch > 0 ? (p->T - m->patch) / m->stride + 1 : p->T;
  if (Tp < 1) return false;
  return (mode & B2T_GRU_WAVE) && (mode & 0xff) == 1 && (mode & B2T_GRU_BF16) && p->bf16_gemm && gru_wave_ok(m->L, std::min(Tp, 4096), p->B, m->H, nullptr);
}

size_t colsum_ws_floats(long long rows, int cols) { return b2t_colsum_ws_bytes(rows, cols) / sizeof(float); }

void carve(const b2t_model_t* m, const b2t_pass_t* p, char* base, Layout& w) {
  const size_t B = p->B, T = p->T, F = m->F, H = m->H, L = m->L, C = m->C;
  const size_t Tp = out_T(m, p->T), In0 = in0(m);
  size_t off = 0;
  auto take = [&](size_t nfloats) {
    float* r = reinterpret_cast<float*>(base + off);
    off += align_up(nfloats * sizeof(float), 256);
    return r;
  };
  w.U = take(B * T * F);
  w.Ud = p->in_drop > 0.f ? take(B * T * F) : w.U;
  for (size_t l = 0; l < L; ++l) {
    w.out[l] = take((Tp + 1) * B * H);
    w.outd[l] = (p->rnn_drop > 0.f && l + 1 < L) ? take((Tp + 1) * B * H) : w.out[l];
    w.gi[l] = take(Tp * B * 3 * H);
  }
  // split-K slabs of the streaming-sized input projections (chunks of n*B <= 512 rows, see b2t_model_forward)
  for (size_t l = 0; l < L; ++l) {
    const size_t sk = l == 0 ? (In0 >= 2048 ? std::max<size_t>(1, std::min<size_t>(16, In0 / 448)) : 0)
                             : (H >= 384 ? std::max<size_t>(1, H / 192) : 0);
    // (layer 0 with a patch input, K = In0 >= 2048, also splits K three ways at full size: see b2t_model_forward)
    const size_t big0 = (l == 0 && In0 >= 2048 && !p->bf16_gemm) ? 3 * Tp * B * 3 * H : 0;
    w.slab_gi[l] = sk > 1 ? take(std::max(sk * std::min<size_t>(512, Tp * B) * 3 * H, big0)) : nullptr;
  }
  // amp mode: packed-operand scratch, sized for the largest GEMM of either pass, one per queue
  w.pack_bytes = 0;
  for (int q = 0; q < NPACK; ++q) w.pack[q] = nullptr;
  if (p->bf16_gemm) {
    const int R = (int)(Tp * B);
    const int shapes[][3] = {{R, (int)(3 * H), (int)In0}, {R, (int)(3 * H), (int)H}, {R, (int)C, (int)H}, {R, (int)In0, (int)(3 * H)},
                             {R, (int)H, (int)(3 * H)}, {(int)(3 * H), (int)H, R}, {(int)(3 * H), (int)In0, R}, {(int)C, (int)H, R}, {R, (int)H, (int)C}};
    for (const auto& sh : shapes) w.pack_bytes = std::max(w.pack_bytes, b2t_gemm_bf16p_ws_bytes(sh[0], sh[1], sh[2]));
    // the day layer's per-sentence products (Z = B): forward x[b] W[day[b]], backward x[b]^T dpre[b]
    w.pack_bytes = std::max(w.pack_bytes, b2t_gemm_bf16p_ws_bytes_z((int)T, (int)F, (int)F, (int)B));
    if (p->save) w.pack_bytes = std::max(w.pack_bytes, b2t_gemm_bf16p_ws_bytes_z((int)F, (int)F, (int)T, (int)B));
    w.pack_bytes = align_up(w.pack_bytes, 256);
    for (int q = 0; q < NPACK; ++q) { w.pack[q] = base + off; off += w.pack_bytes; }
  }
  for (size_t l = 0; l < MAXL; ++l) { w.wv_ring_f[l] = w.wv_ringd_f[l] = w.wv_ring_b[l] = w.wv_ringx_b[l] = nullptr; w.wih_t[l] = nullptr; }
  w.wv_cnt_f = w.wv_cnt_b = nullptr;
  if (wave_pass(m, p, p->fwd_mode)) {
    const int Tc = chunk_len((int)Tp, p->chunks);     // a launch per time chunk: rings and counters hold one chunk
    w.wv_cnt_f = reinterpret_cast<unsigned*>(base + off); off += align_up(gru_wave_cnt_words_fwd((int)L, Tc, (int)B) * sizeof(unsigned), 256);
    const size_t rb = align_up(gru_wave_ring_bytes_fwd(Tc, (int)B, (int)H), 256);
    const bool drop = p->rnn_drop > 0.f && L > 1;
    for (size_t l = 0; l < L; ++l) { w.wv_ring_f[l] = base + off; off += rb; w.wv_ringd_f[l] = w.wv_ring_f[l]; }
    // the ring the layer above reads when it is not the own-recurrence ring: the dropped states, or the written-through copy of the local form
    if (drop || gru_wave_local((int)L, (int)H)) for (size_t l = 0; l + 1 < L; ++l) { w.wv_ringd_f[l] = base + off; off += rb; }
  }
  for (size_t l = 0; l < MAXL; ++l) w.wpk_f[l] = w.wpk_b[l] = nullptr;
  if (p->bf16_gemm)
    for (size_t l = 0; l < L; ++l) { w.wpk_f[l] = base + off; off += align_up(gemm_bf16p_operand_bytes((int)(3 * H), (int)(l == 0 ? In0 : H)), 256); }
  if (!p->save) { w.xpk_day = nullptr; w.bytes = off; return; }
  for (size_t l = 0; l < MAXL; ++l) { w.xpk_hh[l] = w.xpk_ih[l] = nullptr; w.slab_hh[l] = w.asum_hh[l] = nullptr; }
  w.xpk_day = nullptr;
  if (p->bf16_gemm) { w.xpk_day = base + off; off += align_up(B * gemm_bf16p_operand_bytes((int)F, (int)T), 256); }
  if (p->bf16_gemm)
    for (size_t l = 0; l < L; ++l) {
      w.wpk_b[l] = base + off; off += align_up(gemm_bf16p_operand_bytes((int)(l == 0 ? In0 : H), (int)(3 * H)), 256);
      w.slab_hh[l] = take((size_t)splitk_cap(3 * H, H, Tp * B) * 3 * H * H);
      w.asum_hh[l] = take((std::max(std::min<size_t>(1024, Tp * B / 256), Tp * B / 64 + 1) + 8) * 3 * H);
      w.xpk_hh[l] = base + off; off += align_up(gemm_bf16p_operand_bytes((int)H, (int)(Tp * B)), 256);
      w.xpk_ih[l] = base + off; off += align_up(gemm_bf16p_operand_bytes((int)(l == 0 ? In0 : H), (int)(Tp * B)), 256);
    }
  for (size_t l = 0; l < L; ++l) w.res[l] = take(Tp * B * 4 * H);
  if (wave_pass(m, p, p->bwd_mode)) {
    const int Tc = (int)Tp;      // rings and counters hold the whole sequence (one chunk = one launch over all of it)
    w.wv_cnt_b = reinterpret_cast<unsigned*>(base + off); off += align_up(gru_wave_cnt_words_bwd((int)L, Tc, (int)B) * sizeof(unsigned), 256);
    const size_t rb = align_up(gru_wave_ring_bytes_bwd(Tc, (int)B, (int)H), 256);
    for (size_t l = 0; l < L; ++l) { w.wv_ring_b[l] = base + off; off += rb; w.wv_ringx_b[l] = w.wv_ring_b[l]; }
    if (gru_wave_local((int)L, (int)H)) for (size_t l = 1; l < L; ++l) { w.wv_ringx_b[l] = base + off; off += rb; }
    for (size_t l = 1; l < L; ++l) w.wih_t[l] = take(H * 3 * H);
  }
  const size_t K = Tp * B;
  for (size_t l = 0; l < L; ++l) {
    w.dY[l] = take(Tp * B * H);
    w.dG[l] = take(Tp * B * 4 * H);
    w.carry[l] = take(2 * B * H);
    w.scratch[l] = take(B * H);
    w.whh_t[l] = take(H * 3 * H);
    const size_t In = l == 0 ? In0 : H;
    const size_t a = (size_t)splitk_cap(3 * H, H, K) * 3 * H * H, b = (size_t)splitk_cap(3 * H, In, K) * 3 * H * In;
    const size_t b2 = (size_t)splitk_cap(2 * H, In, K) * 2 * H * In;   // the two-GEMM form of dW_ih (odd H)
    w.slab[l] = take(std::max(a, std::max(b, b2)));
    w.s4[l] = take(4 * H);
    w.cs_layer[l] = take(colsum_ws_floats(K, 4 * H) + 4);
    w.asum[l] = take((std::max(std::min<size_t>(1024, K / 256), K / 64 + 1) + 8) * 3 * H);   // per-slice column sums of dG out of the weight-gradient GEMMs + their reduction scratch
  }
  // two K slices for the input-gradient GEMMs of the serial plan (one at a time: one slab), see b2t_model_backward
  w.slab_dx = (!p->bf16_gemm && L > 1) ? take(2 * K * H) : nullptr;
  w.dh_init = take(L * B * H);
  w.dU = take(B * T * F);
  w.dV = m->patch > 0 ? take(B * Tp * In0) : nullptr;
  w.day_slab = take(B * F * F);
  w.day_bslab = take(B * align_up(F, 4));
  w.slab_head = take((size_t)splitk_cap(C, H, K) * C * H);
  w.cs_head = take(colsum_ws_floats(B * Tp, C) + 4);
  w.cs_day = take(B * colsum_ws_floats(T, F) + 4);
  w.cs_h0 = take(colsum_ws_floats(L * B, H) + 4);
  w.bytes = off;
}

// ---- pass context: streams, events, profiling ----------------------------------------------------------------------
constexpr int KSLOT = 4096;   // tile counters per split-K call site (slot = layer, MAXL = output layer)

struct Ctx {
  b2t_exec* ex;
  hipStream_t main;
  bool bf16_gemm;
  int rc = 0;
  hipStream_t qs[8] = {};      // the pass's queues (plan_queues); qs[0] = main
  bool exact_k = false;         // pipelined (chunked) passes: every GEMM keeps the tile kernel's k order, so that the result does not depend on the chunking
  int nq = 0;
  const Layout* lay = nullptr;  // for the per-queue pack scratch of the amp-mode GEMM
  unsigned* kcnt = nullptr;     // tile counters of the split-K GEMMs' in-kernel slab reduction (last block of sync_ws): KSLOT words per slot
  uint64_t gkey = 0;            // != 0: everything this pass launches is determined by this key (run_plan may replay it as a graph)

  // B2T_EXEC_HOST_DELAY_US=n (round 6): a busy wait of n microseconds in front of every runtime call the executor makes (launch, event
  // record, stream wait) -- emulates the pool's slow-host mode (host enqueue 5-8 ms per C2 step instead of 1.3) on a healthy box, to
  // find which call's host latency reaches the GPU timeline (tools/r6_hostdelay.sh, NOTES.md R6.1)
  // B2T_EXEC_HOST_TIMING=1: host time between consecutive runtime calls of the executor, attributed to the call that just returned
  // (kind 0 event record, 1 stream wait, 2 a launch inside gemm(), 3 any other launch): count, total and maximum per kind, printed
  // to stderr every 64 passes -- which CALLS take the time in a process whose enqueue is slow (NOTES.md R6.1)
  struct HostTiming { bool on; std::chrono::steady_clock::time_point last; double tot[4]; double mx[4]; long n[4]; long passes; };
  static HostTiming& ht() { static HostTiming h{getenv("B2T_EXEC_HOST_TIMING") != nullptr, std::chrono::steady_clock::now(), {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, 0}; return h; }
  static void ht_mark() { HostTiming& h = ht(); if (h.on) h.last = std::chrono::steady_clock::now(); }
  static void ht_point(int kind) {
    HostTiming& h = ht();
    if (!h.on) return;
    const auto now = std::chrono::steady_clock::now();
    const double us = std::chrono::duration<double, std::micro>(now - h.last).count();
    h.tot[kind] += us; h.mx[kind] = std::max(h.mx[kind], us); ++h.n[kind]; h.last = now;
  }
  static void ht_pass() {
    HostTiming& h = ht();
    if (!h.on || (++h.passes % 64) != 0) return;
    static const char* nm[4] = {"event_record", "stream_wait", "gemm_launch", "other_launch"};
    fprintf(stderr, "[exec host timing] after %ld passes:", h.passes);
    for (int k = 0; k < 4; ++k) fprintf(stderr, " %s n=%ld mean=%.1fus max=%.0fus total/pass=%.2fms;", nm[k], h.n[k], h.n[k] ? h.tot[k] / h.n[k] : 0.0, h.mx[k], h.tot[k] / h.passes * 1e-3);
    fprintf(stderr, "\n");
  }
  static void host_delay() {
    static const int us = getenv("B2T_EXEC_HOST_DELAY_US") ? atoi(getenv("B2T_EXEC_HOST_DELAY_US")) : 0;
    if (us <= 0) return;
    const auto t0 = std::chrono::steady_clock::now();
    while (std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() < 1000ll * us) {}
  }
  hipEvent_t record(hipStream_t s) {
    host_delay();
    if (ex->next_ev == ex->pool.size()) {
      hipEvent_t e;
      if (check_hip(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate")) { rc = 1; return nullptr; }
      ex->pool.push_back(e);
    }
    hipEvent_t e = ex->pool[ex->next_ev++];
    ht_mark();
    if (check_hip(hipEventRecord(e, s), "hipEventRecord")) rc = 1;
    ht_point(0);
    return e;
  }
  void wait(hipStream_t s, hipEvent_t e) {
    host_delay();
    ht_mark();
    if (e && check_hip(hipStreamWaitEvent(s, e, 0), "hipStreamWaitEvent")) rc = 1;
    ht_point(1);
  }
  hipEvent_t tev() {
    if (ex->next_tev == ex->tpool.size()) {
      hipEvent_t e;
      if (check_hip(hipEventCreate(&e), "hipEventCreate")) { rc = 1; return nullptr; }
      ex->tpool.push_back(e);
    }
    return ex->tpool[ex->next_tev++];
  }
  struct Scope {
    Ctx& c; hipStream_t s; int kind; double flops; hipEvent_t e0 = nullptr;
    Scope(Ctx& c_, hipStream_t s_, int kind_, double flops_) : c(c_), s(s_), kind(kind_), flops(flops_) {
      if (c.ex->profile) { e0 = c.tev(); if (e0) (void)hipEventRecord(e0, s); }
    }
    ~Scope() {
      if (c.ex->profile && e0) {
        hipEvent_t e1 = c.tev();
        if (e1) { (void)hipEventRecord(e1, s); c.ex->recs.push_back(ProfRec{kind, flops, e0, e1}); }
      }
    }
  };

  // C = A.B^T through b2t_gemm_f32 / b2t_gemm_bf16_f32.  splitk > 1: partial products go to `slab` ([splitk][M*N]) and
  // are summed deterministically into C by b2t_slab_reduce_f32 (weight gradients, K = T*B; streaming-sized projections).
  // Bp_pre: the B operand already packed for the two-pass bf16 kernel (the pass's weights, packed once: round 5); dropA: nn.GRU's
  // inter-layer dropout folded into the A pack.  Both only where would_pack(d, s) holds (the caller checks).
  void gemm(hipStream_t s, b2t_gemm_desc d, int splitk = 1, float* slab = nullptr, int accumulate = 0, int kslot = -1,
            const void* Bp_pre = nullptr, const PackDrop* dropA = nullptr, const void* Ap_pre = nullptr) {
    if (rc) return;
    host_delay();
    ht_mark();
    struct HtExit { ~HtExit() { Ctx::ht_point(2); } } ht_exit;
    if ((Bp_pre || dropA) && !(bf16_gemm && would_pack(d, s))) { set_error("exec: pre-packed operands need the two-pass bf16 GEMM"); rc = 2; return; }
    if (Ap_pre && !(bf16_gemm && would_pack_z(d, s))) { set_error("exec: a pre-packed Z-batched A needs the two-pass bf16 GEMM"); rc = 2; return; }
    void* st = reinterpret_cast<void*>(s);
    const int kind = (bf16_gemm ? 4 : 0) + (d.a_kcontig ? 2 : 0) + (d.b_kcontig ? 1 : 0);
    const double flops = 2.0 * d.M * d.N * (double)d.K * (d.Z > 0 ? d.Z : 1);
    if (d.Z <= 0) d.Z = 1;
    if (splitk > 1) {
      float* Cdst = d.C;
      if (d.Z != 1 || d.epilogue != 0 || d.c_div != 0 || d.c_s0 != d.N) {
        set_error("exec: split-K gemm supports Z=1, dense row-major C, no epilogue"); rc = 2; return;
      }
      d.C = slab; d.splitk = splitk; d.c_ks = (long long)d.M * d.N; d.accumulate = 0;
      // opt-in (B2T_FUSED_SLABS=1): the tile's last slice workgroup sums the slabs inside the GEMM (same order as the reduction
      // pass: bit-identical).  Measured slower than the separate pass: 19.64-19.71 vs 19.46-19.54 ms per C2 step -- 48 workgroups
      // re-read 50 MB of written-through slabs at the GEMM's tail where the reduction kernel uses the whole chip.
      static const bool want_fused = getenv("B2T_FUSED_SLABS") != nullptr;
      const int tiles = ((d.M + 127) / 128) * ((d.N + 127) / 128);
      const bool fused = want_fused && !bf16_gemm && kcnt && kslot >= 0 && tiles <= KSLOT && (d.N % 4) == 0 &&
                         ((uintptr_t)Cdst & 15) == 0 && (long long)d.M * d.N * 4 < (1ll << 31);
      if (fused) { d.ks_counters = kcnt + (size_t)kslot * KSLOT; d.ks_out = Cdst; d.ks_accumulate = accumulate; }
      {
        Scope sc(*this, s, kind, flops);
        rc = bf16_gemm ? gemm_amp(d, s, Bp_pre, dropA, Ap_pre) : b2t_gemm_f32(&d, st);
      }
      if (!rc && !fused) rc = b2t_slab_reduce_f32(slab, splitk, (long long)d.M * d.N, Cdst, accumulate, st);
      return;
    }
    d.accumulate = accumulate;
    if (exact_k && d.splitk <= 1) d.splitk = -1;
    Scope sc(*this, s, kind, flops);
    rc = bf16_gemm ? gemm_amp(d, s, Bp_pre, dropA, Ap_pre) : b2t_gemm_f32(&d, st);
  }
  // amp mode: the two-pass kernel (pack to dense bf16, then 128x128x64 tiles on packed operands: 2.5-3x the one-pass kernel)
  // for plain GEMMs big enough to pay for the pack passes, on a queue that has pack scratch; the one-pass kernel otherwise
  int pack_queue(hipStream_t s) const {
    int q = -1;
    for (int i = 0; i < nq && i < NPACK; ++i) if (qs[i] == s) q = i;
    if (nq == 0 && s == main) q = 0;
    return q;
  }
  bool pack_shape_ok(const b2t_gemm_desc& d) const {      // the part of would_pack that does not depend on the queue (plan-time decisions)
    return bf16_gemm && lay && lay->pack[0] && (d.Z == 1 || d.Z == 0) && !d.b_zmap && 2.0 * d.M * d.N * (double)d.K >= 2e9 &&
           b2t_gemm_bf16p_ws_bytes(d.M, d.N, d.K) <= lay->pack_bytes && (d.a_brk % 8) == 0;
  }
  // Z-batched products (the day layer; round 5): every matrix of the batch packed, then one launch over (tiles, Z)
  static bool z_pack_on() { const char* e = getenv("B2T_ZPACK"); return !e || atoi(e) != 0; }
  bool pack_shape_ok_z(const b2t_gemm_desc& d) const {    // plan time: the queue is not known yet (the first NPACK queues of a pass have pack scratch; call sites check would_pack_z on the queue)
    return bf16_gemm && lay && lay->pack[0] && d.Z > 1 && d.Z <= 65535 && d.splitk <= 1 && !d.a_sum && d.a_brk == 0 && z_pack_on() && d.M >= 192 &&
           2.0 * d.Z * d.M * d.N * (double)d.K >= 2e9 && b2t_gemm_bf16p_ws_bytes_z(d.M, d.N, d.K, d.Z) <= lay->pack_bytes;
  }
  bool would_pack_z(const b2t_gemm_desc& d, hipStream_t s) const {
    const int q = pack_queue(s);
    // (not the time-chunked day layer: 83-row chunks fill 65 % of a 128-row tile and every chunk would pack the weights again -- measured slower)
    return lay && q >= 0 && lay->pack[q] && d.Z > 1 && d.Z <= 65535 && d.splitk <= 1 && !d.a_sum && d.a_brk == 0 && z_pack_on() && d.M >= 192 &&
           2.0 * d.Z * d.M * d.N * (double)d.K >= 2e9 && b2t_gemm_bf16p_ws_bytes_z(d.M, d.N, d.K, d.Z) <= lay->pack_bytes;
  }
  bool would_pack(const b2t_gemm_desc& d, hipStream_t s) const {
    const int q = pack_queue(s);
    return lay && q >= 0 && lay->pack[q] && (d.Z == 1 || d.Z == 0) && !d.b_zmap && 2.0 * d.M * d.N * (double)d.K >= 2e9 &&
           b2t_gemm_bf16p_ws_bytes(d.M, d.N, d.K) <= lay->pack_bytes && (d.a_brk % 8) == 0;
  }
  int gemm_amp(const b2t_gemm_desc& d, hipStream_t s, const void* Bp_pre = nullptr, const PackDrop* dropA = nullptr, const void* Ap_pre = nullptr) {
    void* st = reinterpret_cast<void*>(s);
    if (would_pack_z(d, s)) return gemm_bf16p_run(&d, Ap_pre, nullptr, lay->pack[pack_queue(s)], lay->pack_bytes, s, nullptr);
    if (!would_pack(d, s)) return b2t_gemm_bf16_f32(&d, st);
    return gemm_bf16p_run(&d, nullptr, Bp_pre, lay->pack[pack_queue(s)], lay->pack_bytes, s, dropA);
  }
  void call(int r) { ht_point(3); host_delay(); if (!rc) rc = r; }     // (r: the launch that just returned)
};

b2t_gemm_desc gd(const float* A, const float* Bm, float* C, int M, int N, int K) {
  b2t_gemm_desc d;
  memset(&d, 0, sizeof(d));
  d.A = A; d.B = Bm; d.C = C; d.M = M; d.N = N; d.K = K; d.Z = 1;
  d.a_kcontig = 1; d.b_kcontig = 1;
  return d;
}

uint64_t mix_seed(uint64_t seed, uint64_t k) { return seed * 1000003ull + k; }

// ---- task graph + list scheduler ------------------------------------------------------------------------------------
// A pass is a DAG of tasks (a GEMM with its epilogue kernels, one sweep chunk, a reduction ...) with rough duration
// estimates.  The command processor serves the hardware queues that share one of its 4 pipes in time slices: with the 11
// streams of the round-1 plan a cross-stream dependency cost 110-140 us inside a step (15 us on an idle chip,
// tools/bench_hop_*.py).  So the plan runs on FOUR in-order queues -- the caller's stream and three workers, one per
// pipe -- and a list scheduler (HEFT: longest path to the end first, earliest finish, gaps may be filled) decides which
// queue a task goes to.  Results do not depend on the schedule: every accumulation order is a dependency of the graph.
constexpr float HOP_US = 20.f;   // event record -> wait on another queue -> launch
constexpr unsigned Q_ANY = 0xffffffffu, Q_MAIN = 1u;

struct Task {
  const char* name; float est; unsigned qmask; std::vector<int> deps; std::function<void(hipStream_t)> run;
  int q = -1; float start = 0.f, end = 0.f, rank = 0.f; bool cross = false; hipEvent_t ev = nullptr;
  int cls = -1;   // admission class (XCD set of a sweep under the XCD-local hand-off): classes 0 / 1 (layer parity) hold two tasks in flight, classes 2..5 (not used by the plans here: sweeps with one workgroup per CU) one
};

struct Plan {
  std::vector<Task> t;
  int add(const char* name, float est, unsigned qmask, std::initializer_list<int> deps, std::function<void(hipStream_t)> run) {
    Task k;
    k.name = name; k.est = est; k.qmask = qmask; k.run = std::move(run);
    for (int d : deps) if (d >= 0) k.deps.push_back(d);
    t.push_back(std::move(k));
    return (int)t.size() - 1;
  }
  void dep(int task, int on) { if (task >= 0 && on >= 0) t[task].deps.push_back(on); }
};

float est_step_us(int bwd) {   // microseconds per time step of a sweep inside the step (H = 512, B = 64)
  static const float f = getenv("B2T_EST_FWD_US") ? (float)atof(getenv("B2T_EST_FWD_US")) : 5.5f;
  static const float b = getenv("B2T_EST_BWD_US") ? (float)atof(getenv("B2T_EST_BWD_US")) : 6.0f;
  return bwd ? b : f;
}
float est_gemm(double M, double N, double K, double Z = 1) {   // launch + FLOPs at the rate a GEMM reaches next to the sweeps
  static const double tfs = getenv("B2T_EST_GEMM_TFS") ? atof(getenv("B2T_EST_GEMM_TFS")) : 80.0;
  return 12.f + (float)(2.0 * M * N * K * Z / (tfs * 1e6));
}

// The scheduling step alone (host arithmetic, no HIP): fills q / start / end / rank / cross of every task and returns the
// issue order (planned start, ties by task id).  The graph may list its tasks in any order (the admission edges added
// after a first pass point from a later-created task to an earlier-created one): ranks are computed over a true topological
// order (Kahn, smallest id first), and since rank(task) > rank(successor) the rank-ordered placement below sees every
// dependency before its dependants.  Returns an empty order if the graph has a cycle.  Exposed for the CPU tests as
// b2t_plan_schedule_host.
std::vector<int> schedule_plan(Plan& P, int nq) {
  const int n = (int)P.t.size();
  std::vector<std::vector<int>> succ(n);
  std::vector<int> indeg(n, 0), topo;
  for (int i = 0; i < n; ++i) for (int d : P.t[i].deps) { succ[d].push_back(i); ++indeg[i]; }
  {
    std::priority_queue<int, std::vector<int>, std::greater<int>> ready;
    for (int i = 0; i < n; ++i) if (!indeg[i]) ready.push(i);
    while (!ready.empty()) {
      const int i = ready.top(); ready.pop();
      topo.push_back(i);
      for (int s2 : succ[i]) if (--indeg[s2] == 0) ready.push(s2);
    }
    if ((int)topo.size() != n) return {};
  }
  for (int k = n - 1; k >= 0; --k) {
    const int i = topo[k];
    float r = 0.f;
    for (int s2 : succ[i]) r = std::max(r, P.t[s2].rank + HOP_US);
    P.t[i].rank = P.t[i].est + r;
  }
  std::vector<int> order = topo;    // stable sort of a topological order: equal ranks (zero-cost chains) keep dependencies first
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return P.t[a].rank > P.t[b].rank; });
  std::vector<std::vector<std::pair<float, float>>> busy(nq);
  for (int id : order) {
    Task& k = P.t[id];
    const float dur = std::max(k.est, 0.5f);   // bookkeeping tasks occupy a slot too: two tasks of a queue never share a start
    int bq = -1; float bs = 0.f;
    for (int q = 0; q < nq; ++q) {
      if (!((k.qmask >> q) & 1u) && nq > 1) continue;
      float s = 0.f;
      for (int d : k.deps) s = std::max(s, P.t[d].end + (P.t[d].q != q ? HOP_US : 0.f));
      for (const auto& iv : busy[q]) {
        if (s + dur <= iv.first) break;
        s = std::max(s, iv.second);
      }
      if (bq < 0 || s < bs - 0.5f) { bq = q; bs = s; }
    }
    if (bq < 0) bq = 0;
    k.q = bq; k.start = bs; k.end = bs + dur;
    auto& b = busy[bq];
    b.insert(std::upper_bound(b.begin(), b.end(), std::make_pair(k.start, k.end)), std::make_pair(k.start, k.end));
  }
  for (int i = 0; i < n; ++i) for (int s : succ[i]) if (P.t[s].q != P.t[i].q) P.t[i].cross = true;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    return P.t[a].start != P.t[b].start ? P.t[a].start < P.t[b].start : a < b;
  });
  return order;
}

// Admission control for the XCD-local sweeps.  A row group's workgroups must ALL be resident on their XCD before its recurrence
// can move, and an XCD holds the row groups of exactly two sweeps (32-unit forward workgroups: 16 + 16 CUs; backward: 32 + 32
// workgroups at two per CU).  Layers of one parity share an XCD set, and nothing in the data dependencies keeps layers 0, 2 and
// 4 from being in flight together: each then gets part of its workgroups resident, the XCD is full and all three spin until
// the hand-off timeout (seen under rocprofv3 in the trainer loop, about once in 150 steps).  So the k-th task of a class, in
// planned start order, waits for the (k-2)-th to finish: never more than two in flight.  The extra edges point forward in a
// topological order, so the graph stays acyclic; they rarely bind (the third sweep of a parity normally starts later anyway).
// (Classes 2..5 have room for ONE task in flight -- the k-th waits for the (k-1)-th: sweeps that fill their XCD set with one
// workgroup per CU.  The plans here use classes 0 / 1 only.)
constexpr int N_CLS = 6;
inline int cls_capacity(int k) { return k < 2 ? 2 : 1; }
void add_admission_edges(Plan& P, const std::vector<int>& order) {
  std::vector<int> seen[N_CLS];
  for (int id : order) {
    const int k = P.t[id].cls;
    if (k < 0 || k >= N_CLS) continue;
    const size_t cap = (size_t)cls_capacity(k);
    if (seen[k].size() >= cap) P.dep(id, seen[k][seen[k].size() - cap]);
    seen[k].push_back(id);
  }
}

// FNV-1a over the bytes that determine a pass
uint64_t key_bytes(uint64_t h, const void* p, size_t n) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
template <typename V> uint64_t key_of(uint64_t h, const V& v) { return key_bytes(h, &v, sizeof(V)); }

uint64_t pass_key(int which, const b2t_model_t* prm, const b2t_model_t* grd, const b2t_pass_t* p, std::initializer_list<const void*> ptrs,
                  std::initializer_list<long long> ints) {
  uint64_t h = 1469598103934665603ull;
  h = key_of(h, which);
  h = key_bytes(h, prm, sizeof(*prm));
  if (grd) h = key_bytes(h, grd, sizeof(*grd));
  const bool drop = p->in_drop > 0.f || p->rnn_drop > 0.f;
  const long long f[] = {p->B, p->T, p->chunks, p->fwd_mode, p->bwd_mode, p->bf16_gemm, p->save, p->chunks_bwd, p->wgrad_chunk_mask,
                         (long long)(drop ? p->seed : 0ull)};
  h = key_bytes(h, f, sizeof(f));
  h = key_of(h, p->in_drop); h = key_of(h, p->rnn_drop);
  for (const void* q : ptrs) h = key_of(h, q);
  for (long long v : ints) h = key_of(h, v);
  for (const char* name : {"B2T_FUSED_PROJ", "B2T_HANDOFF16", "B2T_PREPACK", "B2T_WGRAD_SPLIT", "B2T_ZPACK", "B2T_GEMM_256", "B2T_WAVE_KS", "B2T_WAVE_LOCAL", "B2T_WAVE_SC1_LOADS"}) {   // read per pass by the code below / the sweeps
    const char* e = getenv(name);
    h = key_bytes(h, e ? e : "", e ? strlen(e) + 1 : 1);   // the whole value ("1" and "10" are different plans)
  }
  return h ? h : 1;
}

// The step as a graph (round-3 candidate 6, round-4 verdict item 9).  Stream capture of the four-queue plan as a whole ends the
// process inside the runtime (fork by event, ~100 cross-queue edges, join); so the graph is BUILT from the plan: every task is
// captured alone, on a capture stream standing in for its queue (a task is a short in-order sequence of launches on one
// stream: that captures cleanly), and becomes a child-graph node whose dependencies are the task's edges in the plan plus its
// predecessor on the same queue -- the graph has exactly the plan's order and concurrency (never more than four sweeps in
// flight).  Kernel arguments are baked into the nodes, so a graph serves only passes whose key repeats (every pointer, shape,
// mode; the dropout seed when dropout is on); a key's first pass runs eagerly, its second builds, later ones replay with ONE
// runtime call.  Any HIP error while building switches the mode off for the executor (the pass then runs eagerly: a capture
// launches nothing).  Returns true if the pass was launched.
bool run_plan_graph(Ctx& c, Plan& P, const std::vector<int>& order, int nq) {
  static const bool on = getenv("B2T_EXEC_GRAPH") && atoi(getenv("B2T_EXEC_GRAPH")) != 0;
  b2t_exec* ex = c.ex;
  if (!on || ex->graph_failed || ex->profile || c.rc) return false;
  auto it = ex->graphs.find(c.gkey);
  if (it == ex->graphs.end()) {
    if (ex->seen_keys.insert(c.gkey).second) return false;   // first pass with this key: eager
    if (ex->graphs.size() >= 32) {                            // bounded: pointers that never repeat must not grow the table
      for (auto& kv : ex->graphs) (void)hipGraphExecDestroy(kv.second);
      ex->graphs.clear(); ex->seen_keys.clear();
      return false;
    }
    const int n = (int)P.t.size();
    hipGraph_t G = nullptr;
    std::vector<hipGraphNode_t> node((size_t)n, nullptr);
    hipStream_t real[8];
    for (int q = 0; q < 8; ++q) real[q] = c.qs[q];
    const char* where = ""; hipError_t herr = hipSuccess; const char* tname = "";
    auto H_ = [&](hipError_t e, const char* w) { if (e != hipSuccess && herr == hipSuccess) { herr = e; where = w; } return e == hipSuccess; };
    bool ok = H_(hipGraphCreate(&G, 0), "hipGraphCreate");
    for (int q = 0; q < nq && ok; ++q) {
      if (!ex->cap[q]) ok = H_(hipStreamCreateWithFlags(&ex->cap[q], hipStreamNonBlocking), "hipStreamCreate");
      c.qs[q] = ex->cap[q];                                   // (the amp GEMMs pick their pack scratch by queue)
    }
    int last[8]; for (int q = 0; q < 8; ++q) last[q] = -1;
    for (int id : order) {
      if (!ok || c.rc) break;
      Task& k = P.t[id];
      hipStream_t s = ex->cap[k.q];
      hipGraph_t sub = nullptr;
      tname = k.name;
      ok = H_(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed), "hipStreamBeginCapture");
      if (ok && k.run) k.run(s);
      ok = ok && H_(hipStreamEndCapture(s, &sub), "hipStreamEndCapture") && !c.rc;
      std::vector<hipGraphNode_t> deps;
      for (int d : k.deps) if (node[(size_t)d]) deps.push_back(node[(size_t)d]);
      if (last[k.q] >= 0 && node[(size_t)last[k.q]]) deps.push_back(node[(size_t)last[k.q]]);
      std::sort(deps.begin(), deps.end());
      deps.erase(std::unique(deps.begin(), deps.end()), deps.end());   // (a repeated dependency is an invalid argument)
      size_t nn = 0;
      if (ok && sub) ok = H_(hipGraphGetNodes(sub, nullptr, &nn), "hipGraphGetNodes");
      static const bool flat = !(getenv("B2T_EXEC_GRAPH_FLAT") && atoi(getenv("B2T_EXEC_GRAPH_FLAT")) == 0);
      bool plain = flat;   // only kernels / memsets / empty nodes are copied; a task with anything else (a captured 1-D copy) stays a child graph
      if (ok && nn && flat) {
        std::vector<hipGraphNode_t> ns0(nn);
        size_t n0 = nn;
        ok = H_(hipGraphGetNodes(sub, ns0.data(), &n0), "hipGraphGetNodes");
        for (size_t i = 0; i < n0 && ok; ++i) {
          hipGraphNodeType ty;
          ok = H_(hipGraphNodeGetType(ns0[i], &ty), "hipGraphNodeGetType");
          if (ty != hipGraphNodeTypeKernel && ty != hipGraphNodeTypeMemset && ty != hipGraphNodeTypeEmpty) plain = false;
        }
      }
      if (ok && nn && plain) {
        // the task's nodes copied into the pass graph itself (a child-graph node per task made hipGraphLaunch cost 11 ms): the
        // capture of one stream is a chain -- walked from its root along its edges
        std::vector<hipGraphNode_t> ns(nn), from, to;
        size_t ne = 0;
        ok = H_(hipGraphGetNodes(sub, ns.data(), &nn), "hipGraphGetNodes") && H_(hipGraphGetEdges(sub, nullptr, nullptr, &ne), "hipGraphGetEdges");
        from.resize(ne); to.resize(ne);
        if (ok && ne) ok = H_(hipGraphGetEdges(sub, from.data(), to.data(), &ne), "hipGraphGetEdges");
        std::vector<hipGraphNode_t> chain;
        if (ok) {
          hipGraphNode_t cur = nullptr;
          for (hipGraphNode_t v : ns) { bool has_in = false; for (size_t e = 0; e < ne; ++e) has_in = has_in || to[e] == v; if (!has_in) { cur = v; break; } }
          while (cur && chain.size() < nn) {
            chain.push_back(cur);
            hipGraphNode_t nx = nullptr;
            for (size_t e = 0; e < ne; ++e) if (from[e] == cur) { nx = to[e]; break; }
            cur = nx;
          }
          if (chain.size() != nn) { ok = false; where = "task capture is not a chain"; }
        }
        hipGraphNode_t prev = nullptr;
        for (size_t i = 0; i < chain.size() && ok; ++i) {
          hipGraphNodeType ty;
          ok = H_(hipGraphNodeGetType(chain[i], &ty), "hipGraphNodeGetType");
          std::vector<hipGraphNode_t> dd = i == 0 ? deps : std::vector<hipGraphNode_t>{prev};
          hipGraphNode_t out = nullptr;
          if (!ok) break;
          if (ty == hipGraphNodeTypeKernel) {
            hipKernelNodeParams kp;
            ok = H_(hipGraphKernelNodeGetParams(chain[i], &kp), "hipGraphKernelNodeGetParams") &&
                 H_(hipGraphAddKernelNode(&out, G, dd.data(), dd.size(), &kp), "hipGraphAddKernelNode");
          } else if (ty == hipGraphNodeTypeMemset) {
            hipMemsetParams mp;
            ok = H_(hipGraphMemsetNodeGetParams(chain[i], &mp), "hipGraphMemsetNodeGetParams") &&
                 H_(hipGraphAddMemsetNode(&out, G, dd.data(), dd.size(), &mp), "hipGraphAddMemsetNode");
          } else if (ty == hipGraphNodeTypeEmpty) {
            ok = H_(hipGraphAddEmptyNode(&out, G, dd.data(), dd.size()), "hipGraphAddEmptyNode");
          } else { ok = false; where = "unsupported node type in a task capture"; }
          prev = out;
        }
        node[(size_t)id] = prev;
      } else if (ok) {
        ok = nn ? H_(hipGraphAddChildGraphNode(&node[(size_t)id], G, deps.data(), deps.size(), sub), "hipGraphAddChildGraphNode")
                : H_(hipGraphAddEmptyNode(&node[(size_t)id], G, deps.data(), deps.size()), "hipGraphAddEmptyNode");
      }
      if (sub) (void)hipGraphDestroy(sub);
      last[k.q] = id;
    }
    for (int q = 0; q < 8; ++q) c.qs[q] = real[q];
    hipGraphExec_t exec = nullptr;
    ok = ok && !c.rc && H_(hipGraphInstantiate(&exec, G, nullptr, nullptr, 0), "hipGraphInstantiate");
    if (G) (void)hipGraphDestroy(G);
    if (!ok) {
      (void)hipGetLastError();
      ex->graph_failed = true;
      fprintf(stderr, "exec: building the pass graph failed (%s in task '%s': %s; pass rc %d, last error: %s); eager plans from here on\n", where, tname,
              herr != hipSuccess ? hipGetErrorString(herr) : "-", c.rc, b2t_last_error());
      return c.rc != 0;      // an error of the pass itself stays an error; a runtime refusal falls back to the eager plan
    }
    ++ex->graph_builds;
    it = ex->graphs.emplace(c.gkey, exec).first;
  }
  if (check_hip(hipGraphLaunch(it->second, c.main), "hipGraphLaunch")) { c.rc = 1; return true; }
  ++ex->graph_replays;
  return true;
}

// Timing jitter for the plan's hazard test (B2T_EXEC_JITTER=seed, read per pass; round-5 verdict item 1c): a single wave that
// spins for `us` microseconds of the 100 MHz wall clock, enqueued in front of randomly chosen tasks on the task's own queue,
// behind its cross-queue waits.  Results must not depend on when a task starts: an ordering the plan has only by timing (a
// missing edge) shows up as arenas that differ between seeds (tests/test_gpu_step_parity.py, tools/r5_jitter.py).
__global__ void jitter_spin_kernel(unsigned us) {
  const unsigned long long t0 = wall_clock64();
  while (wall_clock64() - t0 < 100ull * us) __builtin_amdgcn_s_sleep(32);
}
struct Jitter {
  bool on = false; uint64_t s = 0;
  explicit Jitter(uint64_t pass_no) {
    const char* e = getenv("B2T_EXEC_JITTER");
    if (e && e[0]) { on = true; s = (strtoull(e, nullptr, 0) + 1) * 0x9E3779B97F4A7C15ull + pass_no * 0xD1B54A32D192ED03ull; }
  }
  uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
  void maybe(hipStream_t q) {
    if (!on) return;
    const uint64_t r = next();
    if (r % 3 != 0) return;                                   // a third of the tasks start late ...
    const unsigned us = 10u + (unsigned)((r >> 8) % 391u);    // ... by 10-400 us (a sweep chunk takes ~500, a GEMM 20-500)
    hipLaunchKernelGGL(jitter_spin_kernel, dim3(1), dim3(64), 0, q, us);
  }
};

void run_plan(Ctx& c, Plan& P, int nq, const hipStream_t* qs) {
  const int n = (int)P.t.size();
  static std::atomic<uint64_t> pass_no{0};   // (executors may run passes from different host threads)
  Jitter jit(pass_no.fetch_add(1) + 1);
  bool classes = false;
  for (const Task& k : P.t) classes = classes || k.cls >= 0;
  if (classes && nq > 1) add_admission_edges(P, schedule_plan(P, nq));
  const std::vector<int> order = schedule_plan(P, nq);
  if ((int)order.size() != n) { c.call(1); set_error("exec: the plan's task graph has a cycle"); return; }
  static const bool dump = getenv("B2T_PLAN_DUMP") != nullptr;
  if (dump) {
    fprintf(stderr, "plan: %d tasks on %d queues\n", n, nq);
    for (int id : order) fprintf(stderr, "  %9.1f %8.1f q%d %s\n", P.t[id].start, P.t[id].est, P.t[id].q, P.t[id].name);
  }
  if (c.gkey && run_plan_graph(c, P, order, nq)) return;
  Ctx::ht_pass();
  std::vector<int> pos(n);
  for (int i = 0; i < n; ++i) pos[order[i]] = i;
  for (int id : order) {
    if (c.rc) return;
    Task& k = P.t[id];
    hipStream_t s = qs[k.q];
    int last[8]; for (int q = 0; q < 8; ++q) last[q] = -1;   // per foreign queue: the dependency issued last covers the others
    for (int d : k.deps) {
      const int dq = P.t[d].q;
      // a dependency must have been issued already; across queues it must have left an event (never drop an edge silently)
      if (pos[d] >= pos[id] || (dq != k.q && !P.t[d].ev)) {
        c.call(1);
        set_error("exec: task '%s' would be issued before its dependency '%s' (plan order broken)", k.name, P.t[d].name);
        return;
      }
      if (dq != k.q && (last[dq] < 0 || pos[d] > pos[last[dq]])) last[dq] = d;
    }
    for (int q = 0; q < nq; ++q) if (last[q] >= 0) c.wait(s, P.t[last[q]].ev);
    if (k.run) { jit.maybe(s); Ctx::ht_mark(); k.run(s); }
    if (k.cross) k.ev = c.record(s);
  }
}

// Cost of one cross-queue dependency between two streams on the otherwise idle chip: a chain of tiny launches that hop
// from one to the other through events (microseconds per hop; < 0 on a HIP error).
float hop_us(b2t_exec* ex, hipStream_t a, hipStream_t b) {
  const int warm = 2, n = 8;
  std::vector<hipEvent_t> evs;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  bool ok = hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
  auto hop = [&](hipStream_t from, hipStream_t to) {
    hipEvent_t e = nullptr;
    ok = ok && hipMemsetAsync(ex->scratch, 0, 64, from) == hipSuccess && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (e) evs.push_back(e);
    ok = ok && hipEventRecord(e, from) == hipSuccess && hipStreamWaitEvent(to, e, 0) == hipSuccess;
  };
  for (int i = 0; i < warm + n && ok; ++i) {
    if (i == warm) ok = ok && hipEventRecord(e0, a) == hipSuccess;
    hop(a, b); hop(b, a);
  }
  ok = ok && hipEventRecord(e1, a) == hipSuccess && hipEventSynchronize(e1) == hipSuccess;
  float ms = 0.f;
  ok = ok && hipEventElapsedTime(&ms, e0, e1) == hipSuccess;
  for (hipEvent_t e : evs) (void)hipEventDestroy(e);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  return ok ? ms * 1e3f / (2 * n) : -1.f;
}

// Worker queues.  The command processor has 4 pipes; a hardware queue lives on one of them (assigned round-robin as HIP
// creates its queues) and queues that share a pipe are served in time slices: a dependency between two such queues costs
// 35-85 us on an idle chip instead of 15, and 110-140 us inside a step (tools/bench_hop_matrix.py, bench_hop_neighbors.py).
// So the plan wants the caller's stream plus n_workers streams that are pairwise on different pipes.  Which pipe a new
// stream lands on depends on everything the process created before, so it is MEASURED: candidates are created, each
// is kept if its hop to the caller's stream and to every worker kept so far is a fast one, the rest are destroyed.
int choose_workers(b2t_exec* ex, hipStream_t main) {
  for (hipStream_t st : ex->phys) if (st) (void)hipStreamDestroy(st);
  ex->phys.clear();
  const int want = ex->n_workers, n_cand = 2 * (want + 1) + 2;
  std::vector<hipStream_t> cand(n_cand, nullptr);
  for (int i = 0; i < n_cand; ++i)
    if (check_hip(hipStreamCreateWithFlags(&cand[i], hipStreamNonBlocking), "hipStreamCreate")) return 1;
  static const bool verbose = getenv("B2T_PLAN_DUMP") != nullptr;
  std::vector<float> to_main(n_cand);
  float best = 1e30f;
  for (int i = 0; i < n_cand; ++i) {
    to_main[i] = hop_us(ex, main, cand[i]);
    if (to_main[i] < 0.f) { set_error("exec: queue calibration failed (HIP error)"); return 1; }
    best = std::min(best, to_main[i]);
  }
  const float thr = 1.6f * best + 2.f;
  std::vector<int> kept;
  for (int i = 0; i < n_cand && (int)kept.size() < want; ++i) {
    bool fast = to_main[i] <= thr;
    for (size_t k = 0; k < kept.size() && fast; ++k) fast = hop_us(ex, cand[kept[k]], cand[i]) <= thr;
    if (fast) kept.push_back(i);
  }
  for (int i = 0; i < n_cand && (int)kept.size() < want; ++i)   // fewer pipes than queues wanted: take what is there
    if (std::find(kept.begin(), kept.end(), i) == kept.end()) kept.push_back(i);
  if (verbose) {
    fprintf(stderr, "exec: hop to the caller's stream (us):");
    for (int i = 0; i < n_cand; ++i) fprintf(stderr, " %.1f", to_main[i]);
    fprintf(stderr, " -> workers");
    for (int k : kept) fprintf(stderr, " %d", k);
    fprintf(stderr, "\n");
  }
  for (int i = 0; i < n_cand; ++i) {
    if (std::find(kept.begin(), kept.end(), i) != kept.end()) ex->phys.push_back(cand[i]);
    else (void)hipStreamDestroy(cand[i]);
  }
  ex->have_workers = true;
  ex->workers_for = main;
  return 0;
}

// queue 0 = the caller's stream; the workers only when the plan is pipelined (shapes whose sweeps cannot share the chip
// run as one in-order sequence)
int plan_queues(Ctx& c, bool piped, hipStream_t* qs) {
  b2t_exec* ex = c.ex;
  qs[0] = c.main;
  if (!piped) return 1;
  if (!ex->have_workers || ex->workers_for != c.main) c.call(choose_workers(ex, c.main));
  int n = 1;
  for (hipStream_t st : ex->phys) if (n < 8) qs[n++] = st;
  return n;
}

int check_common(const b2t_exec* ex, const b2t_model_t* m, const b2t_pass_t* p, const char* what) {
  B2T_REQUIRE(ex && m && p, "%s: null argument", what);
  B2T_REQUIRE(m->L >= 1 && m->L <= MAXL && m->L <= ex->L, "%s: %d layers (executor has %d, max %d)", what, m->L, ex->L, MAXL);
  B2T_REQUIRE(m->H > 0 && m->H % 16 == 0 && m->F > 0 && m->F % 4 == 0 && m->C > 0, "%s: bad dims F=%d H=%d C=%d", what, m->F, m->H, m->C);
  B2T_REQUIRE(p->B > 0 && p->T > 0 && out_T(m, p->T) > 0, "%s: bad batch B=%d T=%d (sequence shorter than patch_size?)", what, p->B, p->T);
  B2T_REQUIRE(m->patch == 0 || m->stride > 0, "%s: patch_size %d needs patch_stride > 0", what, m->patch);
  return 0;
}

}  // namespace
}  // namespace b2t

using namespace b2t;

extern "C" int b2t_exec_create(int n_layers, b2t_exec** out) {
  B2T_REQUIRE(out && n_layers >= 1 && n_layers <= MAXL, "exec_create: 1..%d layers", MAXL);
  b2t_exec* ex = new b2t_exec();
  ex->L = n_layers;
  // Worker queues are created at the first pipelined pass, when the caller's stream is known (choose_workers).
  if (const char* env = getenv("B2T_WORKERS")) ex->n_workers = std::max(1, std::min(7, atoi(env)));
  ex->sweep_qmask = getenv("B2T_SWEEP_WORKERS_ONLY") ? (((1u << ex->n_workers) - 1u) << 1) : 0xffffffffu;
  if (const char* env = getenv("B2T_SWEEP_QMASK")) ex->sweep_qmask = (unsigned)strtoul(env, nullptr, 0);   // experiments: bit q = queue q
  // Never more than four sweeps in flight, whatever B2T_WORKERS says: with the device-scope hand-off a sweep's workgroups are
  // spread over the chip and four sweeps fill it exactly (forward 4 x 64 workgroups at one per CU, backward 4 x 128 at two); a
  // fifth could leave several of them partly resident, i.e. deadlocked until the hand-off timeout.
  ex->sweep_qmask &= 0xfu;
  if (!ex->sweep_qmask) ex->sweep_qmask = 0xfu;
  if (check_hip(hipMalloc(reinterpret_cast<void**>(&ex->scratch), 256), "hipMalloc")) { delete ex; return 1; }
  *out = ex;
  return 0;
}

extern "C" int b2t_exec_destroy(b2t_exec* ex) {
  if (!ex) return 0;
  for (hipStream_t st : ex->phys) if (st) (void)hipStreamDestroy(st);
  if (ex->scratch) (void)hipFree(ex->scratch);
  for (hipEvent_t e : ex->pool) (void)hipEventDestroy(e);
  for (hipEvent_t e : ex->tpool) (void)hipEventDestroy(e);
  for (auto& kv : ex->graphs) (void)hipGraphExecDestroy(kv.second);
  for (hipStream_t st : ex->cap) if (st) (void)hipStreamDestroy(st);
  delete ex;
  return 0;
}

extern "C" int b2t_plan_schedule_host(int n_tasks, const float* est_us, const uint32_t* qmask, const int32_t* dep_off,
                                      const int32_t* deps, int n_queues, int32_t* queue, float* start_us, int32_t* order) {
  B2T_REQUIRE(n_tasks >= 0 && n_queues >= 1 && n_queues <= 8 && (n_tasks == 0 || (est_us && qmask && dep_off && queue && start_us && order)),
              "plan_schedule_host: bad arguments");
  Plan P;
  for (int i = 0; i < n_tasks; ++i) {
    B2T_REQUIRE(est_us[i] >= 0.f && dep_off[i] <= dep_off[i + 1], "plan_schedule_host: task %d: negative estimate / bad dependency offsets", i);
    const int t = P.add("task", est_us[i], qmask[i], {}, nullptr);
    for (int k = dep_off[i]; k < dep_off[i + 1]; ++k) {
      B2T_REQUIRE(deps && deps[k] >= 0 && deps[k] < i, "plan_schedule_host: task %d depends on %d (tasks must be listed in topological order)", i, deps ? deps[k] : -1);
      P.dep(t, deps[k]);
    }
  }
  const std::vector<int> ord = schedule_plan(P, n_queues);
  for (int i = 0; i < n_tasks; ++i) { queue[i] = P.t[i].q; start_us[i] = P.t[i].start; order[i] = ord[i]; }
  return 0;
}

extern "C" int b2t_plan_admission_host(int n_tasks, const float* est_us, const uint32_t* qmask, const int32_t* dep_off,
                                       const int32_t* deps, const int32_t* cls, int n_queues, int32_t* queue, float* start_us,
                                       float* end_us, int32_t* order) {
  B2T_REQUIRE(n_tasks >= 0 && n_queues >= 1 && n_queues <= 8 && (n_tasks == 0 || (est_us && qmask && dep_off && cls && queue && start_us && end_us && order)),
              "plan_admission_host: bad arguments");
  Plan P;
  for (int i = 0; i < n_tasks; ++i) {
    B2T_REQUIRE(est_us[i] >= 0.f && dep_off[i] <= dep_off[i + 1], "plan_admission_host: task %d: negative estimate / bad dependency offsets", i);
    const int t = P.add("task", est_us[i], qmask[i], {}, nullptr);
    P.t[t].cls = cls[i];
    for (int k = dep_off[i]; k < dep_off[i + 1]; ++k) {
      B2T_REQUIRE(deps && deps[k] >= 0 && deps[k] < i, "plan_admission_host: task %d depends on %d (tasks must be listed in topological order)", i, deps ? deps[k] : -1);
      P.dep(t, deps[k]);
    }
  }
  if (n_queues > 1) add_admission_edges(P, schedule_plan(P, n_queues));
  const std::vector<int> ord = schedule_plan(P, n_queues);
  B2T_REQUIRE((int)ord.size() == n_tasks, "plan_admission_host: the graph with its admission edges has a cycle");
  for (int i = 0; i < n_tasks; ++i) { queue[i] = P.t[i].q; start_us[i] = P.t[i].start; end_us[i] = P.t[i].end; order[i] = ord[i]; }
  return 0;
}

extern "C" size_t b2t_exec_sync_bytes(int n_layers) { return ((size_t)2 * n_layers + 1) * b2t_gru_sync_bytes(0); }   // + the split-K tile counters

extern "C" size_t b2t_pass_ws_bytes(const b2t_model_t* m, const b2t_pass_t* p) {
  if (!m || !p || p->B <= 0 || p->T <= 0 || out_T(m, p->T) <= 0 || m->L < 1 || m->L > MAXL) return 0;
  Layout w;
  carve(m, p, nullptr, w);
  return w.bytes + 256;
}

extern "C" int b2t_exec_graph_stats(const b2t_exec* ex, long long* builds, long long* replays, int* failed) {
  B2T_REQUIRE(ex && builds && replays && failed, "exec_graph_stats: null argument");
  *builds = ex->graph_builds; *replays = ex->graph_replays; *failed = ex->graph_failed ? 1 : 0;
  return 0;
}

extern "C" int b2t_exec_profile(b2t_exec* ex, int on) {
  B2T_REQUIRE(ex, "exec_profile: null executor");
  ex->profile = on != 0;
  return 0;
}

extern "C" int b2t_exec_profile_read(b2t_exec* ex, int* kind_host, double* flops_host, float* ms_host, int cap) {
  if (!ex) { set_error("exec_profile_read: null executor"); return -1; }
  if (check_hip(hipDeviceSynchronize(), "exec_profile_read: sync")) return -1;
  int n = 0;
  for (const ProfRec& r : ex->recs) {
    if (n >= cap) break;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = 0.f;
    kind_host[n] = r.kind; flops_host[n] = r.flops; ms_host[n] = ms; ++n;
  }
  ex->recs.clear();
  ex->next_tev = 0;
  return n;
}

// ------------------------------------------------------------------------------------------------------------------
// forward: day layer -> (patch) -> L x GRU -> head
// ------------------------------------------------------------------------------------------------------------------
extern "C" int b2t_model_forward(b2t_exec* ex, const b2t_model_t* prm, const b2t_pass_t* p, const float* x,
                                 const int32_t* day_idx, const float* states, float* logits, float* hidden, void* ws,
                                 void* sync_ws, void* stream) {
  { int rc = check_common(ex, prm, p, "model_forward"); if (rc) return rc; }
  B2T_REQUIRE(x && day_idx && logits && hidden && ws, "model_forward: null buffer");
  const int B = p->B, T = p->T, F = prm->F, H = prm->H, L = prm->L, Cc = prm->C;
  const int Tp = out_T(prm, T), In0 = in0(prm);
  const int mode = p->fwd_mode;
  B2T_REQUIRE((mode & 0xff) == 0 || sync_ws, "model_forward: sync_ws is required for the persistent sweeps");
  Layout w;
  carve(prm, p, reinterpret_cast<char*>(ws), w);
  Ctx c{ex, as_stream(stream), p->bf16_gemm != 0};
  c.lay = &w;
  ex->next_ev = 0;
  const size_t sync_block = b2t_gru_sync_bytes(0);
  auto sync_of = [&](int l) { return sync_ws ? reinterpret_cast<char*>(sync_ws) + (size_t)l * sync_block : nullptr; };

  // Round 6: the sweeps of all L layers as ONE launch, layer l + 1 a step or two behind layer l (gru_wave.hip); the projections of the
  // layers >= 1 happen inside it.  One "chunk": nothing is pipelined over time any more.
  const bool wave = wave_pass(prm, p, mode);
  int chunks[MAXC][2];
  const int nc = make_chunks(Tp, p->chunks, chunks);
  c.exact_k = nc > 1;
  c.nq = plan_queues(c, nc > 1 || wave, c.qs);   // the queues of this pass (the plan below refers to them by index)
  c.gkey = pass_key(1, prm, nullptr, p, {x, day_idx, states, logits, hidden, ws, sync_ws, stream}, {c.nq});
  const long long a_s0_l0 = prm->patch > 0 ? (long long)prm->stride * F : F;
  // rows x K that b2t_gemm_f32 serves with its skinny (weight-streaming) kernel: exact fp32 only, one frame of <= 64 utterances
  auto skinny = [&](long long rows, int K) { return !c.bf16_gemm && !c.exact_k && rows <= 64 && K % 16 == 0; };
  const float hs = std::max(0.25f, (float)H * H / (512.f * 512.f)) * std::max(1, (B + 63) / 64);   // sweep cost scale
  const unsigned q_sweep = ex->sweep_qmask;

  Plan P;
  const int t_start = P.add("start", 0.f, Q_MAIN, {}, nullptr);
  // 1. day layer: U[b] = softsign(x[b] @ W[day[b]] + c[day[b]])   (rnn_model.py:95-99); the [B,512,512] gather of the
  //    reference does not exist: the GEMM indexes the day weights by day_idx (b_zmap).  Without patching and input
  //    dropout the day layer runs chunk by chunk like everything behind it (the first sweep starts ~0.25 ms earlier).
  const bool day_chunked = prm->patch == 0 && !(p->in_drop > 0.f) && nc > 1;
  int t_day[MAXC];
  auto day_task = [&](int t0, int n) {
    return P.add("day", est_gemm(n, F, F, B), Q_ANY, {t_start}, [&, t0, n](hipStream_t s) {
      b2t_gemm_desc d = gd(x + (long long)t0 * F, prm->day_w, w.U + (long long)t0 * F, n, F, F);
      d.Z = B; d.a_s0 = F; d.a_sz = (long long)T * F; d.b_kcontig = 0; d.b_s0 = F; d.b_sz = prm->day_w_stride;
      d.c_s0 = F; d.c_sz = (long long)T * F; d.bias = prm->day_b; d.bias_sz = prm->day_b_stride; d.b_zmap = day_idx; d.epilogue = 1;
      c.gemm(s, d);
      if (p->in_drop > 0.f)
        c.call(b2t_dropout_f32(w.U, w.Ud, (long long)B * T * F, p->in_drop, mix_seed(p->seed, 17), 0, reinterpret_cast<void*>(s)));
    });
  };
  // (the per-sentence day GEMMs of a chunk have the same 83-of-128-row tiles; whole-sequence or first-chunk-plus-rest day layers
  //  were measured equal, 19.00-19.12 ms all three: 17 GFLOP)
  if (day_chunked) for (int ci = 0; ci < nc; ++ci) t_day[ci] = day_task(chunks[ci][0], chunks[ci][1] - chunks[ci][0]);
  else { const int t = day_task(0, T); for (int ci = 0; ci < nc; ++ci) t_day[ci] = t; }

  // Round 4: the sweep of layer l makes the input projection of layer l + 1 itself, in its idle matrix-core slots, from the h
  // fragments each step holds in LDS anyway (b2t_gru_layer_fwd_fused_f32): the projection GEMMs of layers >= 1 -- 0.2 TFLOP per
  // C2 step and one GEMM + two queue hops on the critical path of every wavefront stage -- are gone.  Exact-fp32 persistent
  // sweeps, H <= 512, no dropout between the layers (training with rnn_dropout > 0 keeps the GEMMs: the mask sits between
  // out[l] and the projection), passes of at least 32 output frames (a streaming call would pay the per-chunk epilogue).
  const char* fused_s = getenv("B2T_FUSED_PROJ");   // read per pass (the tests compare the two forms in one process)
  const bool fused_env = !(fused_s && atoi(fused_s) == 0);
  const bool fuse_ok = fused_env && (mode & 0xff) == 1 && !(mode & B2T_GRU_BF16) && !c.bf16_gemm && H <= 512 && Tp >= 32;
  auto fused_from = [&](int l) { return fuse_ok && l >= 0 && l + 1 < L && w.outd[l] == w.out[l]; };   // layer l's sweep writes gi[l + 1]
  // slot 0 of out[l] = initial state, so out[l][0:T'] is the h_{t-1} matrix
  int t_init[MAXL], t_sw[MAXL][MAXC];
  for (int l = 0; l < L; ++l)
    t_init[l] = P.add("init", 5.f, Q_ANY, {t_start}, [&, l](hipStream_t s) {
      if (states && !p->save) return;   // inference with carried state: the first sweep chunk reads `states` in place (below)
      if (states) c.call(check_hip(hipMemcpyAsync(w.out[l], states + (size_t)l * B * H, sizeof(float) * B * H, hipMemcpyDeviceToDevice, s), "model_forward: state copy"));
      else c.call(b2t_broadcast_rows_f32(prm->h0, w.out[l], B, H, reinterpret_cast<void*>(s)));
    });
  // Round 5, bf16 mode: W_ih of a layer is the B operand of one projection GEMM PER TIME CHUNK; the two-pass kernel packed it to bf16
  // in front of every one of them (layer 0 of the shipped shape: 66 MB read + 33 MB written, three times per pass).  Packed once
  // per pass now, by a task of its own that nothing but the layer's first projection waits for -- and the A pack of the layers
  // >= 1 takes nn.GRU's inter-layer dropout with it (one kernel where there were dropout, pack A, pack B in front of the GEMM:
  // a stage of the layer wavefront is sweep -> pack -> GEMM -> sweep).  Same values, same rounding: bit-identical.
  const bool prepack_env = !(getenv("B2T_PREPACK") && atoi(getenv("B2T_PREPACK")) == 0);   // read per pass (the tests compare the two forms in one process)
  int t_wpk[MAXL];
  bool wpk_ok[MAXL];
  for (int l = 0; l < L; ++l) {
    t_wpk[l] = -1; wpk_ok[l] = false;
    if (!c.bf16_gemm || !prepack_env || !w.wpk_f[l] || fused_from(l - 1) || (wave && l > 0)) continue;
    const int n0 = chunks[0][1] - chunks[0][0], nl = chunks[nc - 1][1] - chunks[nc - 1][0];
    b2t_gemm_desc d0 = gd(nullptr, prm->w_ih[l], nullptr, std::min(n0, nl) * B, 3 * H, l == 0 ? In0 : H);   // the smallest chunk decides
    if (!c.pack_shape_ok(d0) || (l == 0 && !((long long)std::min(n0, nl) * B > 512))) continue;
    wpk_ok[l] = true;
    t_wpk[l] = P.add("wpack", 15.f, Q_ANY, {t_start}, [&, l](hipStream_t s) {
      b2t_gemm_desc d = gd(nullptr, prm->w_ih[l], nullptr, 128, 3 * H, l == 0 ? In0 : H);
      d.b_s0 = l == 0 ? In0 : H;
      c.call(gemm_bf16p_pack(&d, 1, w.wpk_f[l], s));
    });
  }
  int t_hfin = -1;      // wavefront: the task that copies the final states out
  int t_gi_l0c[MAXC];   // wavefront: layer 0's projection task of every chunk (the only projections left)
  for (int i = 0; i < MAXC; ++i) t_gi_l0c[i] = -1;
  for (int l = 0; l < L; ++l) {
    for (int ci = 0; ci < nc; ++ci) {
      const int t0 = chunks[ci][0], t1 = chunks[ci][1], n = t1 - t0;
      // 2. input projection gi = in_t W_ih^T + b_ih for this chunk, time-major [T'][B][3H]
      const int t_gi = fused_from(l - 1) ? t_sw[l - 1][ci] : (wave && l > 0) ? -1 :
                       P.add("gi", est_gemm((double)n * B, 3 * H, l == 0 ? In0 : H), Q_ANY, {l == 0 ? t_day[ci] : t_sw[l - 1][ci], t_wpk[l]},
                             [&, l, t0, n](hipStream_t sg) {
        if (l == 0) {
          static const bool rowmap = !(getenv("B2T_L0_ROWMAP") && atoi(getenv("B2T_L0_ROWMAP")) == 0);
          if ((c.bf16_gemm || rowmap) && (long long)n * B > 512) {
            // ONE row-mapped GEMM over all (t, b) rows of the chunk instead of B per-sentence GEMMs.  amp mode: so that it takes
            // the two-pass packed kernel (Z == 1).  fp32 (late round 3): a per-sentence GEMM of a time chunk has M = 83 rows, i.e.
            // one 128-row tile of which 35 % is padding -- 4608 tiles per step where 3024 dense ones do: 19.24-19.38 -> 18.94-19.12 ms
            // per step, same results bit for bit (B2T_L0_ROWMAP=0: the per-sentence form)
            b2t_gemm_desc d = gd(w.Ud + (long long)t0 * a_s0_l0, prm->w_ih[0], w.gi[0] + (long long)t0 * B * 3 * H, n * B, 3 * H, In0);
            d.a_div = B; d.a_s1 = a_s0_l0; d.a_s0 = (long long)T * F; d.b_s0 = In0; d.c_s0 = 3 * H; d.bias = prm->b_ih[0];
            if (wpk_ok[0] && c.would_pack(d, sg)) c.gemm(sg, d, 1, nullptr, 0, -1, w.wpk_f[0]);
            else c.gemm(sg, d);
          } else if ((long long)n * B <= 512 && In0 >= 2048) {
            // streaming-sized calls (a few frames, patch input K = 7168): one GEMM over all (t, b) rows through the
            // two-level row map, K split over the chip (as B per-sentence GEMMs the K loop runs serially in 18 workgroups)
            b2t_gemm_desc d = gd(w.Ud + (long long)t0 * a_s0_l0, prm->w_ih[0], w.gi[0] + (long long)t0 * B * 3 * H, n * B, 3 * H, In0);
            d.a_div = B; d.a_s1 = a_s0_l0; d.a_s0 = (long long)T * F; d.b_s0 = In0; d.c_s0 = 3 * H; d.bias = prm->b_ih[0];
            if (skinny(n * B, In0)) c.gemm(sg, d);   // <= 64 rows: the weight-streaming kernel inside b2t_gemm_f32, one launch
            else c.gemm(sg, d, std::max(1, std::min(16, In0 / 448)), w.slab_gi[0]);
          } else if (In0 >= 2048 && nc == 1) {
            // patch input at full size (shipped shape: 7808 x 2304 x 7168): 61 x 18 = 1098 tiles are 1.07 waves of the chip's
            // 1024 tile slots, i.e. the second wave runs almost empty (92 TF/s).  Three K slices make 3.2 waves of shorter
            // tiles: 114 TF/s incl. the slab reduction (attic/bench_gemm_c3.py); one row-mapped GEMM over all (t, b) rows.
            b2t_gemm_desc d = gd(w.Ud + (long long)t0 * a_s0_l0, prm->w_ih[0], w.gi[0] + (long long)t0 * B * 3 * H, n * B, 3 * H, In0);
            d.a_div = B; d.a_s1 = a_s0_l0; d.a_s0 = (long long)T * F; d.b_s0 = In0; d.c_s0 = 3 * H; d.bias = prm->b_ih[0];
            c.gemm(sg, d, 3, w.slab_gi[0]);
          } else {
            b2t_gemm_desc d = gd(w.Ud + (long long)t0 * a_s0_l0, prm->w_ih[0], w.gi[0] + (long long)t0 * B * 3 * H, n, 3 * H, In0);
            d.Z = B; d.a_s0 = a_s0_l0; d.a_sz = (long long)T * F; d.b_s0 = In0; d.c_s0 = (long long)B * 3 * H; d.c_sz = 3 * H;
            d.bias = prm->b_ih[0];
            c.gemm(sg, d);
          }
          return;
        }
        const float* src = w.out[l - 1];
        const bool drop = w.outd[l - 1] != w.out[l - 1];   // nn.GRU inter-layer dropout (rnn_model.py:70)
        {
          b2t_gemm_desc d = gd(w.out[l - 1] + (long long)(1 + t0) * B * H, prm->w_ih[l], w.gi[l] + (long long)t0 * B * 3 * H, n * B, 3 * H, H);
          d.a_s0 = H; d.b_s0 = H; d.c_s0 = 3 * H; d.bias = prm->b_ih[l];
          if (wpk_ok[l] && c.would_pack(d, sg) && (!drop || H % 8 == 0)) {
            // pre-packed weights; the dropout rides in the A pack, which also writes the dropped fp32 values the backward pass reads
            PackDrop pd{drop ? p->rnn_drop : 0.f, mix_seed(p->seed, 101 + (l - 1)), (long long)t0 * B * H, w.outd[l - 1] + (long long)(1 + t0) * B * H};
            c.gemm(sg, d, 1, nullptr, 0, -1, w.wpk_f[l], drop ? &pd : nullptr);
            return;
          }
        }
        if (drop) {
          c.call(b2t_dropout_f32(w.out[l - 1] + (long long)(1 + t0) * B * H, w.outd[l - 1] + (long long)(1 + t0) * B * H,
                                 (long long)n * B * H, p->rnn_drop, mix_seed(p->seed, 101 + (l - 1)), (long long)t0 * B * H,
                                 reinterpret_cast<void*>(sg)));
          src = w.outd[l - 1];
        }
        b2t_gemm_desc d = gd(src + (long long)(1 + t0) * B * H, prm->w_ih[l], w.gi[l] + (long long)t0 * B * 3 * H, n * B, 3 * H, H);
        d.a_s0 = H; d.b_s0 = H; d.c_s0 = 3 * H; d.bias = prm->b_ih[l];
        const bool small = (long long)n * B <= 512 && H >= 384;   // streaming-sized call: split K (one 128-row tile otherwise)
        if (small && !skinny(n * B, H)) c.gemm(sg, d, std::max(1, H / 192), w.slab_gi[l]);
        else c.gemm(sg, d);
      });
      // Layer 0 of a patch model in the bf16 mode: the chunks' projections (2624 x 2304 x 7168 each at the shipped shape: 150 us alone) are
      // all ready behind the day layer; launched together on three queues they share the chip and the FIRST one -- the only one the
      // first sweep waits for -- finishes after 290 us.  Chained one after the other the first sweep starts 150 us earlier and the step is
      // SLOWER (5.85 against 5.81 ms: the later chunks' GEMMs then run next to the sweeps instead of in front of them; NOTES.md R5.7).
      if (wave) {
        // 3w. the layer wavefront: ONE task per time chunk for the whole stack, created with the top layer (it needs every layer's
        // initial state).  Chunks are launches one behind the other on a sweep queue: the only thing pipelined over them is what runs
        // NEXT to the sweeps on the CUs they leave free (layer 0's projection of the next chunk; in the backward pass the weight
        // gradients of the chunk before).
        if (l == 0) t_gi_l0c[ci] = t_gi;
        if (l + 1 < L) { t_sw[l][ci] = -1; continue; }
        const int t_ws = P.add("wsweep", 60.f + (n + 2 * L) * est_step_us(0) * hs, q_sweep, {t_gi_l0c[ci], ci > 0 ? t_sw[L - 1][ci - 1] : -1}, [&, t0, t1, n](hipStream_t ss) {
          if (c.rc) return;
          Ctx::Scope sc(c, ss, 8, 2.0 * n * B * 3.0 * H * H * (2 * L - 1));
          WaveFwdArgs a;
          memset(&a, 0, sizeof(a));
          a.L = L; a.T = n; a.B = B; a.H = H; a.gi0 = w.gi[0] + (long long)t0 * B * 3 * H;
          const bool drop = p->rnn_drop > 0.f && L > 1;
          for (int k = 0; k < L; ++k) {
            a.w_hh[k] = prm->w_hh[k]; a.b_hh[k] = prm->b_hh[k]; a.w_ih[k] = prm->w_ih[k]; a.b_ih[k] = prm->b_ih[k];
            a.h_init[k] = (t0 == 0 && states && !p->save) ? states + (size_t)k * B * H : w.out[k] + (long long)t0 * B * H;
            a.out[k] = w.out[k] + (long long)(1 + t0) * B * H;
            a.outd[k] = (drop && k + 1 < L) ? w.outd[k] + (long long)(1 + t0) * B * H : nullptr;
            a.reserve[k] = p->save ? w.res[k] + (long long)t0 * B * 4 * H : nullptr;
            a.ring[k] = w.wv_ring_f[k]; a.ringd[k] = w.wv_ringd_f[k];
            a.seed[k] = mix_seed(p->seed, 101 + k);
          }
          a.cnt = w.wv_cnt_f; a.err = reinterpret_cast<unsigned*>(sync_of(0));
          a.drop_p = drop ? p->rnn_drop : 0.f; a.drop_scale = drop ? 1.0f / (1.0f - p->rnn_drop) : 1.f; a.elem0 = (long long)t0 * B * H;
          c.call(gru_wave_fwd(a, ss));
        });
        for (int k = 0; k < L; ++k) { t_sw[k][ci] = t_ws; if (ci == 0) P.dep(t_ws, t_init[k]); }
        // the final states: a task of its own (the five copies, ~40 us, sat between the sweep and the head on the sweep's queue)
        if (t1 == Tp)
          t_hfin = P.add("hfinal", 40.f, Q_ANY, {t_ws}, [&](hipStream_t ss) {
            for (int k = 0; k < L && !c.rc; ++k)
              c.call(check_hip(hipMemcpyAsync(hidden + (size_t)k * B * H, w.out[k] + (long long)Tp * B * H, sizeof(float) * B * H, hipMemcpyDeviceToDevice, ss), "model_forward: final state"));
          });
        continue;
      }
      // 3. recurrent sweep over the chunk, continuing from out[l][t0] = h_{t0-1}
      t_sw[l][ci] = P.add("sweep", 40.f + n * est_step_us(0) * hs, q_sweep, {t_gi, ci > 0 ? t_sw[l][ci - 1] : t_init[l]}, [&, l, t0, t1, n, ci](hipStream_t ss) {
        if (c.rc) return;
        const bool fused = fused_from(l);
        Ctx::Scope sc(c, ss, 8, (fused ? 2.0 : 1.0) * 2.0 * n * B * 3.0 * H * H);
        // h_{t0-1}: slot t0 of out[l] -- or, for the first chunk of an inference pass with carried state, the caller's buffer
        const float* h_prev = (t0 == 0 && states && !p->save) ? states + (size_t)l * B * H : w.out[l] + (long long)t0 * B * H;
        if (fused) {
          const int mf = (mode & ~(0xff | B2T_GRU_WIDE)) | 1;
          c.call(b2t_gru_layer_fwd_fused_f32(w.gi[l] + (long long)t0 * B * 3 * H, prm->w_hh[l], prm->b_hh[l], h_prev,
                                             w.out[l] + (long long)(1 + t0) * B * H, p->save ? w.res[l] + (long long)t0 * B * 4 * H : nullptr,
                                             t1 == Tp ? hidden + (size_t)l * B * H : nullptr, prm->w_ih[l + 1], prm->b_ih[l + 1],
                                             w.gi[l + 1] + (long long)t0 * B * 3 * H, n, B, H,
                                             (mf & B2T_GRU_LOCAL) ? (mf | ((l & 1) ? B2T_GRU_PARITY : 0)) : mf, sync_of(l),
                                             reinterpret_cast<void*>(ss)));
          return;
        }
        // In the wavefront's fill and drain stages, where at most B2T_NARROW_EDGE (default 2) layers are at work, the exact-fp32
        // sweep runs with 16-unit workgroups (twice the workgroups, half the MFMA time per step: the chip is mostly empty there
        // and the stage is pure latency) instead of the 32-unit ones that crowd the CUs less in the full stages:
        // 19.51-19.57 -> 19.36-19.39 ms per step (k = 1: 19.40-19.42, k = 3: 19.52-19.56; 0 = off).  Same results bit for bit.
        static const int narrow_edge = getenv("B2T_NARROW_EDGE") ? atoi(getenv("B2T_NARROW_EDGE")) : 2;
        int m2 = mode;
        if (narrow_edge > 0 && (mode & B2T_GRU_WIDE) && !(mode & B2T_GRU_BF16) && nc > 1) {
          const int stage = l + ci, active = std::min(std::min(stage + 1, L + nc - 1 - stage), std::min(L, nc));
          if (active <= narrow_edge) m2 &= ~B2T_GRU_WIDE;   // (fill stages only: 19.38-19.50, drain only: 19.25-19.35, both: 19.17-19.39)
        }
        // next to the fused sweeps of the layers below (256 registers per lane, two per CU) only a 16-unit workgroup (168) fits a CU
        if (fuse_ok) m2 &= ~B2T_GRU_WIDE;
        c.call(b2t_gru_layer_fwd_f32(w.gi[l] + (long long)t0 * B * 3 * H, prm->w_hh[l], prm->b_hh[l], h_prev,
                                     w.out[l] + (long long)(1 + t0) * B * H, p->save ? w.res[l] + (long long)t0 * B * 4 * H : nullptr,
                                     t1 == Tp ? hidden + (size_t)l * B * H : nullptr, n, B, H,
                                     (m2 & B2T_GRU_LOCAL) ? (m2 | ((l & 1) ? B2T_GRU_PARITY : 0)) : m2, sync_of(l),
                                     reinterpret_cast<void*>(ss)));
      });
      if (mode & B2T_GRU_LOCAL) P.t[t_sw[l][ci]].cls = l & 1;   // XCD set by layer parity: admission-controlled (run_plan)
    }
  }
  // 4. head: logits[b,t,:] = out W^T + b  (rnn_model.py:129), written batch-first
  const int t_head = P.add("head", est_gemm((double)Tp * B, Cc, H), Q_ANY, {t_sw[L - 1][nc - 1]}, [&](hipStream_t s) {
    b2t_gemm_desc d = gd(w.out[L - 1] + (long long)B * H, prm->out_w, logits, Tp * B, Cc, H);
    d.a_s0 = H; d.b_s0 = H; d.c_div = B; d.c_s1 = Cc; d.c_s0 = (long long)Tp * Cc; d.bias = prm->out_b;
    c.gemm(s, d);
  });
  // the caller's stream leaves ordered after everything: the head transitively depends on every sweep and GEMM except
  // the last chunks of the lower layers' sweeps (their final hidden state)
  {
    const int t_end = P.add("end", 0.f, Q_MAIN, {t_head, t_hfin}, nullptr);
    for (int l = 0; l + 1 < L; ++l) P.dep(t_end, t_sw[l][nc - 1]);
  }
  run_plan(c, P, c.nq, c.qs);
  return c.rc;
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
namespace b2t {
namespace {

// dW_hh = dGh^T h_prev, dW_ih = dGi^T in, bias gradients = column sums of dG (layer l) over the time rows [t0, t1):
// the whole sequence at once (t0 = 0, t1 = T', accumulate = 0), or chunk by chunk as soon as a chunk is swept (the first
// chunk processed overwrites, later ones accumulate in a fixed order: deterministic); `final` copies the bias sums out.
// which: 3 = the GEMMs (default); 1 = only pack their B operands (h_{t-1}^T -> w.xpk_hh[l], x^T -> w.xpk_ih[l]; bf16 mode, whole
// sequence: round 5) -- a later call with pre = true then multiplies by the packed copies.
// part: 0 = both weight gradients of the layer, one after the other (shared slab / sums); 1 = dW_hh (+ b_hh) only, with buffers of
// its own (w.slab_hh / w.asum_hh), 2 = dW_ih (+ b_ih) only: the two as separate tasks of the plan (bf16 mode, round 5).
void layer_weight_grads(Ctx& c, hipStream_t s, const b2t_model_t* prm, const b2t_model_t* grd, const b2t_pass_t* p,
                        Layout& w, int l, int t0, int t1, int accumulate, bool final, int which = 3, bool pre = false, int part = 0) {
  const int B = p->B, T = p->T, F = prm->F, H = prm->H;
  const long long K = (long long)(t1 - t0) * B;
  const long long a0 = (long long)t0 * B * 4 * H;
  void* sp = reinterpret_cast<void*>(s);
  // fp32: the bias gradients (column sums of dGh -> b_hh, of dGi -> b_ih) are by-products of the two GEMMs that read dG
  // as their A operand (per-slice sums, reduced in slice order); bf16 GEMMs and odd H take a column-sum pass over dG
  static const bool no_fused = getenv("B2T_NO_FUSED_BIAS") != nullptr;   // A/B knob
  bool fused_bias = !no_fused && (2 * H) % 128 == 0 && (3 * H) % 128 == 0;
  if (fused_bias && c.bf16_gemm) {   // bf16 GEMMs: the pack pass of the two-pass kernel sums (one slice per 64 k); the one-pass kernel does not
    b2t_gemm_desc a = gd(nullptr, nullptr, nullptr, 3 * H, H, (int)K), b = gd(nullptr, nullptr, nullptr, 3 * H, l == 0 ? in0(prm) : H, (int)K);
    b.a_brk = 2 * H;
    fused_bias = c.would_pack(a, s) && c.would_pack(b, s);
  }
  float* const asum_x = part == 1 ? w.asum_hh[l] : w.asum[l];
  float* const slab_x = part == 1 ? w.slab_hh[l] : w.slab[l];
  auto bias_out = [&](int sk, float* dst) {
    const int ns = c.bf16_gemm ? (int)((K + 63) / 64) : std::max(1, sk);
    c.call(b2t_colsum_f32(asum_x, ns, 3 * H, 3 * H, dst, accumulate, asum_x + (size_t)ns * 3 * H, 1, 0, 0, sp));
  };
  if (part != 2) {
    b2t_gemm_desc d = gd(w.dG[l] + a0, w.out[l] + (long long)t0 * B * H, grd->w_hh[l], 3 * H, H, (int)K);
    d.a_kcontig = 0; d.a_s0 = 4 * H; d.b_kcontig = 0; d.b_s0 = H; d.c_s0 = H;
    const int sk = splitk_for(3 * H, H, K, splitk_target(c.bf16_gemm));
    if (which == 1) { c.call(gemm_bf16p_pack(&d, 1, w.xpk_hh[l], s)); }
    else {
      if (fused_bias) { d.a_sum = asum_x; d.a_sum_ks = 3 * H; }
      // (the pre-packed copy only where this queue has pack scratch: with B2T_WORKERS > 3 a task can land on a queue without --
      //  the GEMM then takes the one-pass kernel on the raw operand, as before round 5)
      c.gemm(s, d, sk, slab_x, accumulate, l, (pre && c.would_pack(d, s)) ? w.xpk_hh[l] : nullptr);
      if (fused_bias) bias_out(sk, grd->b_hh[l]);
    }
  }
  if (part == 1) return;     // (only taken with fused bias sums: the caller checks)
  int In; const float* inp; long long b_s0, b_s1 = 0; int b_div = 0;
  if (l == 0) {
    In = in0(prm);
    b_div = B; b_s1 = prm->patch > 0 ? (long long)prm->stride * F : F; b_s0 = (long long)T * F;
    inp = w.Ud + (long long)t0 * b_s1;
  } else {
    In = H; inp = w.outd[l - 1] + (long long)(1 + t0) * B * H;   // skip the initial-state slot
    b_s0 = H;
  }
  auto wih = [&](int M, long long a_off, long long c_off, int brk, int gap) {
    b2t_gemm_desc d = gd(w.dG[l] + a0 + a_off, inp, grd->w_ih[l] + c_off, M, In, (int)K);
    d.a_kcontig = 0; d.a_s0 = 4 * H; d.b_kcontig = 0; d.b_s0 = b_s0; d.b_s1 = b_s1; d.b_div = b_div; d.c_s0 = In;
    d.a_brk = brk; d.a_gap = gap;
    const int sk = splitk_for(M, In, K, splitk_target(c.bf16_gemm));
    if (which == 1) { c.call(gemm_bf16p_pack(&d, 1, w.xpk_ih[l], s)); return; }
    if (fused_bias) { d.a_sum = w.asum[l]; d.a_sum_ks = 3 * H; }
    c.gemm(s, d, sk, w.slab[l], accumulate, l, (pre && c.would_pack(d, s)) ? w.xpk_ih[l] : nullptr);
    if (fused_bias) bias_out(sk, grd->b_ih[l]);
  };
  if ((2 * H) % 128 == 0 && (3 * H) % 128 == 0) {   // dGi^T as ONE operand with a gap along m
    wih(3 * H, 0, 0, 2 * H, H);
  } else {
    wih(2 * H, 0, 0, 0, 0);
    wih(H, 3 * H, (long long)2 * H * In, 0, 0);
  }
  if (fused_bias || which == 1) return;
  c.call(b2t_colsum_f32(w.dG[l] + a0, K, 4 * H, 4 * H, w.s4[l], accumulate, w.cs_layer[l], 1, 0, 0, sp));   // (s_r, s_z, s_nr, s_n)
  if (!final) return;
  auto cp = [&](float* dst, const float* src, size_t n) {
    c.call(check_hip(hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s), "model_backward: bias gradient copy"));
  };
  cp(grd->b_ih[l], w.s4[l], 2 * H);
  cp(grd->b_ih[l] + 2 * H, w.s4[l] + 3 * H, H);
  cp(grd->b_hh[l], w.s4[l], 3 * H);
}

}  // namespace
}  // namespace b2t

extern "C" int b2t_model_backward(b2t_exec* ex, const b2t_model_t* prm, const b2t_model_t* grd, const b2t_pass_t* p,
                                  const float* x, const int32_t* day_idx, const float* dlogits, int ldd,
                                  const float* dhidden, float* dstates, int custom_states, void* ws, void* sync_ws,
                                  b2t_bucket_cb bucket_cb, void* user, void* stream) {
  { int rc = check_common(ex, prm, p, "model_backward"); if (rc) return rc; }
  B2T_REQUIRE(grd && x && day_idx && dlogits && ws && p->save, "model_backward: null buffer / forward ran without save");
  B2T_REQUIRE(ldd >= prm->C && ldd % 4 == 0, "model_backward: ldd=%d must be a multiple of 4 and >= C", ldd);
  const int B = p->B, T = p->T, F = prm->F, H = prm->H, L = prm->L, Cc = prm->C;
  const int Tp = out_T(prm, T), In0 = in0(prm);
  const long long M = (long long)Tp * B;
  const int mode = p->bwd_mode;
  B2T_REQUIRE((mode & 0xff) == 0 || sync_ws, "model_backward: sync_ws is required for the persistent sweeps");
  Layout w;
  carve(prm, p, reinterpret_cast<char*>(ws), w);
  Ctx c{ex, as_stream(stream), p->bf16_gemm != 0};
  c.lay = &w;
  ex->next_ev = 0;
  const size_t sync_block = b2t_gru_sync_bytes(0);
  auto sync_of = [&](int l) { return sync_ws ? reinterpret_cast<char*>(sync_ws) + (size_t)(L + l) * sync_block : nullptr; };
  static_assert((MAXL + 1) * KSLOT + 64 <= 2 * 64 * 1024, "split-K tile counters must fit one sync block");
  if (sync_ws) c.kcnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(sync_ws) + (size_t)2 * L * sync_block) + 64;
  auto cb = [&](int id, hipStream_t s) { if (bucket_cb && !c.rc) bucket_cb(user, id, reinterpret_cast<void*>(s)); };

  const bool wave = wave_pass(prm, p, mode) && w.wv_cnt_b;   // round 6: every layer's backward sweep in ONE launch (gru_wave.hip), dX of the layers >= 1 inside it
  // K-split form of the wavefront: the sweep reads the weight matrices as they are -- no transposes (and no queue hop) in front of it
  const bool ks_direct = wave && gru_wave_ks(L, Tp, B, H);
  int chunks[MAXC][2];
  const int nc = make_chunks(Tp, p->chunks_bwd > 0 ? p->chunks_bwd : p->chunks, chunks);
  c.exact_k = nc > 1;
  c.nq = plan_queues(c, nc > 1 || wave, c.qs);   // the queues of this pass (the plan below refers to them by index)
  // (data parallel: the bucket callbacks issue collectives from inside the plan -- not replayable)
  if (!bucket_cb) c.gkey = pass_key(2, prm, grd, p, {x, day_idx, dlogits, dhidden, dstates, ws, sync_ws, stream}, {c.nq, ldd, custom_states});
  // (One chunk -- shapes whose sweeps cannot be co-resident, e.g. H = 768 -- runs everything on the caller's stream.  Putting
  // the weight-gradient GEMMs of layer l on a side stream under the sweep of layer l - 1 was measured: C3 fp32 19.7 -> 23.0 ms,
  // bf16 operands 12.7 -> 15.1 ms: a 768-unit sweep workgroup needs a CU's whole register file, and GEMM workgroups that
  // arrive first keep its row group from becoming resident.)
  const float hs = std::max(0.25f, (float)H * H / (512.f * 512.f)) * std::max(1, (B + 63) / 64);
  const unsigned q_sweep = ex->sweep_qmask;

  Plan P;
  const int t_start = P.add("start", 0.f, Q_MAIN, {}, nullptr);
  // head: d_out[t,b,:] = dlogits[b,t,:] W_out ; dW_out = dlogits^T out ; db_out = colsum
  const int t_top = P.add("head_dx", est_gemm((double)M, H, Cc), Q_ANY, {t_start}, [&](hipStream_t s) {
    b2t_gemm_desc d = gd(dlogits, prm->out_w, w.dY[L - 1], (int)M, H, Cc);
    d.a_div = B; d.a_s1 = ldd; d.a_s0 = (long long)Tp * ldd; d.b_kcontig = 0; d.b_s0 = H; d.c_s0 = H;
    c.gemm(s, d);
  });
  // Gradient buckets reach the data-parallel reducer through tiny tasks of their own, chained in a fixed order (head,
  // layers L-1 .. 0, day, h0 -- every rank must start its collectives in the same order whatever its batch length did to
  // the schedule); the GEMMs that fill the buckets stay free to run wherever and whenever the scheduler finds room.
  int t_bucket = -1;
  auto bucket = [&](int id, int producer) {
    if (!bucket_cb) return;
    // (the callback may issue a collective that BLOCKS this queue until every peer has arrived: the estimate is the slack the
    //  scheduler leaves behind it -- work it would have queued there goes to another queue; B2T_BUCKET_EST_US, NOTES.md R6.3)
    static const float est_b = getenv("B2T_BUCKET_EST_US") ? (float)atof(getenv("B2T_BUCKET_EST_US")) : 600.f;   // measured: 1 / 200 / 600 / 1000 / 1500 / 3000 us -> 20.8 / 20.8 / 19.5 / 20.1 / 20.3 / 20.5 ms with every collective 0.5 ms late (18.9 on time)
    t_bucket = P.add("bucket", est_b, Q_ANY, {producer, t_bucket}, [&, id](hipStream_t s) { cb(id, s); });
  };
  const int t_head_w = P.add("head_w", est_gemm(Cc, H, (double)M) + 40.f, Q_ANY, {t_start}, [&](hipStream_t s) {
    b2t_gemm_desc d = gd(dlogits, w.out[L - 1] + (long long)B * H, grd->out_w, Cc, H, (int)M);
    d.a_kcontig = 0; d.a_div = B; d.a_s1 = ldd; d.a_s0 = (long long)Tp * ldd; d.b_kcontig = 0; d.b_s0 = H; d.c_s0 = H;
    c.gemm(s, d, splitk_for(Cc, H, M, splitk_target(c.bf16_gemm)), w.slab_head, 0, MAXL);
    c.call(b2t_colsum_f32(dlogits, M, Cc, ldd, grd->out_b, 0, w.cs_head, 1, 0, 0, reinterpret_cast<void*>(s)));
  });
  bucket(0, t_head_w);
  // W_hh^T for the backward sweeps depends on the parameters only
  int t_wt[MAXL];
  for (int l = 0; l < L; ++l)
    t_wt[l] = ks_direct ? -1 : P.add("whh_t", 8.f, Q_ANY, {t_start}, [&, l](hipStream_t s) {
      c.call(b2t_transpose_f32(prm->w_hh[l], w.whh_t[l], 3 * H, H, reinterpret_cast<void*>(s)));
    });

  // wavefront: W_ih^T of the layers >= 1 (the B operand of dY[l - 1] = dGi[l] W_ih[l], made inside the sweep)
  int t_wit[MAXL];
  for (int l = 0; l < L; ++l) {
    t_wit[l] = -1;
    if (wave && l > 0 && !ks_direct)
      t_wit[l] = P.add("wih_t", 8.f, Q_ANY, {t_start}, [&, l](hipStream_t s) {
        c.call(b2t_transpose_f32(prm->w_ih[l], w.wih_t[l], 3 * H, H, reinterpret_cast<void*>(s)));
      });
  }
  // dIn = dGi W_ih for rows of chunk [t0, t0+n): into dY[l-1] (l > 0) or dU / dV (l == 0).
  // Day-layer backward chunk by chunk (no patching, no input dropout): the Softsign backward rides in the epilogue of
  // layer 0's dX GEMM, the per-sample day-gradient GEMM and bias sums accumulate chunk after chunk behind it, so that
  // only the last chunk's share is left behind the last backward sweep (it was 1.4 ms of tail as whole-sequence passes).
  const bool fast_day = prm->patch == 0 && !(p->in_drop > 0.f);
  const long long bias_ld = (long long)align_up(F, 4);
  // bf16 mode (round 5): W_ih^T of every layer, the B operand of its input-gradient GEMM, packed once per pass (see b2t_model_forward)
  const bool prepack_env = !(getenv("B2T_PREPACK") && atoi(getenv("B2T_PREPACK")) == 0);   // read per pass (the tests compare the two forms in one process)
  // (measured NEGATIVE, opt-in: the shipped shape's bf16 step 6.20 ms against 6.00, C2 bf16 9.95 against 9.81 -- the layers' small dW_hh
  //  GEMMs then start next to the sweeps still running, and a sweep next to a GEMM is the slower sweep: NOTES.md R5.7)
  const bool split_env = getenv("B2T_WGRAD_SPLIT") && atoi(getenv("B2T_WGRAD_SPLIT")) == 1;
  int t_wpk[MAXL];
  bool wpk_ok[MAXL];
  for (int l = 0; l < L; ++l) {
    t_wpk[l] = -1; wpk_ok[l] = false;
    if (!c.bf16_gemm || !prepack_env || !w.wpk_b[l] || (wave && l > 0)) continue;
    const int nmin = std::min(chunks[0][1] - chunks[0][0], chunks[nc - 1][1] - chunks[nc - 1][0]);
    b2t_gemm_desc d0 = gd(nullptr, prm->w_ih[l], nullptr, nmin * B, l > 0 ? H : In0, 3 * H);
    d0.a_brk = 2 * H;
    if (!c.pack_shape_ok(d0)) continue;
    wpk_ok[l] = true;
    t_wpk[l] = P.add("wpack", 15.f, Q_ANY, {t_start}, [&, l](hipStream_t s) {
      const int N = l > 0 ? H : In0;
      b2t_gemm_desc d = gd(nullptr, prm->w_ih[l], nullptr, 128, N, 3 * H);
      d.b_kcontig = 0; d.b_s0 = N;
      c.call(gemm_bf16p_pack(&d, 1, w.wpk_b[l], s));
    });
  }
  auto dx_gemm = [&](hipStream_t s, int l, int t0, int n) {
    // dGi = dG[:, 0:2H] ++ dG[:, 3H:4H] is ONE A operand with a gap at k = 2H (H % 16 == 0 makes 2H a multiple of the k tile)
    const int N = l > 0 ? H : In0;
    b2t_gemm_desc d = gd(w.dG[l] + (long long)t0 * B * 4 * H, prm->w_ih[l], nullptr, n * B, N, 3 * H);
    d.a_s0 = 4 * H; d.b_kcontig = 0; d.b_s0 = N; d.a_brk = 2 * H; d.a_gap = H;
    if (l > 0) { d.C = w.dY[l - 1] + (long long)t0 * B * H; d.c_s0 = H; }
    else if (prm->patch > 0) { d.C = w.dV + (long long)t0 * In0; d.c_div = B; d.c_s1 = In0; d.c_s0 = (long long)Tp * In0; }
    else {
      d.C = w.dU + (long long)t0 * F; d.c_div = B; d.c_s1 = F; d.c_s0 = (long long)T * F;
      if (fast_day) { d.epilogue = 2; d.ep_aux = w.U + (long long)t0 * F; }   // dpre = dU * (1 - |U|)^2
    }
    // Serial plan (shapes whose sweeps cannot share the chip, e.g. the shipped H = 768): the whole sequence's dX of a layer is
    // 61 x 6 = 366 tiles, a third of the chip's tile slots -- two K slices fill it (79 -> 100 TF/s incl. the slab reduction,
    // attic/bench_gemm_c3.py).  Pipelined plans share the CUs with the sweeps anyway (measured neutral there).
    const long long tiles = (((long long)n * B + 127) / 128) * ((N + 127) / 128);
    if (l > 0 && nc == 1 && !c.bf16_gemm && w.slab_dx && tiles <= 512 && 3 * H >= 1024) c.gemm(s, d, 2, w.slab_dx);
    else if (wpk_ok[l] && c.would_pack(d, s)) c.gemm(s, d, 1, nullptr, 0, -1, w.wpk_b[l]);
    else c.gemm(s, d);
    // The day layer's weight gradient (per-sentence x^T dpre, then the reduction by day) ONCE over the whole sequence behind the
    // last chunk instead of chunk by chunk: the per-chunk GEMMs had K = 125 (14 TF/s, and 128 MB of slab read-modify-write
    // each) and four column-sum passes -- 1.9 ms of queue time per step for 17 GFLOP; as one K = 500 GEMM it adds ~0.3 ms to the
    // tail and the step goes from 18.90-19.05 to 18.75-18.88 ms (B2T_DAY_WGRAD_LATE=0: per chunk)
    static const bool day_late = !(getenv("B2T_DAY_WGRAD_LATE") && atoi(getenv("B2T_DAY_WGRAD_LATE")) == 0);
    if (l == 0 && fast_day && !day_late) {
      const int first = t0 + n == Tp ? 0 : 1;   // the top time chunk is swept first: it overwrites, the others accumulate
      b2t_gemm_desc d = gd(x + (long long)t0 * F, w.dU + (long long)t0 * F, w.day_slab, F, F, n);
      d.Z = B; d.a_kcontig = 0; d.a_s0 = F; d.a_sz = (long long)T * F; d.b_kcontig = 0; d.b_s0 = F; d.b_sz = (long long)T * F;
      d.c_s0 = F; d.c_sz = (long long)F * F;
      c.gemm(s, d, 1, nullptr, first);
      c.call(b2t_colsum_f32(w.dU + (long long)t0 * F, n, F, F, w.day_bslab, first, w.cs_day, B, (long long)T * F, bias_ld,
                            reinterpret_cast<void*>(s)));
    }
  };

  // Weight gradients: per chunk (bit l of wgrad_chunk_mask: the first chunk swept overwrites, the others accumulate in sweep
  // order -- a dependency chain, so the sums do not depend on the schedule) or once per layer after its last chunk.
  int t_bs[MAXL][MAXC], t_dx[MAXL][MAXC], t_wg_last[MAXL];
  int t_wbc[MAXC];                // wavefront: the sweep task of each time chunk
  for (int ci = 0; ci < MAXC; ++ci) t_wbc[ci] = -1;
  // Wavefront with more than one time chunk: one sweep launch per chunk, last chunk first, each behind the one before (the state
  // gradient crosses in w.carry); a chunk's consumers -- layer 0's input gradient, every layer's weight gradients -- are ordinary
  // successors of that launch and run BESIDE the next chunk's sweep on the CUs it leaves free.  (One launch for the whole sequence
  // with consumers gated on the device measured slower at every chunk count: NOTES.md R6.2b.)
  // one sweep launch of the whole stack over the steps [t0, t0 + n)
  auto wave_sweep = [&, dhidden](hipStream_t ss, int ci, int t0, int n) {
    if (c.rc) return;
    Ctx::Scope sc(c, ss, 9, 2.0 * n * B * 3.0 * H * H * (2 * L - 1));
    WaveBwdArgs a;
    memset(&a, 0, sizeof(a));
    a.L = L; a.T = n; a.B = B; a.H = H; a.dY_top = w.dY[L - 1] + (long long)t0 * B * H;
    const bool drop = p->rnn_drop > 0.f && L > 1;
    for (int k = 0; k < L; ++k) {
      a.w_hh_t[k] = ks_direct ? prm->w_hh[k] : w.whh_t[k]; a.w_ih_t[k] = ks_direct ? prm->w_ih[k] : w.wih_t[k];
      a.h_init[k] = w.out[k] + (long long)t0 * B * H; a.out[k] = w.out[k] + (long long)(1 + t0) * B * H;
      a.reserve[k] = w.res[k] + (long long)t0 * B * 4 * H; a.dG[k] = w.dG[k] + (long long)t0 * B * 4 * H;
      a.ring[k] = w.wv_ring_b[k]; a.ringx[k] = w.wv_ringx_b[k]; a.seed[k] = mix_seed(p->seed, 101 + k);
      a.dh_last[k] = ci == nc - 1 ? (dhidden ? dhidden + (size_t)k * B * H : nullptr) : w.carry[k] + (size_t)((ci + 1) % 2) * B * H;
      a.dh_init[k] = ci == 0 ? w.dh_init + (size_t)k * B * H : w.carry[k] + (size_t)(ci % 2) * B * H;
    }
    a.cnt = w.wv_cnt_b; a.err = reinterpret_cast<unsigned*>(sync_of(0));
    a.ks = ks_direct; a.flags = ks_direct ? 8 : 0;
    a.drop_p = drop ? p->rnn_drop : 0.f; a.drop_scale = drop ? 1.0f / (1.0f - p->rnn_drop) : 1.f; a.elem0 = (long long)t0 * B * H;
    c.call(gru_wave_bwd(a, ss));
  };
  for (int l = L - 1; l >= 0; --l) {
    // (wavefront: the weight gradients of a chunk run on the CUs the sweep of the chunk before leaves free -- always per chunk)
    const bool per_chunk = nc > 1 && (wave || ((p->wgrad_chunk_mask >> l) & 1));
    const int In = l == 0 ? In0 : H;
    int t_wg = -1, t_wg_hh = -1, t_wg_ih = -1;
    for (int ci = nc - 1; ci >= 0; --ci) {
      const int t0 = chunks[ci][0], t1 = chunks[ci][1], n = t1 - t0;
      if (wave) {
        // created with the top layer (the first iteration of the layer loop)
        if (l == L - 1) {
          t_wbc[ci] = P.add("wbsweep", 60.f + (n + 2 * L) * est_step_us(1) * hs, Q_MAIN, {ci == nc - 1 ? t_top : t_wbc[ci + 1]},
                            [&, ci, t0, n](hipStream_t ss) { wave_sweep(ss, ci, t0, n); });
          if (ci == nc - 1 && !ks_direct) for (int k = 0; k < L; ++k) { P.dep(t_wbc[ci], t_wt[k]); P.dep(t_wbc[ci], t_wit[k]); }
        }
        t_bs[l][ci] = t_wbc[ci];
      } else
      t_bs[l][ci] = P.add("bsweep", 40.f + n * est_step_us(1) * hs, q_sweep,
                          {l < L - 1 ? t_dx[l + 1][ci] : t_top, ci == nc - 1 ? t_wt[l] : t_bs[l][ci + 1]}, [&, l, ci, t0, n](hipStream_t ss) {
        void* ssp = reinterpret_cast<void*>(ss);
        if (p->rnn_drop > 0.f && l < L - 1)   // gradient through the inter-layer dropout mask
          c.call(b2t_dropout_f32(w.dY[l] + (long long)t0 * B * H, w.dY[l] + (long long)t0 * B * H, (long long)n * B * H, p->rnn_drop,
                                 mix_seed(p->seed, 101 + l), (long long)t0 * B * H, ssp));
        const float* dh_last = ci == nc - 1 ? (dhidden ? dhidden + (size_t)l * B * H : nullptr) : w.carry[l] + (size_t)((ci + 1) % 2) * B * H;
        float* dh_out = ci == 0 ? w.dh_init + (size_t)l * B * H : w.carry[l] + (size_t)(ci % 2) * B * H;
        if (c.rc) return;
        Ctx::Scope sc(c, ss, 9, 2.0 * n * B * 3.0 * H * H);
        c.call(b2t_gru_layer_bwd_f32(w.dY[l] + (long long)t0 * B * H, dh_last, w.res[l] + (long long)t0 * B * 4 * H,
                                     w.out[l] + (long long)(1 + t0) * B * H, w.out[l] + (long long)t0 * B * H, w.whh_t[l],
                                     w.dG[l] + (long long)t0 * B * 4 * H, dh_out, w.scratch[l], n, B, H,
                                     (mode & B2T_GRU_LOCAL) ? (mode | ((l & 1) ? B2T_GRU_PARITY : 0)) : mode,
                                     sync_of(l), ssp));
      });
      if (mode & B2T_GRU_LOCAL) P.t[t_bs[l][ci]].cls = l & 1;
      float e_dx = est_gemm((double)n * B, l > 0 ? H : In0, 3 * H);
      if (l == 0 && fast_day) e_dx += est_gemm(F, F, n, B) + 30.f;
      if (wave && l > 0) t_dx[l][ci] = t_bs[l][ci];   // made inside the sweep
      else
      t_dx[l][ci] = P.add("dx", e_dx, Q_ANY, {t_bs[l][ci], (l == 0 && fast_day && ci < nc - 1) ? t_dx[l][ci + 1] : -1, t_wpk[l]},
                          [&, l, t0, n](hipStream_t s) { dx_gemm(s, l, t0, n); });
      if (per_chunk || ci == 0) {
        const int w0 = per_chunk ? t0 : 0, w1 = per_chunk ? t1 : Tp;
        const int acc = per_chunk && ci != nc - 1 ? 1 : 0;
        const bool fin = ci == 0;
        const double K = (double)(w1 - w0) * B;
        // bf16 mode, whole-sequence weight gradients: their B operands (h_{t-1}^T, x^T) exist when the pass starts -- packed by a
        // task of their own that only this layer's weight gradients wait for (the transposing packs of layer 0 were 170 us of the
        // shipped shape's 1.3 ms tail behind the last sweep)
        int t_xp = -1;
        bool xpre = false;
        if (c.bf16_gemm && prepack_env && !per_chunk && w.xpk_hh[l] && (2 * H) % 128 == 0 && (3 * H) % 128 == 0) {
          b2t_gemm_desc a = gd(nullptr, nullptr, nullptr, 3 * H, H, (int)K), b = gd(nullptr, nullptr, nullptr, 3 * H, In, (int)K);
          b.a_brk = 2 * H;
          if (c.pack_shape_ok(a) && c.pack_shape_ok(b)) {
            xpre = true;
            t_xp = P.add("xpack", 20.f + (float)((double)K * (H + In) * 6.0 / 4.0e6), Q_ANY, {t_start},
                         [&, l, w0, w1](hipStream_t s) { layer_weight_grads(c, s, prm, grd, p, w, l, w0, w1, 0, false, 1); });
          }
        }
        // ... and dW_hh / dW_ih as two tasks (own slab and sums for dW_hh): behind the last sweep of the shipped shape the small
        // dW_hh[0] (0.25 ms at 155 TF/s) no longer stands in front of the 258-GFLOP dW_ih[0] on one queue
        if (xpre && split_env && w.slab_hh[l]) {
          const int t_hh = P.add("wgrad_hh", est_gemm(3 * H, H, K) + 30.f, Q_ANY, {t_bs[l][ci], t_wg_hh, t_xp},
                                 [&, l, w0, w1, acc, fin](hipStream_t s) { layer_weight_grads(c, s, prm, grd, p, w, l, w0, w1, acc, fin, 3, true, 1); });
          const int t_ih = P.add("wgrad_ih", est_gemm(3 * H, In, K) + 30.f, Q_ANY, {t_bs[l][ci], t_wg_ih, t_xp},
                                 [&, l, w0, w1, acc, fin](hipStream_t s) { layer_weight_grads(c, s, prm, grd, p, w, l, w0, w1, acc, fin, 3, true, 2); });
          t_wg_hh = t_hh; t_wg_ih = t_ih;
          t_wg = P.add("wgrad_join", 0.f, Q_ANY, {t_hh, t_ih}, nullptr);
        } else
        t_wg = P.add("wgrad", est_gemm(3 * H, H, K) + est_gemm(3 * H, In, K) + 60.f, Q_ANY, {t_bs[l][ci], t_wg, t_xp},
                     [&, l, w0, w1, acc, fin, xpre](hipStream_t s) { layer_weight_grads(c, s, prm, grd, p, w, l, w0, w1, acc, fin, 3, xpre); });
      }
    }
    t_wg_last[l] = t_wg;
    bucket(1 + l, t_wg);
  }

  // layer-0 input gradient -> day layer
  auto day_wgrad_desc = [&]() {      // per-sentence x[b]^T dpre[b] -> day_slab[b] (whole sequence)
    b2t_gemm_desc d = gd(x, w.dU, w.day_slab, F, F, T);
    d.Z = B; d.a_kcontig = 0; d.a_s0 = F; d.a_sz = (long long)T * F; d.b_kcontig = 0; d.b_s0 = F; d.b_sz = (long long)T * F;
    d.c_s0 = F; d.c_sz = (long long)F * F;
    return d;
  };
  // bf16 mode: its A operand is the INPUT (x[b]^T): packed when the pass starts instead of on the step's tail (217 us there, next to
  // layer 0's weight gradients)
  static const bool day_late_env = !(getenv("B2T_DAY_WGRAD_LATE") && atoi(getenv("B2T_DAY_WGRAD_LATE")) == 0);
  const bool day_whole = !fast_day || day_late_env;
  int t_xpk_day = -1;
  if (day_whole && w.xpk_day && prepack_env && c.pack_shape_ok_z(day_wgrad_desc()))
    t_xpk_day = P.add("xpack", 40.f, Q_ANY, {t_start}, [&](hipStream_t s) { b2t_gemm_desc d = day_wgrad_desc(); c.call(gemm_bf16p_pack(&d, 0, w.xpk_day, s)); });
  const void* day_a_pre = t_xpk_day >= 0 ? w.xpk_day : nullptr;
  const int t_dayfin = P.add("day_w", fast_day ? 60.f : est_gemm(F, F, T, B) + 200.f, Q_ANY, {t_dx[0][0], t_xpk_day}, [&, day_a_pre](hipStream_t s) {
    void* sp = reinterpret_cast<void*>(s);
    static const bool day_late = !(getenv("B2T_DAY_WGRAD_LATE") && atoi(getenv("B2T_DAY_WGRAD_LATE")) == 0);
    if (fast_day && day_late) {
      b2t_gemm_desc d = day_wgrad_desc();
      c.gemm(s, d, 1, nullptr, 0, -1, nullptr, nullptr, (day_a_pre && c.would_pack_z(d, s)) ? day_a_pre : nullptr);
      c.call(b2t_colsum_f32(w.dU, T, F, F, w.day_bslab, 0, w.cs_day, B, (long long)T * F, bias_ld, sp));
    }
    if (!fast_day) {
      if (prm->patch > 0) {   // fold + dropout backward + Softsign backward in one pass (three kernels on the step's tail before)
        c.call(b2t_patch_fold_day_bwd_f32(w.dV, w.U, w.dU, B, T, F, Tp, prm->patch, prm->stride, p->in_drop, mix_seed(p->seed, 17), sp));
      } else {
        if (p->in_drop > 0.f) c.call(b2t_dropout_f32(w.dU, w.dU, (long long)B * T * F, p->in_drop, mix_seed(p->seed, 17), 0, sp));
        c.call(b2t_softsign_bwd_f32(w.U, w.dU, (long long)B * T * F, sp));   // dpre = dU * (1-|U|)^2, in place
      }
      // per-sample partial day gradients, then deterministic reduction by day
      b2t_gemm_desc d = day_wgrad_desc();
      c.gemm(s, d, 1, nullptr, 0, -1, nullptr, nullptr, (day_a_pre && c.would_pack_z(d, s)) ? day_a_pre : nullptr);
      c.call(b2t_colsum_f32(w.dU, T, F, F, w.day_bslab, 0, w.cs_day, B, (long long)T * F, bias_ld, sp));
    }
    c.call(b2t_day_reduce_f32(w.day_slab, day_idx, B, (long long)F * F, grd->day_w, grd->day_w_stride, sp));
    c.call(b2t_day_reduce_f32(w.day_bslab, day_idx, B, bias_ld, grd->day_b, grd->day_b_stride, sp));
  });
  if (!fast_day || !(getenv("B2T_DAY_WGRAD_LATE") && atoi(getenv("B2T_DAY_WGRAD_LATE")) == 0)) for (int ci = 1; ci < nc; ++ci) P.dep(t_dayfin, t_dx[0][ci]);
  bucket(L + 2, t_dayfin);
  // h0 gradient: sum over layers and batch rows of the carry after t=0 (rnn_model.py:86,123)
  const int t_h0 = P.add("h0", 20.f, Q_ANY, {t_bs[0][0]}, [&](hipStream_t s) {
    void* sp = reinterpret_cast<void*>(s);
    if (!custom_states) c.call(b2t_colsum_f32(w.dh_init, (long long)L * B, H, H, grd->h0, 0, w.cs_h0, 1, 0, 0, sp));
    else c.call(check_hip(hipMemsetAsync(grd->h0, 0, sizeof(float) * H, s), "model_backward: h0 gradient"));
    if (dstates) c.call(check_hip(hipMemcpyAsync(dstates, w.dh_init, sizeof(float) * L * B * H, hipMemcpyDeviceToDevice, s), "model_backward: dstates"));
  });
  for (int l = 1; l < L; ++l) P.dep(t_h0, t_bs[l][0]);
  bucket(L + 1, t_h0);
  int t_end = -1;
  {
    t_end = P.add("end", 0.f, Q_MAIN, {t_h0, t_dayfin, t_head_w, t_bucket}, nullptr);
    for (int l = 0; l < L; ++l) { P.dep(t_end, t_wg_last[l]); P.dep(t_end, t_dx[l][0]); }
    P.dep(t_end, t_top);
  }
  run_plan(c, P, c.nq, c.qs);
  return c.rc;
}
