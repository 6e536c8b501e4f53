"""b2t_clm_score_tree_cached_f16 (csrc/causal_lm_cache.hip) on the MI355X: the tree forward behind a context cache against
the tree call b2t_clm_score_tree_f16 and the flat call b2t_clm_score_f16 on the same ids, byte for byte -- no tolerance: a
cached K / V row or log-prob IS the value this call would compute (a row's result depends on neither M nor the row's index
nor the tile rule, the tested premise of the tree path).

Every call gets a fresh workspace of exactly the size asked for, filled with 0xFF (NaN in fp16 and fp32); the cache's kv and
logp live inside larger allocations with canaries on both sides, are filled with 0xFF before first use and again beyond n
before each call, and logp[0] (unused) stays 0xFF.  Every check runs under both settings of B2T_CLM_TRUNK_ATTN (a cache per
setting, fed the same calls), and rows / reused / n are compared with the dictionary restatement of the rule in
tests/test_clm_cache_host.py.

Planted bugs this file was checked against are listed in NOTES.md "LLM"."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import SESSION, dict_rule, golden_session
from test_gpu_clm_contract import BOUND, V_OPT, WIDTHS, _err, _model, _ref_logp, _tiles
from test_gpu_clm_tree import _ListDecoder, _edge_model, _pack
from test_gpu_llm_rescore import _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

CAN = 4096
TRUNK_ENV = "B2T_CLM_TRUNK_ATTN"
SETTINGS = ("0", "1")


@contextlib.contextmanager
def _trunk(setting):
    old = os.environ.get(TRUNK_ENV)
    os.environ[TRUNK_ENV] = setting
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(TRUNK_ENV, None)
        else:
            os.environ[TRUNK_ENV] = old


def _split(tok, off):
    return [tok[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _plain(sc, seqs, mode=None, tree=False):
    """(scores, per-sequence token log-probs) of the flat or the tree call through the ABI, on a fresh 0xFF workspace of
    exactly the size asked for."""
    import torch
    import b2t_native as N
    lib = N.load()
    ids, off = _pack(seqs)
    M, S = len(ids), len(seqs)
    if tree:
        need = lib.b2t_clm_tree_ws_bytes(C.byref(sc.desc), R.tree_plan(ids, off)[2], M, S)
    else:
        need = lib.b2t_clm_ws_bytes(C.byref(sc.desc), M, S)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    scores = torch.empty(S, dtype=torch.float32, device="cuda")
    tok = torch.empty(M, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with _tiles(mode):
        if tree:
            rc = lib.b2t_clm_score_tree_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                            tok.data_ptr(), None, ws.data_ptr(), need, stream)
        else:
            rc = lib.b2t_clm_score_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(), tok.data_ptr(),
                                       ws.data_ptr(), need, stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    return scores.cpu().numpy(), _split(tok.cpu().numpy(), off)


class Rig:
    """A caller-owned cache of `cap` positions for the scorer's model, driven through the ABI."""

    def __init__(self, sc, cap, setting):
        import torch
        import b2t_native as N
        self.sc, self.cap, self.setting, self.lib = sc, cap, setting, N.load()
        dm = sc.dims
        self.nl, self.d = dm["n_layers"], dm["d_model"]
        nbytes = self.lib.b2t_clm_cache_kv_bytes(C.byref(sc.desc), cap)
        assert nbytes == self.nl * cap * 2 * self.d * 2
        g = torch.Generator(device="cuda").manual_seed(cap)
        self.kv_buf = torch.randint(0, 256, (nbytes + 2 * CAN,), dtype=torch.uint8, device="cuda", generator=g)
        self.lp_buf = torch.randint(0, 256, (4 * cap + 2 * CAN,), dtype=torch.uint8, device="cuda", generator=g)
        self.kv_can = (self.kv_buf[:CAN].clone(), self.kv_buf[-CAN:].clone())
        self.lp_can = (self.lp_buf[:CAN].clone(), self.lp_buf[-CAN:].clone())
        self.kv = self.kv_buf[CAN:CAN + nbytes].view(torch.float16).view(self.nl, cap, 2 * self.d)
        self.logp = self.lp_buf[CAN:CAN + 4 * cap].view(torch.float32)
        self.kv_buf[CAN:CAN + nbytes] = 0xFF
        self.lp_buf[CAN:CAN + 4 * cap] = 0xFF
        self.ids = np.full(cap + 2, -77, np.int32)            # [0] and [-1] are host canaries
        self.c = N.ClmCache(self.kv.data_ptr(), self.logp.data_ptr(), self.ids[1:].ctypes.data, cap, 0)

    @property
    def n(self):
        return int(self.c.n)

    def chain(self):
        return [int(x) for x in self.ids[1:1 + self.n]]

    def device_bytes(self):
        return self.kv_buf.clone(), self.lp_buf.clone()

    def call(self, seqs, mode=None, update=1, with_tok=True):
        """One cached call: (scores, token log-probs, plan).  Checks rows, reused and n against the dictionary rule, the
        canaries, and that a read-only call leaves the cache's host and device state as it was."""
        import torch
        import b2t_native as N
        ids, off = _pack(seqs)
        M, S = len(ids), len(seqs)
        want = dict_rule(self.chain(), self.cap, seqs)
        assert R.cache_plan(np.asarray(self.chain(), np.int32), self.cap, ids, off) == want
        # poison what the cache does not hold
        n = self.n
        self.kv.view(torch.int16)[:, n:, :] = -1      # 0xFF bytes
        self.logp.view(torch.int32)[n:] = -1
        self.logp.view(torch.int32)[0] = -1
        before = self.device_bytes() if not update else None
        n0, ids0 = self.n, self.ids.copy()
        need = self.lib.b2t_clm_tree_cached_ws_bytes(C.byref(self.sc.desc), want["rows"], M, S)
        assert 0 < need <= self.lib.b2t_clm_tree_cached_ws_bytes(C.byref(self.sc.desc), want["nodes"], M, S)
        ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
        ws[:need] = 0xFF
        ws[need:] = 0x5A
        scores = torch.full((S + 16,), 12345.0, device="cuda")
        tok = torch.full((M + 16,), 12345.0, device="cuda")
        rows, reused = C.c_longlong(-1), C.c_int(-1)
        with _tiles(mode), _trunk(self.setting):
            rc = self.lib.b2t_clm_score_tree_cached_f16(C.byref(self.sc.desc), C.byref(self.c), update, ids.ctypes.data,
                                                        off.ctypes.data, S, scores.data_ptr(),
                                                        tok.data_ptr() if with_tok else None, C.byref(rows), C.byref(reused),
                                                        ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.last_error()
        torch.cuda.synchronize()
        assert (rows.value, reused.value) == (want["rows"], want["reused"]), (rows.value, reused.value, want)
        assert (ws[need:] == 0x5A).all() and (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
        assert torch.equal(self.kv_buf[:CAN], self.kv_can[0]) and torch.equal(self.kv_buf[-CAN:], self.kv_can[1])
        assert torch.equal(self.lp_buf[:CAN], self.lp_can[0]) and torch.equal(self.lp_buf[-CAN:], self.lp_can[1])
        assert self.ids[0] == -77 and self.ids[-1] == -77
        if update:
            assert self.n == want["n_after"] and self.chain() == [int(x) for x in seqs[0][:self.n]]
            # what the cache now holds is finite; logp[0] was not touched
            assert torch.isfinite(self.kv[:, :self.n, :].float()).all() and torch.isfinite(self.logp[1:self.n]).all()
            assert torch.isnan(self.logp[0])
        else:
            after = self.device_bytes()
            assert self.n == n0 and (self.ids == ids0).all()
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
        return scores[:S].cpu().numpy(), (_split(tok[:M].cpu().numpy(), off) if with_tok else None), want


def _same_bytes(a, b, what):
    sa, ta = a[0], a[1]
    sb, tb = b[0], b[1]
    bad = [i for i, (x, y) in enumerate(zip(ta, tb)) if x.tobytes() != y.tobytes()]
    if bad:
        i = bad[0]
        j = int(np.flatnonzero(ta[i].view(np.uint32) != tb[i].view(np.uint32))[0])
        raise AssertionError(f"{what}: {len(bad)} of {len(ta)} sequences differ; first: sequence {i} token {j}: "
                             f"{ta[i][j]!r} against {tb[i][j]!r}")
    assert len(ta) == len(tb) and sa.dtype == sb.dtype and sa.tobytes() == sb.tobytes(), what


def _check(rigs, sc, seqs, mode=None, update=1, what="", flat=True):
    """The cached call of every rig == the tree call == the flat call; returns the plans (one per rig)."""
    tree = _plain(sc, seqs, mode, tree=True)
    assert all(np.isfinite(x).all() for x in tree[1]) and np.isfinite(tree[0]).all(), what
    if flat:
        _same_bytes(_plain(sc, seqs, mode), tree, f"{what}: flat against tree")
    plans = []
    for rig in rigs:
        s, t, plan = rig.call(seqs, mode, update)
        _same_bytes((s, t), tree, f"{what}: cached (trunk attention {rig.setting}) against tree")
        plans.append(plan)
    return plans


def _rigs(sc, cap):
    return [Rig(sc, cap, s) for s in SETTINGS]


def test_session_on_the_recorded_lists():
    """The recorded n-best lists as a conversation of 8 calls (cases 0, 1, 2, 3, 0, 1, 2, 0; context = the first candidates so
    far): trunk, reused and rows are the numbers counted on the CPU, and from the second call on the whole previous trunk is
    found again."""
    sc, _, _ = _tiny()
    calls = golden_session()
    assert max(len(s) for seqs in calls for s in seqs) == 33 <= sc.dims["max_pos"]
    rigs = _rigs(sc, sc.dims["max_pos"])
    prev = None
    for k, seqs in enumerate(calls):
        for plan in _check(rigs, sc, seqs, what=f"recorded session call {k}"):
            assert [plan[x] for x in ("trunk", "reused", "rows", "nodes")] == [SESSION[x][k] for x in ("trunk", "reused", "rows", "nodes")]
            if prev is not None:
                assert plan["common"] == prev and plan["reused"] == prev - 1
        prev = SESSION["trunk"][k]


@pytest.mark.parametrize("shape", ["d320", "1.3b", "2.7b", "6.7b"])
def test_session_of_nbest_lists_across_tile_rules(shape):
    """Six calls of 100-candidate lists, context k+1 = context k + the first candidate of call k, B2T_CLM_GEMM_256 changing
    from call to call (0 / unset / 2): the cached rows come from another tile rule, and from GEMMs of another M, than the
    rows they are mixed with."""
    import bench_llm_rescore as B
    d, H, F, V = (320, 4, 1216, 1000) if shape == "d320" else WIDTHS[shape] + (V_OPT,)
    sc, _, _ = _model(d, H, F, V)
    rng = np.random.default_rng(d)
    rigs = _rigs(sc, 256)
    ctx, prev = [], None
    for k, mode in enumerate(("0", None, "2", None, "0", "2")):
        seqs = B.nbest_list(rng, V, 100, ctx)
        plans = _check(rigs, sc, seqs, mode, what=f"nbest session {shape} call {k}")
        for plan in plans:
            assert plan["trunk"] >= len(ctx) + 1
            if prev is not None:
                assert plan["common"] == prev and plan["reused"] == prev - 1 and plan["rows"] == plan["nodes"] - prev + 1
        print(f"CLM cache session {shape} call {k}: context {len(ctx)}, {sum(map(len, seqs))} tokens, {plans[0]['nodes']} nodes, "
              f"{plans[0]['rows']} rows computed, {plans[0]['reused']} reused")
        prev = plans[0]["n_after"]
        ctx = [int(x) for x in seqs[0][1:]]
    assert prev > 64


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_reuse_at_block_edges_and_max_pos(hd):
    """R = 31, 32, 33, 63, 64, 65 (the key block that straddles R takes keys from both sources; Rb = 0 at 31; Rb = R at 32 and
    64: the suffix kernel's first block has no cached key), with the first owned position of the later sequences right behind
    R and 44 positions later; then a path of exactly max_pos with R = max_pos - 2."""
    sc, _, _ = _edge_model(hd)
    rng = np.random.default_rng(hd)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    chain = [2] + r(149)
    for Rr in (31, 32, 33, 63, 64, 65):
        rigs = _rigs(sc, 150)
        for plan in _check(rigs, sc, [chain[:Rr + 1]], what=f"hd {hd} prime {Rr}", flat=False):
            assert plan["n_after"] == Rr + 1
        near = [chain[:Rr + 1] + r(n) for n in (20, 45, 1, 7)]
        far = [chain[:Rr + 45] + r(n) for n in (20, 33, 1)] + [chain[:Rr + 45]]
        for name, seqs in (("near", near), ("far", far)):
            for plan in _check(rigs, sc, seqs, update=0, what=f"hd {hd} R {Rr} {name}"):
                assert plan["reused"] == Rr and plan["rows"] % 32 != 0
        # and updating: the cache grows to the far trunk, a second call finds all of it
        _check(rigs, sc, far, what=f"hd {hd} R {Rr} far, updating", flat=False)
        for plan in _check(rigs, sc, far, what=f"hd {hd} R {Rr} far again", flat=False):
            assert plan["reused"] == Rr + 44
    rigs = _rigs(sc, 150)
    _check(rigs, sc, [chain[:149]], what="prime 149", flat=False)
    seqs = [chain, chain[:149] + r(1), chain[:149]]
    assert max(map(len, seqs)) == 150 == sc.dims["max_pos"]
    for plan in _check(rigs, sc, seqs, what=f"max_pos hd {hd}"):
        assert plan["reused"] == 148 and plan["rows"] == 3


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_small_caps_and_changing_contexts(hd):
    sc, _, _ = _edge_model(hd)
    rng = np.random.default_rng(100 + hd)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    ctx = [2] + r(69)
    lst = lambda c: [c + t for t in (r(9), r(12), r(3))]
    # cap = trunk - 1 and cap = 1
    for cap in (69, 1):
        rigs = _rigs(sc, cap)
        for plan in _check(rigs, sc, lst(ctx), what=f"cap {cap}"):
            assert plan["trunk"] == 70 and plan["n_after"] == cap
        for plan in _check(rigs, sc, lst(ctx), what=f"cap {cap} again", flat=False):
            assert plan["common"] == cap and plan["reused"] == cap - 1
    # the context replaced by one of equal length that differs from position 35 on, cut to half, emptied, restored
    rigs = _rigs(sc, 150)
    other = ctx[:35] + r(35)
    steps = [("first", ctx, 0), ("replaced", other, 35), ("half", other[:35], 35), ("emptied", [2], 1), ("restored", ctx, 1),
             ("diverging early", ctx[:10] + r(60), 10), ("restored again", ctx, 10)]
    for name, c, common in steps:
        for plan in _check(rigs, sc, lst(c), what=f"context {name}", flat=name in ("first", "replaced")):
            assert plan["common"] == common and plan["n_after"] == len(c), (name, plan)


def test_forest_duplicates_and_a_lone_sequence():
    sc, _, _ = _edge_model(64)
    rng = np.random.default_rng(5)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    a = [2] + r(40)
    rigs = _rigs(sc, 150)
    # read-only on an empty cache: nothing to read, nothing written (every row of the cache is still 0xFF)
    for plan in _check(rigs, sc, [a, a[:10] + r(5)], update=0, what="read-only, empty cache"):
        assert (plan["trunk"], plan["reused"]) == (10, 0)
    # a lone sequence scored twice: the second call computes one row and no head row
    for plan in _check(rigs, sc, [a], what="lone"):
        assert (plan["reused"], plan["rows"], plan["n_after"]) == (0, 41, 41)
    for plan in _check(rigs, sc, [a], what="lone again"):
        assert (plan["reused"], plan["rows"]) == (40, 1)
    # duplicates: all equal -> the trunk is the whole sequence; then duplicates among different ones
    for plan in _check(rigs, sc, [a, a, a], what="all equal"):
        assert (plan["trunk"], plan["rows"]) == (41, 1)
    b = a[:20] + r(10)
    for plan in _check(rigs, sc, [a, b, a, a + r(2), b], what="duplicates"):
        assert (plan["trunk"], plan["reused"], plan["n_after"]) == (20, 19, 20)
    # a forest has no trunk: nothing reused, the cache empties; the next list starts it again
    for plan in _check(rigs, sc, [a, [3] + r(9), a[:7] + r(3), [3]], what="forest"):
        assert (plan["trunk"], plan["reused"], plan["n_after"]) == (0, 0, 0)
    assert all(rig.n == 0 for rig in rigs)
    for plan in _check(rigs, sc, [a + r(3), a + r(4)], what="after the forest"):
        assert (plan["reused"], plan["n_after"]) == (0, 41)
    # one-token sequences
    for plan in _check(rigs, sc, [[2], [2]], what="one token"):
        assert (plan["trunk"], plan["common"], plan["reused"], plan["rows"]) == (1, 1, 0, 1)
    # scores without tok_logp_out equal those with it
    seqs = [a + r(3), a + r(4)]
    for rig in rigs:
        s1, _, _ = rig.call(seqs, update=0)
        s2, t2, _ = rig.call(seqs, update=0, with_tok=False)
        assert t2 is None and s1.tobytes() == s2.tobytes()


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_cached_path_within_fp64_bound(hd):
    """The cached path inherits the contract through the byte comparisons; this guards against all three paths being wrong
    together: a shared-context list whose context comes from the cache, at test_gpu_clm_contract's bound and reference."""
    import bench_llm_rescore as B
    sc, st, dims = _edge_model(hd)
    rng = np.random.default_rng(hd)
    ctx = [int(x) for x in rng.integers(4, 1000, 70)]
    for rig in _rigs(sc, 150):
        rig.call([[2] + ctx], update=1)
        seqs = B.nbest_list(rng, 1000, 30, ctx)
        assert max(map(len, seqs)) <= dims["max_pos"]
        _, got, plan = rig.call(seqs)
        assert plan["reused"] == 70
        err, mx = _err(got, _ref_logp(st, dims, seqs))
        print(f"CLM cache fp64 hd {hd} trunk attention {rig.setting}: {plan['nodes']} nodes, {plan['rows']} rows, "
              f"max |dlogp| {err:.3e} (max |logp| {mx:.2f})")
        assert err <= BOUND, (hd, err)


def test_a_corrupted_cache_entry_is_visible_where_it_is_used():
    """Cache 60 positions, then score a list whose context follows the chain for 40: R = 39.  One K element, one V element or
    one log-prob changed at a reused position changes the scores; the same at a position >= R, which the call overwrites (or,
    read-only, never reads), does not."""
    import torch
    sc, _, _ = _edge_model(64)
    rng = np.random.default_rng(9)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    chain = [2] + r(59)
    ctx = chain[:40] + r(30)
    seqs = [ctx + t for t in (r(8), r(5), r(11))]
    ref = _plain(sc, seqs, tree=True)
    d = sc.dims["d_model"]
    for setting in SETTINGS:
        for update in (1, 0):
            for what, pos, changes in (("K", 5, True), ("V", 37, True), ("logp", 12, True), ("logp", 39, True),
                                       ("K", 39, False), ("V", 45, False), ("logp", 40, False), ("K", 59, False)):
                rig = Rig(sc, 150, setting)
                rig.call([chain])
                assert rig.n == 60
                if what == "K":
                    rig.kv[1, pos, 3] += 0.5
                elif what == "V":
                    rig.kv[0, pos, d + 70] += 0.5
                else:
                    rig.logp[pos] += 0.25
                torch.cuda.synchronize()
                s, t, plan = rig.call(seqs, update=update)
                assert plan["reused"] == 39
                same = s.tobytes() == ref[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(t, ref[1]))
                assert same != changes, (setting, update, what, pos)


def test_scorer_surface():
    """OptScorer(context_cache_tokens=...): cached by default, use_cache=False gives the uncached call and its two-key
    last_stats, update_cache=False reads only, cache_reset forgets."""
    import torch
    _, z, gold = _tiny()
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    dims = R.opt_dims(gold["config"])
    lay = R.device_layout(state, dims)
    plain = R.OptScorer(dims, lay, "cuda")
    assert plain.context_cache_tokens == 0 and plain.cache_len == 0
    with pytest.raises(ValueError, match="use_cache"):
        plain.score([[2, 5]], use_cache=True)
    with pytest.raises(ValueError, match="max_pos"):
        R.OptScorer(dims, lay, "cuda", context_cache_tokens=dims["max_pos"] + 1)
    sc = R.OptScorer(dims, lay, "cuda", context_cache_tokens=64)
    assert sc.cache_len == 0 and sc.share_prefixes is False
    ctx = [2, 9, 8, 7, 6, 5]
    seqs = [ctx + [11, 12], ctx + [11, 13], ctx + [14]]
    want = plain.score(seqs, 0.5)
    assert plain.last_stats == {"tokens": 23, "nodes": 23}
    a = sc.score(seqs, 0.5)
    assert sc.last_stats == {"tokens": 23, "nodes": 10, "reused": 0} and sc.cache_len == 6 and sc.cache_ids.tolist() == ctx
    b = sc.score(seqs, 0.5)
    assert sc.last_stats == {"tokens": 23, "nodes": 5, "reused": 5}
    c = sc.score(seqs, 0.5, use_cache=False)
    assert sc.last_stats == {"tokens": 23, "nodes": 23} and sc.cache_len == 6
    d = sc.score(seqs, 0.5, share_prefixes=True, use_cache=False)
    assert sc.last_stats == {"tokens": 23, "nodes": 10}
    longer = [s + [15] for s in seqs[:2]]
    e = sc.score(longer, 0.5, update_cache=False)
    assert sc.last_stats == {"tokens": 18, "nodes": 6, "reused": 5} and sc.cache_len == 6
    assert e.tobytes() == plain.score(longer, 0.5).tobytes()
    assert want.tobytes() == a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    t = sc.token_logprobs(seqs)
    assert sc.last_stats["reused"] == 5
    assert all(x.tobytes() == y.tobytes() for x, y in zip(t, plain.token_logprobs(seqs)))
    sc.cache_reset()
    assert sc.cache_len == 0
    assert sc.score(seqs, 0.5).tobytes() == want.tobytes() and sc.last_stats["reused"] == 0
    assert len(sc.score([])) == 0 and sc.last_stats == {"tokens": 0, "nodes": 0}
    with pytest.raises(RuntimeError, match="outside"):
        sc.score([[2, 5, 99999]])
    with pytest.raises(RuntimeError, match="max_pos"):
        sc.score([[2] * (dims["max_pos"] + 1)])
    assert sc.score(seqs, 0.5).tobytes() == want.tobytes()


def test_service_replies_are_the_same_with_a_context_cache():
    """LocalLMService with do_opt = 1 over three sentences with a growing context (each reply's sentence joins it, as the
    closed loop does): a scorer with a context cache gives, field by field, the replies of one without, and reuses more at
    every sentence.  remote_lm_reset between the sentences leaves the cache alone."""
    import evaluate_model_helpers as H
    import torch
    from remote_lm import LocalLMService
    _, z, gold = _tiny()
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    dims = R.opt_dims(gold["config"])
    tok = R.WordTokenizer(**gold["tokenizer"])
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies, reused = {}, {}
    for cache_tokens in (0, 128):
        sc = R.OptScorer(dims, R.device_layout(state, dims), "cuda", context_cache_tokens=cache_tokens)
        ctx, replies[cache_tokens], reused[cache_tokens] = "well then", [], []
        for nbest in lists:
            r = LocalLMService(_ListDecoder(nbest), acoustic_scale=0.3, alpha=0.5, nbest=100, decode_fn=lambda *a: None,
                               llm=(sc, tok), do_opt=1, top_candidates_to_augment=20)
            r.set("contextual_decoding_current_context", ctx)
            t0 = H.get_current_redis_time_ms(r)
            H.reset_remote_language_model(r, t0)
            r.xadd("remote_lm_finalize", {"done": 0})
            reply = r.streams["remote_lm_output_final"][-1][1]
            replies[cache_tokens].append(reply)
            reused[cache_tokens].append(sc.last_stats.get("reused"))
            ctx = ctx + " " + reply[b"lm_response_final"].decode()
    for a, b in zip(replies[0], replies[128]):
        assert set(a) == set(b) and b"scoring" in a and a[b"lm_response_final"]
        for k in a:
            assert a[k] == b[k], k
    print(f"CLM cache service: reused per sentence {reused[128]}")
    assert reused[0] == [None, None, None]
    assert reused[128][0] == 0 and reused[128][0] < reused[128][1] < reused[128][2], reused
