"""b2t_clm_llama_score_tree_cached_f16 (csrc/causal_lm_llama.hip over the kernels of csrc/causal_lm_cache.hip) on the MI355X:
the Llama family's tree forward behind a context cache against the tree call b2t_clm_llama_score_tree_f16, the flat call
b2t_clm_llama_score_f16 and an independent read-only cached call on the same ids, byte for byte -- no tolerance: a cached
K / V row (K after the rotation, at its absolute position) or log-prob IS the value this call would compute.

As in tests/test_gpu_clm_cache.py every call gets a fresh workspace of exactly the size asked for, filled with 0xFF (NaN in
fp16 and fp32) with a canary behind it; the cache's kv ([n_layers][cap][2 * n_kv_heads * head_dim]) and logp live inside
larger allocations with canaries on both sides, are filled with 0xFF before first use and again beyond n before each call,
and logp[0] (unused) stays 0xFF.  Every check runs under both settings of B2T_CLM_TRUNK_ATTN (a cache per setting, fed the
same calls), and rows / reused / n are compared with the dictionary restatement of the rule in tests/test_clm_cache_host.py.

The tiny models are tests/test_clm_llama_host.py's: group sizes 2 (llama), 4 (qwen2), 1 (mistral) and 8 (llama3), head dims 64
and 128 (the latter with permuted q / k rows), q / k / v biases, llama3 frequency scaling.

Planted bugs this file was checked against are listed in NOTES.md "LLM"."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import dict_rule
from test_clm_llama_host import TINY, state_of, tiny_model
from test_gpu_clm_cache import CAN, SETTINGS, _same_bytes, _split, _trunk
from test_gpu_clm_llama import _call, _contract, _pack, _prod_list, _tiles, _tiny, _wide
from test_gpu_clm_tree import _ListDecoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


class Rig:
    """A caller-owned cache of `cap` positions for the scorer's model, driven through the ABI; slab rows are
    k[n_kv_heads * head_dim] | v[n_kv_heads * head_dim]."""

    def __init__(self, sc, cap, setting):
        import torch
        import b2t_native as N
        self.sc, self.cap, self.setting, self.lib = sc, cap, setting, N.load()
        dm = sc.dims
        self.nl, self.kvw = dm["n_layers"], dm["n_kv_heads"] * (dm["d_model"] // dm["n_heads"])
        nbytes = self.lib.b2t_clm_llama_cache_kv_bytes(C.byref(sc.desc), cap)
        assert nbytes == self.nl * cap * 2 * self.kvw * 2
        g = torch.Generator(device="cuda").manual_seed(cap)
        self.kv_buf = torch.randint(0, 256, (nbytes + 2 * CAN,), dtype=torch.uint8, device="cuda", generator=g)
        self.lp_buf = torch.randint(0, 256, (4 * cap + 2 * CAN,), dtype=torch.uint8, device="cuda", generator=g)
        self.kv_can = (self.kv_buf[:CAN].clone(), self.kv_buf[-CAN:].clone())
        self.lp_can = (self.lp_buf[:CAN].clone(), self.lp_buf[-CAN:].clone())
        self.kv = self.kv_buf[CAN:CAN + nbytes].view(torch.float16).view(self.nl, cap, 2 * self.kvw)
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
        need = self.lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(self.sc.desc), want["rows"], M, S)
        assert 0 < need <= self.lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(self.sc.desc), want["nodes"], M, S)
        ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
        ws[:need] = 0xFF
        ws[need:] = 0x5A
        scores = torch.full((S + 16,), 12345.0, device="cuda")
        tok = torch.full((M + 16,), 12345.0, device="cuda")
        rows, reused = C.c_longlong(-1), C.c_int(-1)
        with _tiles(mode), _trunk(self.setting):
            rc = self.lib.b2t_clm_llama_score_tree_cached_f16(C.byref(self.sc.desc), C.byref(self.c), update, ids.ctypes.data,
                                                              off.ctypes.data, S, scores.data_ptr(),
                                                              tok.data_ptr() if with_tok else None, C.byref(rows),
                                                              C.byref(reused), ws.data_ptr(), need,
                                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0, N.last_error()
        torch.cuda.synchronize()
        assert (rows.value, reused.value) == (want["rows"], want["reused"]), (rows.value, reused.value, want)
        assert (ws[need:] == 0x5A).all() and (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
        assert torch.equal(self.kv_buf[:CAN], self.kv_can[0]) and torch.equal(self.kv_buf[-CAN:], self.kv_can[1])
        assert torch.equal(self.lp_buf[:CAN], self.lp_can[0]) and torch.equal(self.lp_buf[-CAN:], self.lp_can[1])
        assert self.ids[0] == -77 and self.ids[-1] == -77
        if update:
            assert self.n == want["n_after"] and self.chain() == [int(x) for x in seqs[0][:self.n]]
            # what the cache now holds is finite; logp[0] and what lies beyond both the old and the new n were not touched
            assert torch.isfinite(self.kv[:, :self.n, :].float()).all() and torch.isfinite(self.logp[1:self.n]).all()
            assert torch.isnan(self.logp[0])
            hi = max(n0, self.n, 1)
            assert (self.kv.view(torch.int16)[:, hi:, :] == -1).all() and (self.logp.view(torch.int32)[hi:] == -1).all()
        else:
            after = self.device_bytes()
            assert self.n == n0 and (self.ids == ids0).all()
            assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
        return scores[:S].cpu().numpy(), (_split(tok[:M].cpu().numpy(), off) if with_tok else None), want


class FamilyLib:
    """The library as Rig drives it, for a scorer of another family on the Llama descriptor: Rig's two cached calls,
    b2t_clm_llama_tree_cached_ws_bytes and b2t_clm_llama_score_tree_cached_f16, go to the family's -- the size by sc._SIZES with
    sc._size_args, the score to b2t_clm_<family>_score_tree_cached_f16 with sc._qk -- each extra argument right behind the
    model; every other name is the library's own.  family: what sc._family must be."""

    def __init__(self, lib, sc, family):
        assert sc._family == family
        self._lib, self._sc = lib, sc

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def b2t_clm_llama_tree_cached_ws_bytes(self, desc, *args):
        return getattr(self._lib, self._sc._SIZES + "tree_cached_ws_bytes")(desc, *self._sc._size_args, *args)

    def b2t_clm_llama_score_tree_cached_f16(self, desc, *args):
        return getattr(self._lib, f"b2t_clm_{self._sc._family}_score_tree_cached_f16")(desc, *self._sc._qk, *args)


def _check(rigs, sc, seqs, mode=None, update=1, what="", flat=True):
    """Per rig: an independent read-only cached call, then (update on) the updating one, each == the tree call == the flat
    call; returns the plans (one per rig)."""
    tree = _call(sc, seqs, True, mode)
    if flat:
        _same_bytes(_call(sc, seqs, False, mode), tree, f"{what}: flat against tree")
    plans = []
    for rig in rigs:
        s, t, plan = rig.call(seqs, mode, 0)
        _same_bytes((s, t), tree, f"{what}: read-only cached (trunk attention {rig.setting}) against tree")
        if update:
            s, t, again = rig.call(seqs, mode, 1)
            assert again == plan
            _same_bytes((s, t), tree, f"{what}: cached (trunk attention {rig.setting}) against tree")
        plans.append(plan)
    return plans


def _rigs(sc, cap):
    return [Rig(sc, cap, s) for s in SETTINGS]


def _sc(name):
    return _tiny(name)[0]


def _rand(rng, V):
    return lambda n: [int(x) for x in rng.integers(4, V, n)]


@pytest.mark.parametrize("name", list(TINY))
def test_session_of_nbest_lists_across_tile_rules(name):
    """Six calls of 30-candidate lists, context k+1 = the first candidate of call k, B2T_CLM_GEMM_256 changing from call to
    call (0 / unset / 2): the cached rows come from another tile rule, and from GEMMs of another M, than the rows they are
    mixed with; from the second call on the whole previous trunk is found again."""
    import bench_llm_rescore as B
    sc = _sc(name)
    V, max_pos = sc.dims["vocab"], sc.dims["max_pos"]
    rng = np.random.default_rng(sc.dims["d_model"] + V)
    rigs = _rigs(sc, max_pos)
    ctx, prev = [], None
    for k, mode in enumerate(("0", None, "2", "0", None, "2")):
        seqs = B.nbest_list(rng, V, 30, ctx)
        assert max(map(len, seqs)) <= max_pos
        plans = _check(rigs, sc, seqs, mode, what=f"nbest session {name} call {k}")
        for plan in plans:
            assert plan["trunk"] >= len(ctx) + 1
            if prev is not None:
                assert plan["common"] == prev and plan["reused"] == prev - 1 and plan["rows"] == plan["nodes"] - prev + 1
        print(f"CLM llama cache session {name} call {k}: context {len(ctx)}, {sum(map(len, seqs))} tokens, "
              f"{plans[0]['nodes']} nodes, {plans[0]['rows']} rows computed, {plans[0]['reused']} reused")
        prev = plans[0]["n_after"]
        ctx = [int(x) for x in seqs[0][1:]]
    assert prev > 64


@pytest.mark.parametrize("name", list(TINY))
def test_reuse_at_block_edges_and_max_pos(name):
    """R = 31, 32, 33, 63, 64, 65 (the key block that straddles R takes keys from both sources; Rb = 0 at 31; Rb = R at 32 and
    64: the suffix kernel's first block has no cached key), with the first owned position of the later sequences right behind
    R and 44 positions later; then (llama: 256, mistral: 192, its sliding window) a path of exactly max_pos with
    R = max_pos - 2."""
    sc = _sc(name)
    rng = np.random.default_rng(len(name))
    r = _rand(rng, sc.dims["vocab"])
    chain = [2] + r(149)
    for Rr in (31, 32, 33, 63, 64, 65):
        rigs = _rigs(sc, 150)
        for plan in _check(rigs, sc, [chain[:Rr + 1]], what=f"{name} prime {Rr}", flat=False):
            assert plan["n_after"] == Rr + 1
        near = [chain[:Rr + 1] + r(n) for n in (20, 45, 1, 7)]
        far = [chain[:Rr + 45] + r(n) for n in (20, 33, 1)] + [chain[:Rr + 45]]
        for what, seqs in (("near", near), ("far", far)):
            for plan in _check(rigs, sc, seqs, update=0, what=f"{name} R {Rr} {what}"):
                assert plan["reused"] == Rr and plan["rows"] % 32 != 0
        # and updating: the cache grows to the far trunk, a second call finds all of it
        _check(rigs, sc, far, what=f"{name} R {Rr} far, updating", flat=False)
        for plan in _check(rigs, sc, far, what=f"{name} R {Rr} far again", flat=False):
            assert plan["reused"] == Rr + 44
    if name not in ("llama", "mistral"):
        return
    P = sc.dims["max_pos"]
    assert P == {"llama": 256, "mistral": 192}[name]
    chain = [2] + r(P - 1)
    rigs = _rigs(sc, P)
    _check(rigs, sc, [chain[:P - 1]], what=f"{name} prime {P - 1}", flat=False)
    seqs = [chain, chain[:P - 1] + r(1), chain[:P - 1]]
    assert max(map(len, seqs)) == P
    for plan in _check(rigs, sc, seqs, what=f"{name} max_pos"):
        assert plan["reused"] == P - 2 and plan["rows"] == 3 and plan["n_after"] == P - 1


@pytest.mark.parametrize("name", ["llama", "qwen2"])
def test_small_caps_and_changing_contexts(name):
    sc = _sc(name)
    rng = np.random.default_rng(100 + len(name))
    r = _rand(rng, sc.dims["vocab"])
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
    for what, c, common in steps:
        for plan in _check(rigs, sc, lst(c), what=f"context {what}", flat=what in ("first", "replaced")):
            assert plan["common"] == common and plan["n_after"] == len(c), (what, plan)


def test_forest_duplicates_and_a_lone_sequence():
    sc = _sc("qwen2")   # one K / V head for four query heads
    assert sc.dims["n_kv_heads"] == 1
    rng = np.random.default_rng(5)
    r = _rand(rng, sc.dims["vocab"])
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


@pytest.mark.parametrize("width", ["llama3.2-1b", "qwen2.5-7b"])
def test_full_width_layer_behind_a_cached_context(width):
    """One full-width layer plus the head (group sizes 4 and 7, biases on the latter): a 100-token context primed into the
    cache, then 100 candidates behind it under each tile rule -- the cached rows come from a GEMM of 101 rows."""
    sc, _, rd, _ = _wide(width)
    assert rd["n_heads"] // rd["n_kv_heads"] == {"llama3.2-1b": 4, "qwen2.5-7b": 7}[width]
    seqs = _prod_list(rd["vocab"], seed=1, cands=100, context=100)
    ctx = seqs[0][:101]
    assert all(s[:101] == ctx for s in seqs)
    rigs = _rigs(sc, 256)
    for rig in rigs:
        rig.call([ctx])
        assert rig.n == 101
    base = _call(sc, seqs, True)
    _same_bytes(_call(sc, seqs, False), base, f"{width}: flat against tree")
    for mode in ("0", None, "2"):
        if mode is not None:
            _same_bytes(_call(sc, seqs, True, mode), base, f"{width}: tree under tile rule {mode}")
        for rig in rigs:
            s, t, plan = rig.call(seqs, mode, update=0)
            assert plan["reused"] == 100
            _same_bytes((s, t), base, f"{width}: cached under tile rule {mode}, trunk attention {rig.setting}")


@pytest.mark.parametrize("name", list(TINY))
def test_cached_path_within_the_contract(name):
    """The cached path inherits the contract through the byte comparisons; this guards against all three paths being wrong
    together: a shared-context list whose context comes from the cache, at tests/test_gpu_clm_llama.py's bound and
    reference."""
    import bench_llm_rescore as B
    sc, _, st, rd, inv = _tiny(name)
    V = rd["vocab"]
    rng = np.random.default_rng(V)
    ctx = [int(x) for x in rng.integers(4, V, 70)]
    seqs = B.nbest_list(rng, V, 30, ctx)
    assert max(map(len, seqs)) <= sc.dims["max_pos"]
    for rig in _rigs(sc, 150):
        rig.call([[2] + ctx], update=1)
        _, got, plan = rig.call(seqs)
        assert plan["reused"] == 70
        _contract(f"cache {name} trunk attention {rig.setting}", got, st, rd, inv, seqs)


@pytest.mark.parametrize("name", ["llama", "llama3"])
def test_a_corrupted_cache_entry_is_visible_where_it_is_used(name):
    """Cache 60 positions, then score a list whose context follows the chain for 40: R = 39.  One K element (in the last
    K / V head), one V element or one log-prob changed at a reused position changes the scores; the same at a position >= R,
    which the call overwrites (or, read-only, never reads), does not.  llama: 2 K / V heads; llama3: one for 8 query heads."""
    import torch
    sc = _sc(name)
    dm = sc.dims
    Hkv, hd = dm["n_kv_heads"], dm["d_model"] // dm["n_heads"]
    assert Hkv == {"llama": 2, "llama3": 1}[name]
    rng = np.random.default_rng(9)
    r = _rand(rng, dm["vocab"])
    chain = [2] + r(59)
    ctx = chain[:40] + r(30)
    seqs = [ctx + t for t in (r(8), r(5), r(11))]
    ref = _call(sc, seqs, True)
    kcol, vcol = (Hkv - 1) * hd + 3, Hkv * hd + (Hkv - 1) * hd + 6
    for setting in SETTINGS:
        for update in (1, 0):
            for what, pos, changes in (("K", 5, True), ("V", 37, True), ("logp", 12, True), ("logp", 39, True),
                                       ("K", 39, False), ("V", 45, False), ("logp", 40, False), ("K", 59, False)):
                rig = Rig(sc, 150, setting)
                rig.call([chain])
                assert rig.n == 60
                if what == "K":
                    rig.kv[1, pos, kcol] += 0.5
                elif what == "V":
                    rig.kv[0, pos, vcol] += 0.5
                else:
                    rig.logp[pos] += 0.25
                torch.cuda.synchronize()
                s, t, plan = rig.call(seqs, update=update)
                assert plan["reused"] == 39
                same = s.tobytes() == ref[0].tobytes() and all(x.tobytes() == y.tobytes() for x, y in zip(t, ref[1]))
                assert same != changes, (setting, update, what, pos)


def _layout(name):
    model, cfg = tiny_model(name)
    dims = R.llama_dims(cfg)
    return dims, R.llama_device_layout(state_of(model, TINY[name]["tie_word_embeddings"]), dims, R.rope_inv_freq(cfg))


def test_scorer_surface():
    """LlamaScorer(context_cache_tokens=...), as tests/test_gpu_clm_cache.py's test_scorer_surface for OptScorer: cached by
    default, use_cache=False gives the uncached call and its two-key last_stats, update_cache=False reads only, cache_reset
    forgets."""
    dims, lay = _layout("llama")
    plain = _sc("llama")
    assert plain.context_cache_tokens == 0 and plain.cache_len == 0
    with pytest.raises(ValueError, match="context cache"):
        plain.score([[2, 5]], use_cache=True)
    with pytest.raises(ValueError, match="max_pos"):
        R.LlamaScorer(dims, lay, "cuda", context_cache_tokens=dims["max_pos"] + 1)
    sc = R.LlamaScorer(dims, lay, "cuda", context_cache_tokens=64)
    assert sc.cache_len == 0 and sc.share_prefixes is False and sc.context_cache_tokens == 64
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
    closed loop does): a LlamaScorer with a context cache gives, field by field, the replies of one without, and reuses more
    at every sentence."""
    import json
    import evaluate_model_helpers as H
    from remote_lm import LocalLMService
    with open(os.path.join(ROOT, "tests", "golden", "llm_rescore.json")) as f:
        gold = json.load(f)
    dims, lay = _layout("qwen2")
    tok = R.WordTokenizer(vocab_size=dims["vocab"], bos_id=2, pad_id=1)
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies, reused = {}, {}
    for cache_tokens in (0, 128):
        sc = R.LlamaScorer(dims, lay, "cuda", context_cache_tokens=cache_tokens)
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
    print(f"CLM llama cache service: reused per sentence {reused[128]}")
    assert reused[0] == [None, None, None]
    assert reused[128][0] == 0 and reused[128][0] < reused[128][1] < reused[128][2], reused
