"""Host-side checks of csrc/causal_lm_cache.hip (no GPU): the cache rule b2t_clm_cache_plan_host against a dictionary
restatement (on the recorded n-best lists chained into a session and on constructed lists), b2t_clm_cache_kv_bytes and
b2t_clm_tree_cached_ws_bytes as host arithmetic, the refusals of b2t_clm_score_tree_cached_f16 (all before any device work, so
fake non-null pointers will do), the struct layout against the C compiler, the kernels' resources and the Python defaults."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from test_clm_tree_host import FAKE, GOLD, _model, _pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def dict_rule(cache, cap, seqs):
    """The rule restated: trunk = the longest prefix common to all sequences, P = its common prefix with the cached chain,
    R = max(P - 1, 0), nodes = distinct prefix tuples, rows = nodes - R, the cache afterwards holds min(Tn, cap) positions."""
    seqs = [[int(x) for x in s] for s in seqs]
    cache = [int(x) for x in cache]
    tn = 0
    while all(len(s) > tn for s in seqs) and len({s[tn] for s in seqs}) == 1:
        tn += 1
    p = 0
    while p < tn and p < len(cache) and cache[p] == seqs[0][p]:
        p += 1
    r = max(p - 1, 0)
    nodes = len({tuple(s[:k + 1]) for s in seqs for k in range(len(s))})
    return {"trunk": tn, "common": p, "reused": r, "nodes": nodes, "rows": nodes - r, "n_after": min(tn, cap)}


def _check(cache, cap, seqs):
    import llm_rescore as R
    ids, off = _pack(seqs)
    got = R.cache_plan(np.asarray(cache, np.int32), cap, ids, off)
    want = dict_rule(cache, cap, seqs)
    assert got == want, (cache, cap, seqs, got, want)
    assert got["nodes"] == R.tree_plan(ids, off)[2]
    assert got["rows"] >= 1 and (got["reused"] < got["trunk"] or got["reused"] == 0)
    return got


def golden_session(order=(0, 1, 2, 3, 0, 1, 2, 0)):
    """The recorded n-best lists as a conversation: call k scores case order[k] behind the context = the first candidates of
    the calls before it, the strings glued and normalised as gpt2_lm_decode does, word-tokenised (BOS first)."""
    import llm_rescore as R
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(**gold["tokenizer"])
    cases = {}
    for c in gold["decode"]:
        cases.setdefault(c["case"], [e[0].strip() for e in c["nbest"] if e[0].strip()])
    ctx, calls = "", []
    for k in order:
        hyps = [R._normalise(ctx + " " + h if ctx.split() else h) for h in cases[k]]
        calls.append([np.asarray(r, np.int32) for r in tok(hyps)["input_ids"]])
        ctx = (ctx + " " + cases[k][0]).strip()
    return calls


# per call of golden_session(): trunk, reused, rows computed, tree nodes -- properties of the fixture, counted with a Python
# restatement of the rule before the library had one
SESSION = {"trunk": [1, 7, 12, 15, 15, 21, 26, 27], "reused": [0, 0, 6, 11, 14, 14, 20, 25],
           "rows": [50, 24, 11, 4, 50, 24, 11, 51], "nodes": [50, 24, 17, 15, 64, 38, 31, 76]}


def test_rule_on_the_recorded_lists_as_a_session():
    calls = golden_session()
    assert max(len(s) for seqs in calls for s in seqs) == 33
    cache, got = [], {k: [] for k in SESSION}
    for seqs in calls:
        p = _check(cache, 128, seqs)
        for k in got:
            got[k].append(p[k])
        # from the second call on the previous call's whole trunk is found again
        assert p["common"] == len(cache) and p["n_after"] == p["trunk"]
        cache = [int(x) for x in seqs[0][:p["n_after"]]]
    assert got == SESSION, got


def test_rule_on_constructed_lists():
    chain = [2, 11, 12, 13, 14, 15, 16, 17]
    tails = [[21, 22], [21, 23], [24]]
    seqs = [chain + t for t in tails]
    # empty cache, the cache = the trunk, longer and shorter than the trunk
    assert _check([], 64, seqs)["reused"] == 0
    p = _check(chain, 64, seqs)
    assert (p["trunk"], p["common"], p["reused"], p["rows"]) == (8, 8, 7, p["nodes"] - 7)
    assert _check(chain + [21, 22, 9], 64, seqs)["common"] == 8          # the cache goes on where the list forks
    assert _check(chain + [99, 98], 64, seqs)["common"] == 8
    assert _check(chain[:3], 64, seqs)["reused"] == 2
    assert _check(chain[:1], 64, seqs)["reused"] == 0                     # P = 1: position 0 is recomputed
    # divergence at every position of the chain
    for k in range(len(chain)):
        other = list(chain)
        other[k] = 999
        p = _check(other, 64, seqs)
        assert p["common"] == k and p["reused"] == max(k - 1, 0) and p["n_after"] == 8
    # cap smaller than the trunk: the cache stops at cap
    for cap in (1, 2, 7, 8, 9):
        p = _check(chain[:min(cap, 5)], cap, seqs)
        assert p["n_after"] == min(cap, 8) and p["common"] == min(cap, 5)
    # a forest: no trunk, nothing reused, the cache empties
    p = _check(chain, 64, [[2, 5, 6], [3, 5, 6], [2, 5, 7]])
    assert (p["trunk"], p["common"], p["reused"], p["n_after"]) == (0, 0, 0, 0)
    # one sequence, and all equal: the trunk is the whole sequence
    p = _check(chain, 64, [chain])
    assert (p["trunk"], p["reused"], p["rows"]) == (8, 7, 1)
    p = _check(chain[:4], 64, [chain, chain, chain])
    assert (p["trunk"], p["reused"], p["nodes"], p["rows"]) == (8, 3, 8, 5)
    # a sequence that is a prefix of the others bounds the trunk
    p = _check(chain, 64, [chain + [5], chain[:4], chain + [6]])
    assert (p["trunk"], p["common"], p["reused"]) == (4, 4, 3)
    # random lists behind random chains
    rng = np.random.default_rng(0)
    for _ in range(200):
        pre = [2] + [int(x) for x in rng.integers(4, 7, int(rng.integers(0, 8)))]
        lists = [pre + [int(x) for x in rng.integers(4, 7, int(rng.integers(0, 5)))] for _ in range(int(rng.integers(1, 6)))]
        cache = (pre + [int(x) for x in rng.integers(4, 7, 3)])[:int(rng.integers(0, 12))]
        if rng.integers(0, 3) == 0 and cache:
            cache[int(rng.integers(0, len(cache)))] = 9
        cap = int(rng.integers(max(1, len(cache)), 16))
        _check(cache, cap, lists)


def test_plan_refusals():
    import b2t_native as N
    lib = N.load()
    ids, off = _pack([[2, 5, 6], [2, 5, 7]])
    cid = np.array([2, 5], np.int32)
    out = C.c_int(-7)

    def plan(cache=cid.ctypes.data, n=2, cap=8, ids_p=ids.ctypes.data, off_p=off.ctypes.data, n_seq=2):
        return lib.b2t_clm_cache_plan_host(cache, n, cap, ids_p, off_p, n_seq, C.byref(out), None, None, None, None, None)

    assert plan() == 0 and out.value == 2
    assert plan(cache=None, n=0) == 0
    assert plan(cache=None) == 2 and re.search("null", N.last_error())
    assert plan(ids_p=None) == 2 and plan(off_p=None) == 2
    assert plan(cap=0) == 2 and re.search("cap 0", N.last_error())
    assert plan(n=9) == 2 and re.search("outside", N.last_error())
    assert plan(n=-1) == 2
    assert plan(n_seq=0) == 2 and re.search("n_seq 0", N.last_error())
    bad = np.array([0, 3, 3], np.int32)
    assert plan(off_p=bad.ctypes.data) == 2 and re.search("empty", N.last_error())
    bad = np.array([1, 3, 6], np.int32)
    assert plan(off_p=bad.ctypes.data) == 2 and re.search(r"seq_off\[0\] = 1", N.last_error())


def test_cache_and_workspace_sizes_are_host_arithmetic():
    import b2t_native as N
    lib = N.load()
    desc = _model(n_layers=3, d=256, heads=4, ffn=512, vocab=1000, max_pos=64)
    kvb = lambda cap, m=desc: lib.b2t_clm_cache_kv_bytes(C.byref(m) if m is not None else None, cap)
    for cap in (1, 2, 33, 64):
        assert kvb(cap) == 3 * cap * 2 * 256 * 2
    assert kvb(0) == 0 and kvb(-1) == 0 and kvb(65) == 0 and kvb(8, None) == 0
    # OPT-6.7b: 512 KiB per position, 1 GiB for 2048
    big = _model(n_layers=32, d=4096, heads=32, ffn=16384, vocab=50272, max_pos=2048)
    assert kvb(1, big) == 512 << 10 and kvb(2048, big) == 1 << 30

    ws = lambda r, t, s: lib.b2t_clm_tree_cached_ws_bytes(C.byref(desc), r, t, s)
    tree = lambda r, t, s: lib.b2t_clm_tree_ws_bytes(C.byref(desc), r, t, s)
    assert lib.b2t_clm_tree_cached_ws_bytes(None, 5, 10, 1) == 0
    for r, t, s in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (3, 5, 0), (3, 5, 6)):
        assert ws(r, t, s) == 0, (r, t, s)
    for r, t, s in ((1, 1, 1), (1, 40, 1), (40, 400, 7), (257, 3000, 100), (3000, 3000, 100)):
        b = ws(r, t, s)
        # what the tree call needs for r rows, plus m, l per (row, head) and the unnormalised o per row in fp32
        assert b % 256 == 0 and b >= tree(r, t, s) + 4 * r * 4 * 2 + 4 * r * 256
        assert b <= tree(r, t, s) + 4 * r * 4 * 2 + 4 * r * 256 + 512
    s_ = [ws(r, 3000, 7) for r in range(1, 3001, 11)]
    assert all(a > 0 for a in s_) and all(a <= b for a, b in zip(s_, s_[1:]))
    s_ = [ws(40, t, 7) for t in range(40, 3000, 13)]
    assert all(a <= b for a, b in zip(s_, s_[1:]))
    s_ = [ws(40, 3000, n) for n in range(1, 3001, 17)]
    assert all(a <= b for a, b in zip(s_, s_[1:]))
    # the tree call's own size function did not move: no term for the state
    parts = [4 * (4 * 40 + 2 * 400 + 2 * 7 + 1), 4 * 40 * 256, 2 * 256 * 256, 2 * 40 * 3 * 256, 2 * 256 * 512,
             4 * 40 * 16, 4 * 40 * 16, 4 * 40, 4 * 40]
    assert tree(40, 400, 7) == sum(-(-p // 256) * 256 for p in parts)


def _cache(kv=FAKE, logp=FAKE, ids=(2, 5), cap=8, n=None):
    import b2t_native as N
    arr = np.zeros(max(cap, len(ids), 1), np.int32)
    arr[:len(ids)] = ids
    c = N.ClmCache(kv, logp, arr.ctypes.data, cap, len(ids) if n is None else n)
    c._keep = arr
    return c


def test_cached_score_refusals_before_device_work():
    """Every refusal of the tree call is one here, plus the cache's own."""
    import b2t_native as N
    lib = N.load()
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def call(desc, cache, ids=ok_ids, off=ok_off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        return lib.b2t_clm_score_tree_cached_f16(C.byref(desc) if desc is not None else None,
                                                 C.byref(cache) if cache is not None else None, update, ids.ctypes.data,
                                                 off.ctypes.data, len(off) - 1 if n_seq is None else n_seq, scores, None, None,
                                                 None, ws, ws_bytes, None)

    def refused(match, desc, cache=None, **kw):
        cache = _cache() if cache is None else cache
        n0, ids0 = cache.n, cache._keep.copy()
        rc = call(desc, cache, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        assert cache.n == n0 and (cache._keep == ids0).all()      # a refusal leaves the cache alone

    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8))
    refused("multiples of 64", _model(d=80, heads=1))
    refused("multiples of 64", _model(d=256, heads=4, ffn=500))
    refused("null weight", N.ClmDesc(0, 256, 4, 512, 1000, 64, FAKE, 0, FAKE, FAKE, None))
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), cache=_cache(cap=3), ids=[2, 5, 7, 9], off=[0, 4])
    # the cache's own
    rc = call(_model(), None)
    assert rc != 0 and re.search("null cache", N.last_error())
    refused("null cache member", _model(), cache=_cache(kv=None))
    refused("null cache member", _model(), cache=_cache(logp=None))
    c = _cache()
    c.ids_host = None
    rc = call(_model(), c)
    assert rc != 0 and re.search("null cache member", N.last_error())
    refused("cap 0", _model(), cache=_cache(ids=(), cap=0))
    refused("cap -1", _model(), cache=_cache(ids=(), cap=-1))
    refused("above max_pos", _model(max_pos=64), cache=_cache(cap=65))
    refused(r"n 9 outside", _model(), cache=_cache(cap=8, n=9))
    refused(r"n -1 outside", _model(), cache=_cache(cap=8, n=-1))
    refused("cached token 1 has id 1000", _model(vocab=1000), cache=_cache(ids=(2, 1000)))
    refused("cached token 0 has id -3", _model(vocab=1000), cache=_cache(ids=(-3, 5)))
    # the workspace: one byte less than the rows computed need, with and without reuse, updating or not
    desc = _model()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]              # 9 tokens, 4 nodes, trunk 2
    need = lib.b2t_clm_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
    refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
    need3 = lib.b2t_clm_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)  # the cache (2, 5) spares one row
    assert 0 < need3 <= need
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)


def test_cache_struct_layout_matches_the_header(tmp_path):
    """b2t_native.ClmCache against the C compiler's view of b2t_clm_cache_t, as tests/test_abi_host.py does for the others."""
    import shutil
    import subprocess
    import b2t_native as N
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in N.ClmCache._fields_]
    assert fields == ["kv", "logp", "ids_host", "cap", "n"]
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){ printf("%zu\\n", sizeof(b2t_clm_cache_t));\n' +
                   "".join(f'printf("{f} %zu\\n", offsetof(b2t_clm_cache_t, {f}));\n' for f in fields) + "return 0; }\n")
    exe = tmp_path / "lay"
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    assert int(out[0]) == C.sizeof(N.ClmCache)
    seen = 0
    for line in out[1:]:
        if line.strip():
            name, off = line.split()
            assert getattr(N.ClmCache, name).offset == int(off), name
            seen += 1
    assert seen == len(fields)


def test_header_cites_the_reference_lines():
    with open(os.path.join(ROOT, "include", "b2t.h")) as f:
        h = f.read()
    sec = h[h.index("b2t_clm_cache_t") - 3000:h.index("} b2t_clm_cache_t;")]
    assert "language-model-standalone.py:188-190" in sec and "577-583" in sec and "ordered by the caller" in sec


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_cache_kernels_do_not_spill():
    # at the time of writing the cached attention uses 115 / 150 / 184 VGPRs, the trunk attention 115 / 128 / 153, both
    # 32 / 48 / 64 AGPRs, scratch 0 throughout
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm_cache.hip").items() if "clm_" in k}
    for name, count in (("clm_attn_tree_cached_kernel", 3), ("clm_attn_trunk_kernel", 3), ("clm_cache_append_kernel", 1),
                        ("clm_cache_logp_kernel", 1), ("clm_seq_sum_tree_cached_kernel", 1)):
        assert len([k for k in res if name in k]) == count, (name, sorted(res))
    assert len(res) == 9, sorted(res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    # the tree path's translation unit still compiles to its four kernels
    tree = {k: v for k, v in W.resources(src="causal_lm_tree.hip").items() if "clm_" in k}
    assert len(tree) == 4 and len([k for k in tree if "clm_attn_tree_kernel" in k]) == 3, sorted(tree)
    assert all(v.get("ScratchSize", -1) == 0 for v in tree.values()), tree


def test_python_surface_defaults():
    """The cache is off unless asked for, on OptScorer, build_opt and the two scoring calls; the parameters the tree path
    pinned keep their places."""
    import inspect
    import llm_rescore as R
    assert inspect.signature(R.OptScorer.__init__).parameters["context_cache_tokens"].default == 0
    assert inspect.signature(R.build_opt).parameters["context_cache_tokens"].default == 0
    for fn in (R.OptScorer.score, R.OptScorer.token_logprobs):
        assert inspect.signature(fn).parameters["use_cache"].default is None
        assert inspect.signature(fn).parameters["update_cache"].default is True
    assert list(inspect.signature(R.OptScorer.score).parameters)[:5] == ["self", "ids_list", "length_penalty", "share_prefixes",
                                                                         "use_cache"]
    assert list(inspect.signature(R.OptScorer.__init__).parameters)[:6] == ["self", "dims", "arrays", "device", "share_prefixes",
                                                                            "context_cache_tokens"]
    assert list(inspect.signature(R.build_opt).parameters)[:5] == ["model_name", "cache_dir", "device", "share_prefixes",
                                                                   "context_cache_tokens"]
    assert callable(R.OptScorer.cache_reset) and isinstance(R.OptScorer.cache_len, property)
