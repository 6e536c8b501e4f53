"""Host-side checks of csrc/causal_lm_tree.hip (no GPU): the shared-prefix plan b2t_clm_tree_plan_host against a dictionary
restatement (prefix tuple -> node), the node counts of the recorded n-best lists, b2t_clm_tree_ws_bytes, the refusals of
b2t_clm_score_tree_f16 (all before any device work, so fake non-null weight pointers will do) and the kernels' resources."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden")
FAKE = 0x10000   # a non-null "device" pointer that is never dereferenced


def _pack(seqs):
    ids = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in seqs]).astype(np.int32))
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return ids, off


def dict_plan(seqs):
    """The definition restated: a node per distinct prefix tuple, numbered by first appearance."""
    nodes, node_of_token, parent = {}, [], []
    for s in seqs:
        for p in range(len(s)):
            key = tuple(int(x) for x in s[:p + 1])
            if key not in nodes:
                nodes[key] = len(nodes)
                parent.append(nodes[key[:-1]] if p else -1)
            node_of_token.append(nodes[key])
    return np.array(node_of_token, np.int32), np.array(parent, np.int32), len(nodes)


def _check(seqs):
    import llm_rescore as R
    ids, off = _pack(seqs)
    node, parent, n = R.tree_plan(ids, off)
    rn, rp, rc = dict_plan(seqs)
    assert n == rc and node.tolist() == rn.tolist() and parent.tolist() == rp.tolist(), (n, rc)
    # structure: inside a sequence a token's node hangs under the previous token's node; first tokens are roots
    for s in range(len(seqs)):
        a, b = off[s], off[s + 1]
        assert parent[node[a]] == -1
        assert (parent[node[a + 1:b]] == node[a:b - 1]).all()
    # first appearance numbering: the running maximum grows by at most one
    assert node[0] == 0 and (np.diff(np.maximum.accumulate(node)) <= 1).all() and node.max() == n - 1
    return node, parent, n


def _golden_lists():
    """(case, context, token id lists) of the recorded decode cases: the non-empty sentences as recorded, the context string
    glued in front with one space, word-tokenised (BOS first)."""
    import llm_rescore as R
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(**gold["tokenizer"])
    out = []
    for c in gold["decode"]:
        ctx = c["context"] if c["context"] is not None and c["context"].split() else None
        hyps = [e[0].strip() for e in c["nbest"] if e[0].strip()]
        hyps = [ctx + " " + h if ctx else h for h in hyps]
        out.append((c["case"], ctx, tok(hyps)["input_ids"]))
    return out


# tokens -> nodes of the recorded lists: properties of the fixture, counted with dict_plan and WordTokenizer
COUNTS = {(0, None): (19, 130, 50), (0, "well then"): (19, 168, 52), (1, None): (6, 40, 23), (1, "well then"): (6, 52, 25),
          (2, None): (5, 12, 6), (2, "well then"): (5, 22, 8), (3, None): (1, 3, 3), (3, "well then"): (1, 5, 5)}


def test_plan_on_recorded_nbest_lists():
    lists = _golden_lists()
    assert {(c, x) for c, x, _ in lists} == set(COUNTS)
    for case, ctx, seqs in lists:
        _, _, n = _check(seqs)
        tokens = sum(map(len, seqs))
        assert (len(seqs), tokens, n) == COUNTS[(case, ctx)], (case, ctx, len(seqs), tokens, n)


def test_sharing_exists_on_recorded_lists_with_context():
    for case, ctx, seqs in _golden_lists():
        if ctx is None:
            continue
        ids, off = _pack(seqs)
        import llm_rescore as R
        n = R.tree_plan(ids, off)[2]
        tokens = len(ids)
        print(f"CLM tree case {case} ({len(seqs)} candidates, context {ctx!r}): {tokens} tokens -> {n} nodes "
              f"({n / tokens:.2f})")
        if len(seqs) >= 2:
            assert n < tokens, (case, n, tokens)
        else:
            assert n == tokens, (case, n, tokens)


def test_plan_on_constructed_lists():
    rng = np.random.default_rng(0)
    # random lists over a tiny alphabet (much accidental sharing) and a large one (almost none)
    for V in (3, 5, 50000):
        for _ in range(20):
            seqs = [[2] + list(rng.integers(0, V, int(n))) for n in rng.integers(0, 12, int(rng.integers(1, 30)))]
            _check(seqs)
    # exact duplicates map to the same nodes throughout
    a, b = [2, 7, 8, 9], [2, 7, 5]
    node, _, n = _check([a, b, a, a, b])
    assert n == 5 and node[7:11].tolist() == node[0:4].tolist() and node[15:18].tolist() == node[4:7].tolist()
    # one-token sequences, equal and different
    _, parent, n = _check([[2], [2], [3], [2], [4]])
    assert n == 3 and (parent == -1).all()
    # different first tokens: a forest; the same tail under two roots is two chains
    _, parent, n = _check([[2, 5, 6], [3, 5, 6], [2, 5, 7], [3, 5]])
    assert n == 7 and (parent == -1).sum() == 2
    # a prefix of an earlier candidate, and an extension of one
    _, _, n = _check([[2, 5, 6, 7], [2, 5], [2, 5, 6, 7, 8]])
    assert n == 5
    # the same ids at different positions are different nodes
    _, _, n = _check([[2, 5, 5, 5], [2, 5, 5]])
    assert n == 4
    # no sharing: the identity
    seqs = [[10 * i + j for j in range(1, 6)] for i in range(1, 9)]
    node, _, n = _check(seqs)
    assert n == 40 and node.tolist() == list(range(40))
    # a lone sequence
    node, parent, n = _check([[2, 9, 9, 9, 4]])
    assert node.tolist() == [0, 1, 2, 3, 4] and parent.tolist() == [-1, 0, 1, 2, 3]


def test_plan_cap_and_refusals():
    import b2t_native as N
    lib = N.load()
    seqs = [[2, 5, 6, 7], [2, 5, 8], [3, 5, 8]]
    ids, off = _pack(seqs)
    rn, rp, rc = dict_plan(seqs)
    assert rc == 8

    def plan(cap, ids=ids, off=off, node=True, parent=True, nn=True):
        nd = np.full(len(ids), -7, np.int32)
        pr = np.full(16, -7, np.int32)
        n = C.c_longlong(-7)
        rc_ = lib.b2t_clm_tree_plan_host(ids.ctypes.data, off.ctypes.data, len(off) - 1, nd.ctypes.data if node else None,
                                         pr.ctypes.data if parent else None, cap, C.byref(n) if nn else None)
        return rc_, nd, pr, n.value

    rc_, nd, pr, n = plan(8)
    assert rc_ == 0 and n == 8 and nd.tolist() == rn.tolist() and pr[:8].tolist() == rp.tolist() and (pr[8:] == -7).all()
    rc_, nd, pr, n = plan(16)
    assert rc_ == 0 and n == 8 and (pr[8:] == -7).all()
    for cap in (7, 3, 1, 0):
        rc_, nd, pr, n = plan(cap)
        assert rc_ == -2 and re.search("room for", N.last_error()), (cap, rc_)
        assert (pr[cap:] == -7).all(), cap                       # nothing past cap
        assert pr[:cap].tolist() == rp[:cap].tolist() and n == 8 and nd.tolist() == rn.tolist()
    assert plan(8, node=False)[0] == 2 and re.search("null", N.last_error())
    assert plan(8, parent=False)[0] == 2
    assert plan(8, nn=False)[0] == 2
    assert plan(8, off=np.array([1, 4, 7, 10], np.int32))[0] == 2 and re.search(r"seq_off\[0\] = 1", N.last_error())
    assert plan(8, off=np.array([0, 4, 4, 10], np.int32))[0] == 2 and re.search("empty", N.last_error())


def _model(n_layers=1, d=256, heads=4, ffn=512, vocab=1000, max_pos=64):
    import b2t_native as N
    layers = (N.ClmLayer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmLayer._fields_:
            setattr(layers[i], f, FAKE)
    desc = N.ClmDesc(n_layers, d, heads, ffn, vocab, max_pos, FAKE, FAKE, FAKE, FAKE, layers)
    desc._keep = layers
    return desc


def _ws(lib, desc, n_nodes, n_tokens, n_seq):
    return lib.b2t_clm_tree_ws_bytes(C.byref(desc), n_nodes, n_tokens, n_seq)


def test_tree_ws_bytes():
    import b2t_native as N
    lib = N.load()
    desc = _model()
    assert lib.b2t_clm_tree_ws_bytes(None, 5, 10, 1) == 0
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert _ws(lib, desc, nn, nt, ns) == 0, (nn, nt, ns)
    d, F, V = 256, 512, 1000
    ncg = (V + 63) // 64
    for M in (1, 2, 255, 256, 257, 600, 4097):
        for Mn in sorted({1, M // 2 + 1, M}):
            for n_seq in sorted({1, max(1, M // 3), M}):
                b = _ws(lib, desc, Mn, M, n_seq)
                Mp = -(-Mn // 256) * 256
                # the node-sized buffers of the forward, a head row per node at most, the token-sized maps
                parts = [4 * (4 * Mn + 2 * M + 2 * n_seq + 1), 4 * Mn * d, 2 * Mp * d, 2 * Mn * 3 * d, 2 * Mp * F,
                         4 * Mn * ncg, 4 * Mn * ncg, 4 * Mn, 4 * Mn]
                assert b >= sum(parts) and b % 256 == 0, (Mn, M, n_seq, b, sum(parts))
    # non-decreasing in each argument
    s = [_ws(lib, desc, Mn, 3000, 7) for Mn in range(1, 3001, 11)]
    assert all(a > 0 for a in s) and all(a <= b for a, b in zip(s, s[1:]))
    s = [_ws(lib, desc, 40, M, 7) for M in range(40, 3000, 13)]
    assert all(a > 0 for a in s) and all(a <= b for a, b in zip(s, s[1:]))
    s = [_ws(lib, desc, 40, 3000, n) for n in range(1, 3001, 17)]
    assert all(a > 0 for a in s) and all(a <= b for a, b in zip(s, s[1:]))
    # with every token its own node the tree path needs no less than the node-sized part of the flat path's buffers, and
    # sharing shrinks it
    assert _ws(lib, desc, 500, 2500, 100) < _ws(lib, desc, 2500, 2500, 100)


def _call(lib, desc, ids, off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    return lib.b2t_clm_score_tree_f16(C.byref(desc) if desc is not None else None, ids.ctypes.data, off.ctypes.data,
                                      len(off) - 1 if n_seq is None else n_seq, scores, None, None, ws, ws_bytes, None)


def test_tree_score_refusals_before_device_work():
    """Every refusal of the flat call (tests/test_clm_host.py) is one here."""
    import b2t_native as N
    lib = N.load()
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, **kw):
        rc = _call(lib, desc, ids, off, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())

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
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    # the workspace: one byte less than the plan's node count needs, with and without sharing
    desc = _model()
    need = _ws(lib, desc, 4, 4, 2)
    assert need > 0
    refused("workspace", desc, ws_bytes=need - 1)
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes
    need = _ws(lib, desc, 4, 9, 3)
    assert 0 < need <= _ws(lib, desc, 9, 9, 3)
    refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)
    # null ids / offsets
    rc = lib.b2t_clm_score_tree_f16(C.byref(desc), None, None, 1, FAKE, None, None, FAKE, 1 << 30, None)
    assert rc != 0 and re.search("null argument", N.last_error())


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_tree_kernels_do_not_spill():
    # the bound of tests/test_clm_host.py; at the time of writing the three attention instances use 113 / 151 / 202 VGPRs and
    # 32 / 48 / 64 AGPRs, scratch 0.  clm_attn_tree_kernel is the Llama family's tree attention too
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm_tree.hip").items() if "clm_" in k}
    attn = [k for k in res if "clm_attn_tree_kernel" in k]
    assert len(attn) == 3 and any("clm_seq_sum_tree_kernel" in k for k in res) and len(res) == 4, sorted(res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_python_surface_defaults():
    """share_prefixes is off unless asked for, on OptScorer, build_opt and the two scoring calls."""
    import inspect
    import llm_rescore as R
    assert inspect.signature(R.OptScorer.__init__).parameters["share_prefixes"].default is False
    assert inspect.signature(R.build_opt).parameters["share_prefixes"].default is False
    assert inspect.signature(R.OptScorer.score).parameters["share_prefixes"].default is None
    assert inspect.signature(R.OptScorer.token_logprobs).parameters["share_prefixes"].default is None
    assert list(inspect.signature(R.OptScorer.score).parameters)[:3] == ["self", "ids_list", "length_penalty"]
