"""b2t_clm_score_tree_f16 (csrc/causal_lm_tree.hip) on the MI355X: the shared-prefix tree path against the flat path
b2t_clm_score_f16, byte for byte, and against the fp64 restatement of tests/test_gpu_clm_contract.py.

Bit identity carries no tolerance.  Its premises: the embedding, LayerNorm, GEMM and head kernels are the flat path's own, and a
row's result there depends on neither M nor the row's index (test_gpu_llm_rescore.test_batch_invariance, the tile identity of
test_gpu_clm_contract); the tree attention keeps a query's arithmetic order; the sums follow the path in token order.  Every
call gets a fresh workspace of exactly the size asked for, filled with 0xFF (NaN in fp16 and fp32).

Planted bugs this file was checked against (NOTES.md "LLM" has the counts): path index off by one in the K/V gather, queries
started one position late, head source = the node instead of its parent, owner start index taken from the previous sequence,
the per-sequence sum taken in another order than the tokens' (node order along one path is token order: a parent is numbered
before its child; the planted sum ran from the last token to the first)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import llm_rescore as R
from test_gpu_clm_contract import BOUND, V_OPT, WIDTHS, _err, _logp, _model, _ref_logp, _same, _tiles
from test_gpu_llm_rescore import _tiny

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu


def _pack(seqs):
    ids = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in seqs]).astype(np.int32))
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return ids, off


def _tree(sc, seqs, mode=None, scores=False):
    """The tree path's per-sequence token log-probs (or scores) on a fresh poisoned workspace of exactly the size needed,
    under B2T_CLM_GEMM_256 = mode; checks last_stats against the host plan."""
    import torch
    import b2t_native as N
    ids, off = _pack(seqs)
    nodes = R.tree_plan(ids, off)[2]
    need = N.load().b2t_clm_tree_ws_bytes(C.byref(sc.desc), nodes, len(ids), len(seqs))
    assert need > 0
    sc._ws = None
    torch.cuda.empty_cache()
    sc._ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    with _tiles(mode):
        out = sc.score(seqs, share_prefixes=True) if scores else sc.token_logprobs(seqs, share_prefixes=True)
    assert sc._ws.numel() == need and sc.last_stats == {"tokens": len(ids), "nodes": nodes}
    sc._ws = None
    return out


def _flat_scores(sc, seqs, mode=None):
    import torch
    import b2t_native as N
    need = N.load().b2t_clm_ws_bytes(C.byref(sc.desc), sum(map(len, seqs)), len(seqs))
    sc._ws = None
    torch.cuda.empty_cache()
    sc._ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    with _tiles(mode):
        out = sc.score(seqs, share_prefixes=False)
    assert sc.last_stats == {"tokens": sum(map(len, seqs)), "nodes": sum(map(len, seqs))}
    sc._ws = None
    return out


def _identical(sc, seqs, mode=None, what=""):
    """Token log-probs and scores of the two paths, byte for byte; returns the flat log-probs."""
    flat = _logp(sc, seqs, mode)
    tree = _tree(sc, seqs, mode)
    assert all(np.isfinite(x).all() for x in flat), what
    bad = [i for i, (x, y) in enumerate(zip(flat, tree)) if x.tobytes() != y.tobytes()]
    if bad:
        i = bad[0]
        j = int(np.flatnonzero(flat[i].view(np.uint32) != tree[i].view(np.uint32))[0])
        raise AssertionError(f"{what} mode {mode}: {len(bad)} of {len(seqs)} sequences differ; first: sequence {i} token {j} "
                             f"flat {flat[i][j]!r} tree {tree[i][j]!r}")
    assert len(flat) == len(tree)
    a, b = _flat_scores(sc, seqs, mode), _tree(sc, seqs, mode, scores=True)
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
    return flat


def _golden_token_lists(gold):
    """The recorded n-best lists as gpt2_lm_decode hands them to the scorer, with the recorded context and without."""
    tok = R.WordTokenizer(**gold["tokenizer"])
    out = []
    for c in gold["decode"]:
        ctx = c["context"] if c["context"] is not None and c["context"].split() else None
        hyps = [e[0].strip() for e in c["nbest"] if e[0].strip()]
        hyps = [R._normalise(ctx + " " + h if ctx else h) for h in hyps]
        out.append((c["case"], ctx, [np.asarray(r, np.int32) for r in tok(hyps)["input_ids"]]))
    return out


def test_golden_lists_bit_identical():
    sc, _, gold = _tiny()
    seen = set()
    for case, ctx, seqs in _golden_token_lists(gold):
        if (case, ctx) in seen:
            continue
        seen.add((case, ctx))
        _identical(sc, seqs, what=f"golden case {case} context {ctx!r}")
        nodes = R.tree_plan(*_pack(seqs))[2]
        assert nodes < sum(map(len, seqs)) or len(seqs) == 1
    assert len(seen) == 8


def _nbest(V, seed, context, cands=100):
    import bench_llm_rescore as B
    rng = np.random.default_rng(seed)
    return B.nbest_list(rng, V, cands, [int(x) for x in rng.integers(4, V, context)])


@pytest.mark.parametrize("shape", ["d320", "1.3b", "2.7b", "6.7b"])
def test_nbest_list_with_context_bit_identical_on_every_tile_rule(shape):
    """An augment_nbest-style list of 100 candidates behind a 100-token context (about 12 000 tokens, 1 000 - 2 000 nodes),
    2 layers, under B2T_CLM_GEMM_256 = 0, unset and 2: the flat path runs its GEMMs at M = tokens, the tree path at M = nodes,
    so under the default rule the two may sit on different tiles."""
    d, H, F, V = (320, 4, 1216, 1000) if shape == "d320" else WIDTHS[shape] + (V_OPT,)
    sc, _, _ = _model(d, H, F, V)
    seqs = _nbest(V, seed=d, context=100)
    ids, off = _pack(seqs)
    nodes = R.tree_plan(ids, off)[2]
    print(f"CLM tree nbest {shape}: {len(ids)} tokens -> {nodes} nodes")
    assert len(seqs) == 100 and nodes * 4 < len(ids)
    ref = None
    for mode in ("0", None, "2"):
        flat = _identical(sc, seqs, mode, what=f"nbest {shape}")
        assert ref is None or _same(ref, flat)
        ref = flat


def _edge_model(hd):
    d = {64: 128, 80: 320, 128: 256}[hd]
    return _model(d, d // hd, 2 * d, 1000, max_pos=150)


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_owned_suffix_at_block_edges_and_max_pos(hd):
    """Pairs that share their first p tokens, p = 31, 32, 33, 63, 64, 65: the second of a pair owns positions p.., so its first
    owned position falls one before, on and one after a 32-row block edge; its 32-aligned query block then holds rows it must
    not write.  Then a 140-token context in front of four tails that bring the paths to max_pos = 150 and just below."""
    sc, _, _ = _edge_model(hd)
    rng = np.random.default_rng(hd)
    seqs = []
    for p in (31, 32, 33, 63, 64, 65):
        pre = [2] + list(rng.integers(4, 1000, p - 1))
        seqs.append(pre + list(rng.integers(4, 1000, 20)))
        seqs.append(pre + list(rng.integers(4, 1000, 45)))
        seqs.append(pre + list(rng.integers(4, 1000, 1)))
    ids, off = _pack(seqs)
    node, _, nodes = R.tree_plan(ids, off)
    # the first owned position of the 2nd and 3rd of each triple is p (the pair's prefixes differ from the other pairs' from
    # position 1 on)
    for k, p in enumerate((31, 32, 33, 63, 64, 65)):
        for j in (1, 2):
            s = 3 * k + j
            path = node[off[s]:off[s + 1]]
            assert (path[:p] == node[off[3 * k]:off[3 * k] + p]).all() and path[p] > node[off[s] - 1]
    _identical(sc, seqs, what=f"block edges hd {hd}")
    ctx = [2] + list(rng.integers(4, 1000, 139))
    seqs = [ctx + list(rng.integers(4, 1000, n)) for n in (10, 10, 9, 1)] + [ctx]
    assert max(map(len, seqs)) == 150 == sc.dims["max_pos"]
    _identical(sc, seqs, what=f"max_pos hd {hd}")


def test_duplicates_forest_no_sharing_lone_sequence():
    sc, _, _ = _edge_model(64)
    rng = np.random.default_rng(1)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    a, b = [2] + r(37), [2] + r(12)
    cases = {"duplicates": [a, b, a, a, b, a[:20], a + r(3)],
             "forest": [[2] + r(9), [3] + r(9), [2] + r(40), [3], [2], [5, 6], [3] + r(33)],
             "no sharing": [[10 + i] + r(5 + 7 * i) for i in range(8)],
             "lone": [[2] + r(70)],
             "one token": [[2]],
             "one-token sequences": [[2], [3], [2]]}
    fo = cases["forest"]
    fo.append(fo[0][:5] + r(4)); fo.append(fo[6][:30] + r(4))
    for what, seqs in cases.items():
        ids, off = _pack(seqs)
        node, _, nodes = R.tree_plan(ids, off)
        if what in ("no sharing", "lone", "one token"):
            assert nodes == len(ids) and node.tolist() == list(range(len(ids)))
        else:
            assert nodes < len(ids)
        _identical(sc, seqs, what=what)


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_tree_path_within_fp64_bound(hd):
    """Pinned to the fp64 restatement of the contract, not only to the flat path: one shared-context list per head dim, at
    test_gpu_clm_contract's bound of 1e-2 on |dlogp| (the flat path measured 1.2e-3 .. 3.8e-3 there)."""
    sc, st, dims = _edge_model(hd)
    seqs = _nbest(1000, seed=hd, context=60, cands=30)
    assert max(map(len, seqs)) <= dims["max_pos"]
    got = _tree(sc, seqs)
    err, mx = _err(got, _ref_logp(st, dims, seqs))
    ids, off = _pack(seqs)
    print(f"CLM tree fp64 hd {hd}: {len(ids)} tokens -> {R.tree_plan(ids, off)[2]} nodes, max |dlogp| {err:.3e} "
          f"(max |logp| {mx:.2f})")
    assert err <= BOUND, (hd, err)


def test_a_wrong_gather_is_visible():
    """Two candidates share 40 tokens and differ in the next: identical log-probs up to the split, different ones after it
    (a path that followed the other branch, or a head row fed by the wrong parent, would repeat them).  A candidate inside a
    shared list equals itself alone on the flat path.  Swapping two sibling branches in the input order permutes the results
    and changes nothing else."""
    sc, _, _ = _edge_model(64)
    rng = np.random.default_rng(8)
    r = lambda n: [int(x) for x in rng.integers(4, 1000, n)]
    pre = [2] + r(39)
    tail = r(12)
    a, b = pre + [7] + tail, pre + [8] + tail          # same ids after the split too: only the prefix tells them apart
    c = pre[:20] + r(25)
    seqs = [a, b, c, pre + [9]]
    ta = _tree(sc, seqs)
    assert ta[0][:40].tobytes() == ta[1][:40].tobytes() and ta[0][1:40].all()
    assert ta[0][40] != ta[1][40]                      # different targets from the same row
    assert (ta[0][41:] != ta[1][41:]).all()            # same targets from different rows
    assert ta[2][:20].tobytes() == ta[0][:20].tobytes() and ta[2][20] != ta[0][20]
    for i, s in enumerate(seqs):
        assert ta[i].tobytes() == _logp(sc, [s])[0].tobytes(), i
    swapped = [b, a, c, pre + [9]]
    tb = _tree(sc, swapped)
    assert tb[0].tobytes() == ta[1].tobytes() and tb[1].tobytes() == ta[0].tobytes()
    assert tb[2].tobytes() == ta[2].tobytes() and tb[3].tobytes() == ta[3].tobytes()
    sa, sb = _tree(sc, seqs, scores=True), _tree(sc, swapped, scores=True)
    assert sa[[1, 0, 2, 3]].tobytes() == sb.tobytes() and sa[0] != sa[1]


@pytest.mark.parametrize("mode", ["0", "2"])
def test_tree_abi_with_canaries(mode):
    """The ABI driven directly: a workspace of exactly b2t_clm_tree_ws_bytes(plan's n_nodes) bytes filled with 0xFF gives the
    same bits as a zeroed one and as the flat call; the canaries behind the workspace, scores_out and tok_logp_out are
    untouched; n_nodes_out is the host plan's; the scores without tok_logp_out equal those with it."""
    import torch
    import b2t_native as N
    lib = N.load()
    sc, _, _ = _model(576, 9, 1344, 65)
    rng = np.random.default_rng(3)
    r = lambda n: [int(x) for x in rng.integers(0, 65, n)]
    pre = [2] + r(32)
    seqs = [pre + r(37), [2], pre + r(96), pre[:5], pre + r(8), [3] + r(40), pre + r(37)]
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    nodes = R.tree_plan(ids, off)[2]
    assert nodes < M
    need = lib.b2t_clm_tree_ws_bytes(C.byref(sc.desc), nodes, M, S)
    assert need > 0
    canary = torch.randint(0, 256, (CAN,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(fill, with_tok, with_n=True):
        ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
        ws[:need] = fill
        ws[need:] = canary
        scores = torch.full((S + 64,), 12345.0, device="cuda")
        tok = torch.full((M + 64,), 12345.0, device="cuda")
        n = C.c_longlong(-1)
        with _tiles(mode):
            rc = lib.b2t_clm_score_tree_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                            tok.data_ptr() if with_tok else None, C.byref(n) if with_n else None,
                                            ws.data_ptr(), need, stream)
        assert rc == 0, N.last_error()
        torch.cuda.synchronize()
        assert n.value == (nodes if with_n else -1)
        assert torch.equal(ws[need:], canary)
        assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
        if not with_tok:
            assert (tok == 12345.0).all()
        return scores[:S].cpu().numpy(), tok[:M].cpu().numpy()

    s_p, t_p = run(0xFF, True)
    s_z, t_z = run(0, True)
    s_n, _ = run(0xFF, False, with_n=False)
    assert np.isfinite(s_p).all() and np.isfinite(t_p).all()
    assert s_p.tobytes() == s_z.tobytes() and t_p.tobytes() == t_z.tobytes()
    assert s_n.tobytes() == s_p.tobytes()
    assert (t_p[off[:-1]] == 0).all()
    flat = np.concatenate(_logp(sc, seqs, mode))
    assert flat.tobytes() == t_p.tobytes()
    # one byte less is refused before any launch
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.b2t_clm_score_tree_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, canary.data_ptr(), None, None,
                                    ws.data_ptr(), need - 1, stream)
    assert rc != 0 and "workspace" in N.last_error()


def test_scorer_default_and_override():
    sc, _, gold = _tiny()
    assert sc.share_prefixes is False and sc.last_stats is None
    seqs = [[2, 9, 8, 7], [2, 9, 8, 6], [2, 9, 5]]
    a = sc.score(seqs, 0.5)
    assert sc.last_stats == {"tokens": 11, "nodes": 11}
    b = sc.score(seqs, 0.5, share_prefixes=True)
    assert sc.last_stats == {"tokens": 11, "nodes": 6}
    sc.share_prefixes = True
    c = sc.score(seqs, 0.5)
    assert sc.last_stats == {"tokens": 11, "nodes": 6}
    d = sc.score(seqs, 0.5, share_prefixes=False)
    assert sc.last_stats == {"tokens": 11, "nodes": 11}
    assert a.tobytes() == b.tobytes() == c.tobytes() == d.tobytes()
    assert len(sc.score([], share_prefixes=True)) == 0 and sc.last_stats == {"tokens": 0, "nodes": 0}
    tok = R.WordTokenizer(**gold["tokenizer"])
    assert R.rescore_with_gpt2(sc, tok, "cuda", ["the cat sat", "the cat sat on", "the bat"], 0.0) is not None
    assert sc.last_stats["nodes"] < sc.last_stats["tokens"]
    with pytest.raises(RuntimeError, match="outside"):
        sc.score([[2, 5, 99999]], share_prefixes=True)
    with pytest.raises(RuntimeError, match="max_pos"):
        sc.score([[2] * (sc.dims["max_pos"] + 1)], share_prefixes=True)


def test_service_reply_is_the_same_with_shared_prefixes():
    """LocalLMService with do_opt = 1 and a context string: a scorer built with share_prefixes=True gives the reply (strings
    and the scoring field) of one built with False, and has computed fewer rows."""
    import evaluate_model_helpers as H
    import lm_decoder, ngram_lm
    from remote_lm import LocalLMService
    _, z, gold = _tiny()
    import torch
    cfg = gold["config"]
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    dims = R.opt_dims(cfg)
    Cc = 41
    prons = ngram_lm.synthetic_lexicon(200, Cc, seed=5)
    lex = ngram_lm.Lexicon(prons, Cc)
    wlm = ngram_lm.SparseNGramLM.from_arpa(ngram_lm.synthetic_word_arpa(lex.words, 2, 400, seed=2), lex.words)
    res = lm_decoder.DecodeResource("", "", "", "", "")
    res.set_lexicon_lm(lex, wlm, sil=1)
    tok = R.WordTokenizer(**gold["tokenizer"])
    rs = np.random.RandomState(0)
    words = [lex.words[i] for i in rs.randint(0, 200, size=4)]
    frames = []
    for w in words:
        for c in list(prons[w][0]) + [1]:
            frames += [c, 0]
    lg = np.full((len(frames), Cc), -1.0, dtype=np.float32)
    for t, c in enumerate(frames):
        lg[t, c] = 2.0
    replies, stats = [], []
    for share in (False, True):
        sc = R.OptScorer(dims, R.device_layout(state, dims), "cuda", share_prefixes=share)
        opts = lm_decoder.DecodeOptions(7000, 200, 17.0, 8.0, 0.35, 0.95, 0.0, 10)
        opts.lm_alpha, opts.lm_beta = 0.8, 0.0
        dec = lm_decoder.BrainSpeechDecoder(res, opts, max_len=128)
        r = LocalLMService(dec, acoustic_scale=0.35, blank_penalty=9.0, nbest=10, llm=(sc, tok), do_opt=1, alpha=0.5,
                           top_candidates_to_augment=5)
        r.set("contextual_decoding_current_context", "well then we went home")
        seen = H.get_current_redis_time_ms(r)
        H.reset_remote_language_model(r, seen)
        H.send_logits_to_remote_lm(r, 'remote_lm_input', 'remote_lm_output_partial', seen, lg)
        H.finalize_remote_lm(r, 'remote_lm_output_final', seen)
        replies.append(r.streams['remote_lm_output_final'][-1][1])
        stats.append(sc.last_stats)
    a, b = replies
    assert set(a) == set(b) and b"scoring" in a and a[b"context_str"] == b"well then we went home"
    for k in a:
        assert a[k] == b[k], k
    n_cand = len(a[b"scoring"].split(b";")) // 5     # five fields per candidate
    print(f"CLM tree service: {n_cand} candidates, {stats[1]['tokens']} tokens -> {stats[1]['nodes']} nodes")
    assert n_cand >= 1 and stats[0]["nodes"] == stats[0]["tokens"] == stats[1]["tokens"], stats
    assert stats[1]["nodes"] < stats[1]["tokens"] if n_cand >= 2 else stats[1]["nodes"] == stats[1]["tokens"], stats


class _Res:
    def __init__(self, sentence, ac, lm):
        self.sentence, self.ac_score, self.lm_score = sentence, ac, lm


class _ListDecoder:
    """A decoder that answers with a fixed n-best list (the service's decoder surface: Reset / FinishDecoding / result)."""

    def __init__(self, nbest):
        self.nbest = [_Res(*e[:3]) for e in nbest]

    def Reset(self):
        pass

    def FinishDecoding(self):
        pass

    def result(self):
        return self.nbest


def test_service_on_a_recorded_list_with_context():
    """The service's finalize on the recorded 19-candidate list (grown by augment_nbest) behind a context string: the reply of
    a scorer with share_prefixes=True is the reply of one without, from about a third of the rows."""
    import evaluate_model_helpers as H
    import torch
    from remote_lm import LocalLMService
    _, z, gold = _tiny()
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    dims = R.opt_dims(gold["config"])
    tok = R.WordTokenizer(**gold["tokenizer"])
    nbest = gold["decode"][0]["nbest"]
    assert len(nbest) == 19
    replies, stats = [], []
    for share in (False, True):
        sc = R.OptScorer(dims, R.device_layout(state, dims), "cuda", share_prefixes=share)
        r = LocalLMService(_ListDecoder(nbest), acoustic_scale=0.3, alpha=0.5, nbest=100, decode_fn=lambda *a: None,
                           llm=(sc, tok), do_opt=1, top_candidates_to_augment=20)
        r.set("contextual_decoding_current_context", "well then we all went home")
        t0 = H.get_current_redis_time_ms(r)
        H.reset_remote_language_model(r, t0)
        r.xadd("remote_lm_finalize", {"done": 0})
        replies.append(r.streams["remote_lm_output_final"][-1][1])
        stats.append(sc.last_stats)
    a, b = replies
    assert a == b and a[b"context_str"] == b"well then we all went home" and a[b"lm_response_final"]
    fields = a[b"scoring"].decode().split(";")
    assert len(fields) >= 5 * 19 and all(float(v) != 0.0 for v in fields[3::5])
    print(f"CLM tree service, recorded list: {len(fields) // 5} candidates, {stats[1]['tokens']} tokens -> {stats[1]['nodes']} nodes")
    assert stats[0]["nodes"] == stats[0]["tokens"] == stats[1]["tokens"] and 2 * stats[1]["nodes"] < stats[1]["tokens"], stats
