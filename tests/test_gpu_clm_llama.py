"""b2t_clm_llama_score_f16 / b2t_clm_llama_score_tree_f16 (csrc/causal_lm_llama.hip) on the MI355X, driven through the C
ABI: against the float64 restatement of the contract (_ref_logp_llama of tests/test_clm_llama_host.py, on the GPU here),
against HF fp32, tree against flat byte for byte, the rotary and grouped-query edges, and the service end to end.

Every call (_call) gets a fresh workspace of exactly the size the library asks for, filled with 0xFF (NaN in fp16 and fp32),
with canaries behind it and behind both outputs.

The contract bound is measured per case, not guessed: e16 = max |rounded restatement - unrounded restatement| is what the
contract's fp16 roundings alone do to the log-probs of that case; the kernels must be within 3 x e16 of the rounded
restatement (the margin covers accumulation order and the fast exponentials), and never looser than the 1e-2 of
tests/test_gpu_clm_contract.py.  The measured ratios are in NOTES.md ("LLM")."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_llama_host import TINY, _ref_logp_llama, hf_inv_freq, hf_logp, ref_dims, state_of, tiny_model, tiny_seqs

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENV = "B2T_CLM_GEMM_256"
pytestmark = pytest.mark.gpu

# (d, Hq, Hkv, F, vocab, q / k / v biases, tied head, rope theta): one layer of these widths plus the head
WIDTHS = {"llama3.2-1b": (2048, 32, 8, 8192, 128256, False, True, 500000.0),
          "llama3-8b": (4096, 32, 8, 14336, 128256, False, False, 500000.0),
          "qwen2.5-7b": (3584, 28, 4, 18944, 152064, True, False, 1000000.0)}


@contextlib.contextmanager
def _tiles(mode):
    old = os.environ.get(ENV)
    if mode is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = mode
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


def _pack(seqs):
    ids = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int64) for s in seqs]).astype(np.int32))
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return ids, off


def _call(sc, seqs, tree=False, mode=None, fill=0xFF, with_tok=True, finite=True, family="llama"):
    """(scores, per-sequence token log-probs) of one C ABI call of the scorer's family (b2t_clm_<sc._family>_score_* in the
    scorer's dtype, with sc._qk between the model and the lists; the sizes by sc._SIZES with sc._size_args) on a fresh workspace
    of exactly the size asked for.  family: what sc._family must be (the other families' files pass theirs); finite=False skips
    the assertion that every output is finite."""
    import torch
    import b2t_native as N
    lib = N.load()
    assert sc._family == family
    desc = C.byref(sc.desc)
    pre, sfx = f"b2t_clm_{sc._family}_score_", "bf16" if sc.dtype is torch.bfloat16 else "f16"
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    if tree:
        nodes = R.tree_plan(ids, off)[2]
        need = getattr(lib, sc._SIZES + "tree_ws_bytes")(desc, *sc._size_args, nodes, M, S)
    else:
        need = getattr(lib, sc._SIZES + "ws_bytes")(desc, *sc._size_args, M, S)
    assert need > 0
    canary = torch.randint(0, 256, (CAN,), dtype=torch.uint8, device="cuda")
    ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
    ws[:need] = fill
    ws[need:] = canary
    scores = torch.full((S + 64,), 12345.0, device="cuda")
    tok = torch.full((M + 64,), 12345.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with _tiles(mode):
        if tree:
            nn = C.c_longlong(-1)
            rc = getattr(lib, pre + "tree_" + sfx)(desc, *sc._qk, ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                                   tok.data_ptr() if with_tok else None, C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == nodes
        else:
            rc = getattr(lib, pre + sfx)(desc, *sc._qk, ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                         tok.data_ptr() if with_tok else None, ws.data_ptr(), need, stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], canary), "wrote behind the workspace"
    assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
    if not with_tok:
        assert (tok == 12345.0).all()
    s, t = scores[:S].cpu().numpy(), tok[:M].cpu().numpy()
    if finite:
        assert np.isfinite(s).all() and np.isfinite(t).all(), "non-finite output"
    del ws
    return s, [t[off[i]:off[i + 1]] for i in range(S)]


def _same(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _flat_and_tree(sc, seqs, mode=None):
    """Both calls; asserts tree == flat byte for byte in scores and log-probs, returns the flat results."""
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


_TINY = {}


def _tiny(name, **over):
    """(LlamaScorer, HF fp32 CPU model, GPU state dict, reference dims, inv_freq) of a tiny model, cached."""
    key = (name, tuple(sorted(over.items())))
    if key not in _TINY:
        model, cfg = tiny_model(name, **over)
        tied = TINY[name]["tie_word_embeddings"]
        st = state_of(model, tied)
        dims = R.llama_dims(cfg)
        sc = R.LlamaScorer(dims, R.llama_device_layout(st, dims, R.rope_inv_freq(cfg)), "cuda")
        _TINY[key] = (sc, model, {k: v.cuda() for k, v in st.items()}, ref_dims(cfg), hf_inv_freq(model))
    return _TINY[key]


_WIDE = {}


def _wide(width):
    """(LlamaScorer, GPU state dict, reference dims, inv_freq) of one random layer plus head at a full width, cached one at a
    time (the 8B width holds 2.5 GB of weights twice: HF's layout for the restatement, the device layout for the kernels)."""
    import torch
    if width not in _WIDE:
        _WIDE.clear()
        torch.cuda.empty_cache()
        d, Hq, Hkv, Fd, V, bias, tied, theta = WIDTHS[width]
        hd = d // Hq
        g = torch.Generator(device="cuda").manual_seed(d + V)
        rn = lambda *s, std: (torch.randn(*s, generator=g, device="cuda") * std).half()
        st = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "model.norm.weight": (1 + rn(d, std=0.2).float()).half()}
        if not tied:
            st["lm_head.weight"] = rn(V, d, std=2.0 / d ** 0.5)
        p = "model.layers.0."
        for n, (o, i) in {"self_attn.q_proj": (Hq * hd, d), "self_attn.k_proj": (Hkv * hd, d), "self_attn.v_proj": (Hkv * hd, d),
                          "self_attn.o_proj": (d, d), "mlp.gate_proj": (Fd, d), "mlp.up_proj": (Fd, d),
                          "mlp.down_proj": (d, Fd)}.items():
            st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
            if bias and n.split(".")[1] in ("q_proj", "k_proj", "v_proj"):
                st[p + n + ".bias"] = rn(o, std=0.3)
        for n in ("input_layernorm", "post_attention_layernorm"):
            st[p + n + ".weight"] = (1 + rn(d, std=0.2).float()).half()
        cfg = dict(model_type="qwen2" if bias else "llama", hidden_size=d, num_attention_heads=Hq, num_key_value_heads=Hkv,
                   intermediate_size=Fd, vocab_size=V, num_hidden_layers=1, max_position_embeddings=2048, rms_norm_eps=1e-5,
                   rope_theta=theta, tie_word_embeddings=tied)
        dims = R.llama_dims(cfg)
        inv = R.rope_inv_freq(cfg)
        sc = R.LlamaScorer(dims, R.llama_device_layout(st, dims, inv), "cuda")
        _WIDE[width] = (sc, st, ref_dims(cfg), inv)
    return _WIDE[width]


def _contract(tag, got, st, rd, inv, seqs):
    """Asserts got against the rounded restatement within min(3 x e16, 1e-2); prints the figures first."""
    ref = np.concatenate(_ref_logp_llama(st, rd, inv, seqs, rounded=True))
    exact = np.concatenate(_ref_logp_llama(st, rd, inv, seqs, rounded=False))
    g = np.concatenate(got)
    assert g.shape == ref.shape
    e16 = float(np.abs(ref - exact).max())
    err = float(np.abs(g - ref).max())
    print(f"CLM llama contract {tag}: tokens {len(g)} max |dlogp| {err:.3e}  e16 {e16:.3e}  ratio {err / e16:.3f}  "
          f"(max |logp| {np.abs(ref).max():.2f})")
    assert e16 > 0 and err <= min(3 * e16, 1e-2), (tag, err, e16)


def _prod_list(V, seed=0, cands=100, context=0):
    """tools/bench_llm_rescore.py's list: cands candidates of 10-40 tokens, BOS first, behind `context` shared tokens."""
    rng = np.random.default_rng(seed)
    ctx = list(rng.integers(4, V, context))
    return [[2] + ctx + list(rng.integers(4, V, int(n) - 1)) for n in rng.integers(10, 41, cands)]


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_against_the_contract(name):
    """Flat and tree (bit-identical) against the rounded float64 restatement.  The four models cover group sizes 2, 4, 1 and
    8, head dims 64 and 128 (the permuted q / k rows), biases, tied and untied heads, and llama3 frequency scaling."""
    sc, _, st, rd, inv = _tiny(name)
    V = rd["vocab"]
    seqs = tiny_seqs(V, seed=3, lens=(1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129))
    seqs += [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate
    _, got = _flat_and_tree(sc, seqs)
    _contract(f"tiny {name}", got, st, rd, inv, seqs)
    for mode in ("0", "2"):
        assert _same(_call(sc, seqs, False, mode)[1], got), mode


def test_rms_eps_is_the_models():
    """rms_norm_eps = 1e-2, large against the embedding rows' mean square (4 / d): dropping or changing it moves the first
    RMSNorm by tens of per cent.  Against the restatement and against HF."""
    sc, model, st, rd, inv = _tiny("llama", rms_norm_eps=1e-2)
    assert abs(sc.desc.rms_eps - 1e-2) < 1e-9
    seqs = tiny_seqs(rd["vocab"], seed=9, lens=(1, 17, 64, 65))
    _, got = _flat_and_tree(sc, seqs)
    _contract("tiny llama rms_eps 1e-2", got, st, rd, inv, seqs)
    g, h = np.concatenate(got), np.concatenate(hf_logp(model, seqs))
    assert np.all(np.abs(g - h) <= HF_ABS + HF_REL * np.abs(h))


def test_group_sizes_and_head_dims_covered():
    groups = {c["num_attention_heads"] // c["num_key_value_heads"] for c in TINY.values()}
    hds = {c["hidden_size"] // c["num_attention_heads"] for c in TINY.values()}
    assert groups == {1, 2, 4, 8} and hds == {64, 128}


@pytest.mark.parametrize("width", list(WIDTHS))
def test_full_width_layer_against_the_contract(width):
    """One full-width layer plus the head (128256 / 152064 columns): flat and tree, default tile rule and both forced."""
    sc, st, rd, inv = _wide(width)
    V = rd["vocab"]
    rng = np.random.default_rng(rd["d_model"])
    seqs = [[2] + list(rng.integers(0, V, n - 1)) for n in (1, 2, 17, 33, 300)]
    seqs += [seqs[4][:120] + list(rng.integers(0, V, 30)), seqs[4][:120] + list(rng.integers(0, V, 5))]
    _, got = _flat_and_tree(sc, seqs)
    _contract(width, got, st, rd, inv, seqs)
    for mode in ("0", "2"):
        assert _same(_call(sc, seqs, False, mode)[1], got), mode


# ---- against HF fp32 ----------------------------------------------------------------------------------------------------
# |dlogp| <= HF_ABS + HF_REL * |logp| per token, |dscore| <= SC_ABS + SC_REL * |score| per sequence: the bound form of
# test_gpu_llm_rescore.test_tiny_opt_matches_hf_fp32 (fp16 operands against an fp32 forward: the error of a log-prob grows
# with its logit's magnitude).  HF_REL and SC_ABS are that test's (2 x fp16's relative precision 2^-11 on the head's
# operands; 1e-2); the other two are 2 x what was measured on an MI355X over the four tiny models (NOTES.md "LLM"): the
# largest |dlogp| - HF_REL |logp| was 8.9e-4 (max |dlogp| 6.7e-3 at log-probs down to -15), the largest |dscore| 3.7e-2 on
# scores down to -866, so SC_REL = (2 x 3.7e-2 - 1e-2) / 854.
HF_ABS, HF_REL = 1.8e-3, 1e-3
SC_ABS, SC_REL = 1e-2, 7.5e-5


class _HfScorer:
    """The HF fp32 model behind OptScorer's `score`, for gpt2_lm_decode."""

    def __init__(self, model):
        self.model = model

    def score(self, ids_list, length_penalty=0.0):
        lp = hf_logp(self.model, [list(map(int, s)) for s in ids_list])
        return np.array([x.sum() - len(x) * length_penalty for x in lp])


@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_match_hf_fp32(name):
    sc, model, _, rd, _ = _tiny(name)
    V = rd["vocab"]
    seqs = tiny_seqs(V, seed=4)
    s, got = _flat_and_tree(sc, seqs)
    hf = hf_logp(model, seqs)
    g, h = np.concatenate(got), np.concatenate(hf)
    hs = np.array([x.sum() for x in hf])
    need_abs = float(np.max(np.abs(g - h) - HF_REL * np.abs(h)))
    print(f"CLM llama vs HF fp32 {name}: max |dlogp| {np.abs(g - h).max():.3e} (max |logp| {np.abs(h).max():.2f}), "
          f"max (|dlogp| - {HF_REL} |logp|) {need_abs:.3e}, max |dscore| {np.abs(s - hs).max():.3e} (max |score| {np.abs(hs).max():.1f})")
    assert np.all(np.abs(g - h) <= HF_ABS + HF_REL * np.abs(h))
    assert np.all(np.abs(s - hs) <= SC_ABS + SC_REL * np.abs(hs))
    # the picks of gpt2_lm_decode on the recorded lists: the HIP scorer and HF fp32 choose the same sentence
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tk = R.WordTokenizer(vocab_size=V, bos_id=2, pad_id=1)
    hfs = _HfScorer(model)
    seen = set()
    for c in gold["decode"]:
        kw = dict(length_penalty=c["length_penalty"], alpha=c["alpha"], returnConfidence=c["confidence"],
                  current_context_str=c["context"])
        for tree in (False, True):
            sc.share_prefixes = tree
            ours = R.gpt2_lm_decode(sc, tk, "cuda", c["nbest"], 0.35, **kw)
            theirs = R.gpt2_lm_decode(hfs, tk, "cpu", c["nbest"], 0.35, **kw)
            assert ours[0] == theirs[0], (name, c["case"], c["context"], tree)
        seen.add(bool(c["context"] and c["context"].split()))
    sc.share_prefixes = False
    assert seen == {True, False}   # with and without a context string


# ---- bit identity ---------------------------------------------------------------------------------------------------------
def _golden_lists(V):
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(vocab_size=V, bos_id=2, pad_id=1)
    out = []
    for c in gold["decode"]:
        ctx = c["context"] if c["context"] is not None and c["context"].split() else None
        hyps = [e[0].strip() for e in c["nbest"] if e[0].strip()]
        out.append(tok([ctx + " " + h if ctx else h for h in hyps])["input_ids"])
    return out


@pytest.mark.parametrize("name", list(TINY))
def test_tree_equals_flat_on_recorded_lists(name):
    sc, _, _, rd, _ = _tiny(name)
    for seqs in _golden_lists(rd["vocab"]):
        _flat_and_tree(sc, seqs)


@pytest.mark.parametrize("width", list(WIDTHS))
def test_tree_equals_flat_at_full_width_on_every_tile_path(width):
    """100 candidates behind a 100-token context: ~12500 tokens flat, ~2600 nodes; B2T_CLM_GEMM_256 = 0, unset and 2 give the
    same bits on both paths."""
    sc, _, rd, _ = _wide(width)
    seqs = _prod_list(rd["vocab"], seed=1, cands=100, context=100)
    base = None
    for mode in ("0", None, "2"):
        s, t = _flat_and_tree(sc, seqs, mode)
        if base is None:
            base = (s, t)
        assert s.tobytes() == base[0].tobytes() and _same(t, base[1]), mode


@pytest.mark.parametrize("name", ["llama", "qwen2"])
def test_tree_equals_flat_on_constructed_lists(name):
    sc, _, _, rd, _ = _tiny(name)
    V = rd["vocab"]
    rng = np.random.default_rng(5)
    r = lambda n: list(rng.integers(4, V, n))
    # the first owned position of the later candidates at the 32-row block edges
    for own in (31, 32, 33, 63, 64, 65):
        ctx = [2] + r(own - 1)
        seqs = [ctx + r(int(n)) for n in rng.integers(1, 40, 12)]
        assert all(s[:own] == ctx for s in seqs)
        _flat_and_tree(sc, seqs)
    a, b = [2] + r(20), [2] + r(7)
    _flat_and_tree(sc, [a, b, a, a, b])                                         # duplicates
    _flat_and_tree(sc, [[2] + r(5), [3] + r(5), [2, 5, 7], [3, 5]])             # a forest
    _flat_and_tree(sc, [[10 * i + j for j in range(1, 6)] for i in range(1, 9)])   # no sharing
    _flat_and_tree(sc, [[2] + r(40)])                                           # a lone sequence
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])                               # one-token sequences
    s, t = _call(sc, [[2], [5, 6]], False)
    assert s[0] == 0.0 and t[0].tolist() == [0.0]


@pytest.mark.parametrize("which", ["llama", "mistral", "llama3.2-1b"])
def test_score_alone_equals_score_in_a_batch(which):
    if which in TINY:
        sc, _, _, rd, _ = _tiny(which)
    else:
        sc, _, rd, _ = _wide(which)
    V = rd["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=99)
    s0, t0 = _call(sc, [probe], False)
    for pos in (0, 50, 99):
        batch = others[:pos] + [probe] + others[pos:]
        for tree in (False, True):
            s, t = _call(sc, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(sc, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()
    assert _call(sc, [probe], False, fill=0)[0].tobytes() == s0.tobytes()


# ---- rotary and grouped-query edges -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llama3", "mistral"])
def test_sequence_of_exactly_max_pos(name):
    """A 2048-token sequence at max_pos = 2048 (the rotary table's last row; llama3 scaling at positions far beyond its
    original 64; head dim 128 on the mistral model), beside short ones, against the restatement."""
    over = dict(max_position_embeddings=2048)
    if name == "mistral":
        over["sliding_window"] = None
    sc, _, st, rd, inv = _tiny(name, **over)
    assert sc.desc.max_pos == 2048
    seqs = tiny_seqs(rd["vocab"], seed=6, lens=(2048, 5, 33))
    _, got = _flat_and_tree(sc, seqs)
    _contract(f"max_pos 2048 {name}", got, st, rd, inv, seqs)
    with pytest.raises(RuntimeError, match="max_pos"):
        sc.score([[2] * 2049])
    with pytest.raises(RuntimeError, match="outside"):
        sc.score([[2, 5, rd["vocab"]]], share_prefixes=True)
    assert sc.score([[2, 5, 7]]).shape == (1,)   # the device is still usable


def test_scorer_surface_on_the_gpu():
    sc, _, _, rd, _ = _tiny("qwen2")
    seqs = tiny_seqs(rd["vocab"], seed=8, lens=(1, 9, 40))
    s, t = _call(sc, seqs, False)
    for tree in (False, True):
        got = sc.token_logprobs(seqs, share_prefixes=tree)
        assert _same(got, t)
        assert sc.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}   # the three sequences share their first token
        assert sc.score(seqs, 0.25, share_prefixes=tree).tobytes() == (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    sc.score([seqs[2], seqs[2][:30] + [5]], share_prefixes=True)
    assert sc.last_stats == {"tokens": 71, "nodes": 41}


# ---- the service ------------------------------------------------------------------------------------------------------------
def test_service_end_to_end_with_a_llama_scorer():
    import evaluate_model_helpers as H
    import lm_decoder, ngram_lm
    from remote_lm import LocalLMService
    sc, _, _, rd, _ = _tiny("llama")
    Cc = 41
    prons = ngram_lm.synthetic_lexicon(200, Cc, seed=5)
    lex = ngram_lm.Lexicon(prons, Cc)
    wlm = ngram_lm.SparseNGramLM.from_arpa(ngram_lm.synthetic_word_arpa(lex.words, 2, 400, seed=2), lex.words)
    res = lm_decoder.DecodeResource("", "", "", "", "")
    res.set_lexicon_lm(lex, wlm, sil=1)
    opts = lm_decoder.DecodeOptions(7000, 200, 17.0, 8.0, 0.35, 0.95, 0.0, 10)
    opts.lm_alpha, opts.lm_beta = 0.8, 0.0
    dec = lm_decoder.BrainSpeechDecoder(res, opts, max_len=128)
    tok = R.WordTokenizer(vocab_size=rd["vocab"], bos_id=2, pad_id=1)
    r = LocalLMService(dec, acoustic_scale=0.35, blank_penalty=9.0, nbest=10, llm=(sc, tok), do_opt=1, alpha=0.5,
                       top_candidates_to_augment=5)
    rs = np.random.RandomState(0)
    words = [lex.words[i] for i in rs.randint(0, 200, size=4)]
    frames = []
    for w in words:
        for c in list(prons[w][0]) + [1]:
            frames += [c, 0]
    lg = np.full((len(frames), Cc), -1.0, dtype=np.float32)
    for t, c in enumerate(frames):
        lg[t, c] = 2.0
    seen = H.get_current_redis_time_ms(r)
    H.reset_remote_language_model(r, seen)
    H.send_logits_to_remote_lm(r, 'remote_lm_input', 'remote_lm_output_partial', seen, lg)
    _, out = H.finalize_remote_lm(r, 'remote_lm_output_final', seen)
    nb = [[d.sentence, d.ac_score, d.lm_score] for d in dec.result()[:10]]
    nb = R.augment_nbest(nb, top_candidates_to_augment=5, acoustic_scale=0.35)
    best, lines = R.gpt2_lm_decode(sc, tok, "cuda", nb, 0.35, length_penalty=0.0, alpha=0.5, current_context_str="")
    llm = out['candidate_llm_scores']
    assert 1 <= len(llm) <= len(nb) and all(v != 0.0 for v in llm)
    assert r.streams['remote_lm_output_final'][-1][1][b'lm_response_final'].decode() == best
