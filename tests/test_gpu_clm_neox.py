"""b2t_clm_neox_score_f16 / _tree_f16 / _tree_cached_f16 (csrc/causal_lm_neox.hip) on the MI355X, driven through the C ABI:
against the float64 restatement of the contract (ref_logp_neox of tests/test_clm_neox_host.py, on the GPU here), the bit
identities (tree = flat = cached, read-only and updating, both B2T_CLM_TRUNK_ATTN settings, the forced tile modes, alone = in
a batch), block edges, a growing context, a sequence of exactly max_pos, saturated pre-activations, the full widths of
Pythia-160M and Pythia-6.9B, build_scorer and the service.

Conventions as in the sibling files: every call (_call, Rig of tests/test_gpu_clm_cache.py) gets a fresh workspace of exactly
the size the library asks for, filled with 0xFF, with canaries behind it, behind both outputs and around the cache.

The bound is the project's: max |dlogp| <= min(3 x e16, 1e-2) against the fp16-rounded restatement, e16 = max |rounded -
unrounded restatement| of the case (restatement against restatement, never the kernels), after 0 < e16 <= 1e-2 / 3.  On the
ordinary tiny models that bound does not tell the erf GELU from the tanh form; on `sep` it does
(tests/test_clm_neox_host.py, test_the_bound_separates_erf_from_tanh_on_sep).  The measured ratios are in NOTES.md ("LLM")."""
import contextlib
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import dict_rule  # noqa: F401  (Rig uses it)
from test_clm_llama_host import tiny_seqs
from test_clm_neox_host import (BOUND_CAP, CONTRACT_SEED, TINY, contract_seqs, gelu_erf, gelu_tanh, neox_state, ref_logp_neox,
                                tiny_neox, tiny_state)
from test_gpu_clm_cache import SETTINGS, Rig, _same_bytes
from test_gpu_clm_llama import GOLD, _pack, _prod_list, _same, _tiles
from test_gpu_clm_tree import _ListDecoder

pytestmark = pytest.mark.gpu
MODELS = list(TINY) + ["sep"]


def _call(sc, seqs, tree=False, mode=None, with_tok=True):
    """(scores, per-sequence token log-probs) of one flat or tree GPT-NeoX C ABI call."""
    import torch
    import b2t_native as N
    lib = N.load()
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    if tree:
        nodes = R.tree_plan(ids, off)[2]
        need = lib.b2t_clm_neox_tree_ws_bytes(C.byref(sc.desc), nodes, M, S)
    else:
        need = lib.b2t_clm_neox_ws_bytes(C.byref(sc.desc), M, S)
    assert need > 0
    canary = torch.randint(0, 256, (CAN,), dtype=torch.uint8, device="cuda")
    ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
    ws[:need] = 0xFF
    ws[need:] = canary
    scores = torch.full((S + 64,), 12345.0, device="cuda")
    tok = torch.full((M + 64,), 12345.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    with _tiles(mode):
        if tree:
            nn = C.c_longlong(-1)
            rc = lib.b2t_clm_neox_score_tree_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                                 tok.data_ptr() if with_tok else None, C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == nodes
        else:
            rc = lib.b2t_clm_neox_score_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                            tok.data_ptr() if with_tok else None, ws.data_ptr(), need, stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], canary), "wrote behind the workspace"
    assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
    if not with_tok:
        assert (tok == 12345.0).all()
    s, t = scores[:S].cpu().numpy(), tok[:M].cpu().numpy()
    assert np.isfinite(s).all() and np.isfinite(t).all(), "non-finite output"
    del ws
    return s, [t[off[i]:off[i + 1]] for i in range(S)]


def _flat_and_tree(sc, seqs, mode=None):
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


class _NeoxLib:
    """The library as Rig (tests/test_gpu_clm_cache.py) drives it, with the three calls that take the model routed to this
    family's; the plan, the rule and the cache are the same."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def b2t_clm_cache_kv_bytes(self, *args):
        return self._lib.b2t_clm_neox_cache_kv_bytes(*args)

    def b2t_clm_tree_cached_ws_bytes(self, *args):
        return self._lib.b2t_clm_neox_tree_cached_ws_bytes(*args)

    def b2t_clm_score_tree_cached_f16(self, *args):
        return self._lib.b2t_clm_neox_score_tree_cached_f16(*args)


@contextlib.contextmanager
def _neox_lib():
    """Rig takes its library from b2t_native.load(): inside, that is the routed one."""
    import b2t_native as N
    real = N.load()
    N._lib = _NeoxLib(real)
    try:
        yield
    finally:
        N._lib = real


def _rigs(sc, cap):
    with _neox_lib():
        rigs = [Rig(sc, cap, s) for s in SETTINGS]
    assert all(isinstance(rig.lib, _NeoxLib) for rig in rigs)
    return rigs


def _check(rigs, sc, seqs, mode=None, update=1, what="", flat=True):
    """The cached call of every rig == the tree call (== the flat call); returns the plans (one per rig)."""
    tree = _call(sc, seqs, True, mode)
    if flat:
        _same_bytes(_call(sc, seqs, False, mode), tree, f"{what}: flat against tree")
    plans = []
    for rig in rigs:
        s, t, plan = rig.call(seqs, mode, update)
        _same_bytes((s, t), tree, f"{what}: cached (update {update}, trunk attention {rig.setting}) against tree")
        plans.append(plan)
    return plans


def _scorer(st, cfg):
    dims = R.neox_dims(cfg)
    return R.NeoxScorer(dims, R.neox_device_layout(st, dims, R.neox_inv_freq(cfg)), "cuda")


_TINY = {}


def _tiny(name):
    """(NeoxScorer, GPU state dict, dims) of a tiny model or `sep`, cached."""
    if name not in _TINY:
        st, cfg = tiny_state(name)
        sc = _scorer(st, cfg)
        _TINY[name] = (sc, {k: v.cuda() for k, v in st.items()}, dict(sc.dims))
    return _TINY[name]


def _against_contract(tag, got, st, dims, seqs):
    """Prints e16, the error and their ratio, then asserts 0 < e16 <= 1e-2 / 3 and max |dlogp| <= min(3 e16, 1e-2)."""
    ref = np.concatenate(ref_logp_neox(st, dims, seqs, True))
    exact = np.concatenate(ref_logp_neox(st, dims, seqs, False))
    g = np.concatenate(got)
    assert g.shape == ref.shape and np.isfinite(g).all()
    e16, err = float(np.abs(ref - exact).max()), float(np.abs(g - ref).max())
    print(f"CLM neox contract {tag}: tokens {len(g)} max |dlogp| {err:.3e}  e16 {e16:.3e}  ratio {err / e16:.3f}  "
          f"bound {min(3 * e16, BOUND_CAP):.3e}  (min logp {ref.min():.2f})")
    assert 0 < e16 <= BOUND_CAP / 3, (tag, e16)
    assert err <= min(3 * e16, BOUND_CAP), (tag, err, e16)
    return err, e16


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_tiny_models_against_the_contract(name):
    """Flat == tree byte for byte, and within min(3 e16, 1e-2) of the rounded float64 restatement, on lengths 1 .. 128 (=
    max_pos) plus two candidates sharing a prefix and a duplicate; B2T_CLM_GEMM_256 = 0 and 2 give the default's bytes on both
    paths.  `sep` is the model on which that bound tells the erf GELU from the tanh form.

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, st, dims = _tiny(name)
    seqs = contract_seqs(dims["vocab"], CONTRACT_SEED)
    assert max(map(len, seqs)) == dims["max_pos"] == 128
    fs, got = _flat_and_tree(sc, seqs)
    _against_contract(name, got, st, dims, seqs)
    for mode in ("0", "2"):
        for tree in (False, True):
            s, t = _call(sc, seqs, tree, mode)
            assert s.tobytes() == fs.tobytes() and _same(t, got), (mode, tree)


@pytest.mark.parametrize("name", MODELS)
def test_cached_equals_tree(name):
    """A shared context primed by one call, then a list behind it: the cached call, read-only and updating, with
    B2T_CLM_TRUNK_ATTN 0 and 1, on every tile mode, gives the tree call's bytes (which are the flat call's)."""
    sc, _, dims = _tiny(name)
    rng = np.random.default_rng(dims["vocab"])
    ctx = [2] + [int(x) for x in rng.integers(4, dims["vocab"], 40)]
    lst = [ctx + [int(x) for x in rng.integers(4, dims["vocab"], int(n))] for n in (5, 12, 1, 30, 12)]
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [ctx], what=f"{name} prime", flat=False)
    for mode in (None, "0", "2"):
        for update in (0, 1):
            for plan in _check(rigs, sc, lst, mode, update, what=f"{name} mode {mode}", flat=mode is None and update == 0):
                assert plan["reused"] == 40


@pytest.mark.parametrize("act", ["gelu", "gelu_fast"])
def test_saturated_pre_activations(act):
    """dense_h_to_4h's bias at +-60 (alternating): every pre-activation is beyond +-40, where erf is +-1 exactly and the tanh
    form's exp overflows to inf or underflows to 0.  Every output is finite (_call asserts it), and the three paths agree byte
    for byte.  (No contract bound here: activations of 60 have an fp16 spacing of 0.03, so e16 is far beyond 1e-2 / 3.)"""
    import torch
    model, cfg = tiny_neox("hd64_q", hidden_act=act)
    st = neox_state(model)
    for l in range(2):
        k = f"gpt_neox.layers.{l}.mlp.dense_h_to_4h.bias"
        st[k] = 60.0 * (1 - 2 * (torch.arange(st[k].numel()) % 2)).float()
    sc = _scorer(st, cfg)
    dims = dict(sc.dims)
    assert dims["act"] == (0 if act == "gelu" else 1)
    seqs = contract_seqs(dims["vocab"], CONTRACT_SEED)
    seen = []

    def spy(v):
        seen.append((float(v.abs().min()), float(v.min()), float(v.max())))
        return (gelu_erf if act == "gelu" else gelu_tanh)(v)
    ref = ref_logp_neox({k: v.cuda() for k, v in st.items()}, dims, seqs[:6], True, spy)
    assert len(seen) == 2 and all(lo > 40 and mn < -40 and mx > 40 for lo, mn, mx in seen), seen
    # the kernels' own forms at those magnitudes, in fp32: no NaN, the sign kept
    v = torch.tensor([-100.0, -60.0, -40.0, 40.0, 60.0, 100.0])
    want = torch.tensor([-0.0, -0.0, -0.0, 40.0, 60.0, 100.0])
    assert torch.equal(0.5 * v * (1 + torch.erf(v * 0.7071067811865476)), want)
    fs, got = _flat_and_tree(sc, seqs)
    err = float(np.abs(np.concatenate(got[:6]) - np.concatenate(ref)).max())
    print(f"CLM neox saturation {act}: fc1 pre-activations (min |v|, min, max) {seen}; max |dlogp| to the restatement {err:.3e}")
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [seqs[5][:20]], what="saturated prime", flat=False)
    for plan in _check(rigs, sc, seqs[-3:-1], what="saturated cached"):
        assert plan["reused"] == 19


# ---- full widths ------------------------------------------------------------------------------------------------------------
# (d, heads, F, vocab, untied): one layer of these widths plus the head
WIDTHS = {"pythia-160m": (768, 12, 3072, 50304, False), "pythia-6.9b": (4096, 32, 16384, 50432, True)}


def _wide_state(d, H, F, V, untied, seed):
    """One GPT-NeoX layer of that width plus the head, in the tiny models' weight recipe (fp16 GPU tensors)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *shape, std: (torch.randn(*shape, generator=g, device="cuda") * std).half()
    st = {"gpt_neox.embed_in.weight": rn(V, d, std=2.0 / d ** 0.5)}
    if untied:
        st["embed_out.weight"] = rn(V, d, std=2.0 / d ** 0.5)
    p = "gpt_neox.layers.0."
    for ln in (p + "input_layernorm", p + "post_attention_layernorm", "gpt_neox.final_layer_norm"):
        st[ln + ".weight"], st[ln + ".bias"] = (1 + rn(d, std=0.2).float()).half(), rn(d, std=0.3)
    for name, n_in, n_out in (("attention.query_key_value", d, 3 * d), ("attention.dense", d, d), ("mlp.dense_h_to_4h", d, F),
                              ("mlp.dense_4h_to_h", F, d)):
        st[p + name + ".weight"] = rn(n_out, n_in, std=1.0 / n_in ** 0.5)
        st[p + name + ".bias"] = rn(n_out, std=0.3)
    return st


@pytest.mark.parametrize("width", list(WIDTHS))
def test_full_width_layer_and_head(width):
    """One layer plus the head at the widths of Pythia-160M (768 / 12, head dim 64, tied here) and Pythia-6.9B (4096 / 32, head
    dim 128, untied), 16 resp. 32 rotary dims, on sequences of 1, 2, 17, 33 and 300 tokens plus two that share 120: tree ==
    flat byte for byte, within the bound of the restatement."""
    import torch
    d, H, F, V, untied = WIDTHS[width]
    st = _wide_state(d, H, F, V, untied, seed=d)
    cfg = dict(model_type="gpt_neox", hidden_size=d, num_attention_heads=H, num_hidden_layers=1, intermediate_size=F,
               vocab_size=V, max_position_embeddings=512, rotary_pct=0.25, rotary_emb_base=10000, hidden_act="gelu",
               layer_norm_eps=1e-5, use_parallel_residual=True, tie_word_embeddings=not untied)
    sc = _scorer(st, cfg)
    dims = dict(sc.dims)
    assert dims["rotary_ndims"] == d // H // 4 and (sc.desc.embed_out != sc.desc.embed_in) == untied
    rng = np.random.default_rng(d)
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    seqs = tiny_seqs(V, seed=5, lens=(1, 2, 17, 33, 300))
    shared = [2] + r(119)
    seqs += [shared + r(10), shared + r(15) + [V - 1]]
    fs, got = _flat_and_tree(sc, seqs)
    _against_contract(width, got, st, dims, seqs)
    del sc, st
    torch.cuda.empty_cache()


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hd64_q", "hd64_f", "hd128_q", "hd128_f"])
def test_block_edges_on_the_tree_and_cache_paths(name):
    """The first owned position of the later candidates, and the cache's R, at 31, 32, 33, 63, 64, 65 (read-only, then
    updating)."""
    sc, _, dims = _tiny(name)
    V = dims["vocab"]
    rng = np.random.default_rng(dims["d_model"])
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    chain = [2] + r(127)
    for Rr in (31, 32, 33, 63, 64, 65):
        _flat_and_tree(sc, [chain[:Rr] + r(int(n)) for n in rng.integers(1, 40, 8)])      # first owned position Rr
        rigs = _rigs(sc, 128)
        for plan in _check(rigs, sc, [chain[:Rr + 1]], what=f"{name} prime {Rr}", flat=False):
            assert plan["n_after"] == Rr + 1
        far = [chain[:Rr + 30] + r(n) for n in (20, 30, 1)] + [chain[:Rr + 30]]
        for plan in _check(rigs, sc, far, update=0, what=f"{name} R {Rr}"):
            assert plan["reused"] == Rr
        _check(rigs, sc, far, what=f"{name} R {Rr}, updating", flat=False)
        for plan in _check(rigs, sc, far, what=f"{name} R {Rr} again", flat=False):
            assert plan["reused"] == Rr + 29


@pytest.mark.parametrize("name", ["hd64_h", "hd128_q", "hd128_h"])
def test_a_growing_context_over_three_cached_calls(name):
    """A conversation: the context grows by the chosen candidate after every call; each call reuses what the one before left,
    and every call gives the tree call's bytes."""
    sc, _, dims = _tiny(name)
    V = dims["vocab"]
    rng = np.random.default_rng(11)
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    rigs = _rigs(sc, 128)
    ctx, want = [2] + r(20), 0
    for call in range(3):
        lst = [ctx + r(n) for n in (9, 14, 5, 14)]
        for plan in _check(rigs, sc, lst, what=f"{name} call {call}", flat=call == 0):
            assert plan["reused"] == want and plan["n_after"] == len(ctx), (call, plan)
        want = len(ctx) - 1
        ctx = lst[1]
    assert all(rig.n == len(lst[0]) - 9 for rig in rigs)


@pytest.mark.parametrize("name", ["hd64_q", "hd128_q"])
def test_sequence_of_exactly_max_pos_and_one_more(name):
    """A path of exactly max_pos = 128 tokens on all three paths (R = 126); one token more is refused under the entry point's
    own name before any launch."""
    import b2t_native as N
    sc, _, dims = _tiny(name)
    V = dims["vocab"]
    rng = np.random.default_rng(3)
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    chain = [2] + r(127)
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [chain[:127]], what="prime 127", flat=False)
    seqs = [chain, chain[:127] + r(1), chain[:127]]
    assert max(map(len, seqs)) == 128 == dims["max_pos"]
    for plan in _check(rigs, sc, seqs, what=f"{name} max_pos"):
        assert plan["reused"] == 126 and plan["rows"] == 3
    lib = N.load()
    ids, off = _pack([chain + [5]])
    for who, tail in (("b2t_clm_neox_score_f16", ()), ("b2t_clm_neox_score_tree_f16", (None,))):
        rc = getattr(lib, who)(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, 1, 0x10000, None, *tail, 0x10000, 1 << 30, None)
        assert rc != 0 and N.last_error().startswith(who + ":") and "max_pos" in N.last_error(), N.last_error()
    n0 = rigs[0].n
    rc = lib.b2t_clm_neox_score_tree_cached_f16(C.byref(sc.desc), C.byref(rigs[0].c), 1, ids.ctypes.data, off.ctypes.data, 1, 0x10000,
                                                None, None, None, 0x10000, 1 << 30, None)
    assert rc != 0 and N.last_error().startswith("b2t_clm_neox_score_tree_cached_f16:") and "max_pos" in N.last_error()
    assert rigs[0].n == n0


@pytest.mark.parametrize("name", ["hd64_q", "hd64_f", "hd128_q", "hd128_f"])
def test_score_alone_equals_score_in_a_batch(name):
    sc, _, dims = _tiny(name)
    V = dims["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=99)
    s0, t0 = _call(sc, [probe], False)
    for pos in (0, 50, 99):
        batch = others[:pos] + [probe] + others[pos:]
        for tree in (False, True):
            s, t = _call(sc, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(sc, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()


# ---- build_scorer and the service ---------------------------------------------------------------------------------------------
def test_service_end_to_end_with_a_neox_scorer(tmp_path):
    """build_scorer on a saved GPT-NeoX directory gives a NeoxScorer; LocalLMService with do_opt = 1 over three sentences with a
    growing context: with a context cache the replies are, field by field, those of a scorer without, and from the second
    sentence on the context is reused.  Then the scorer's surface against the ABI's bytes."""
    import evaluate_model_helpers as H
    from remote_lm import LocalLMService
    model, cfg = tiny_neox("hd64_q")
    model.save_pretrained(str(tmp_path))
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(vocab_size=cfg["vocab_size"], bos_id=2, pad_id=1)
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies, reused = {}, {}
    for cache_tokens in (0, 128):
        sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto", context_cache_tokens=cache_tokens)
        assert type(sc) is R.NeoxScorer
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
    print(f"CLM neox service: reused per sentence {reused[128]}")
    assert reused[0] == [None, None, None]
    assert reused[128][0] == 0 and 0 < reused[128][1] < reused[128][2], reused
    # the scorer's surface: the ABI's bytes, last_stats, the length penalty, and HF's numbers to fp16 precision
    from test_clm_llama_host import hf_logp
    sc = R.build_scorer(str(tmp_path), device="cuda")
    seqs = tiny_seqs(cfg["vocab_size"], seed=8, lens=(1, 9, 40))
    s, t = _call(sc, seqs, False)
    for tree in (False, True):
        assert _same(sc.token_logprobs(seqs, share_prefixes=tree), t)
        assert sc.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
        assert sc.score(seqs, 0.25, share_prefixes=tree).tobytes() == (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    assert np.abs(np.concatenate(t) - np.concatenate(hf_logp(model, seqs))).max() <= BOUND_CAP
    with pytest.raises(RuntimeError, match="b2t_clm_neox_score_f16.*max_pos"):
        sc.score([[2] * 129])
    with pytest.raises(RuntimeError, match="b2t_clm_neox_score_tree_f16.*outside"):
        sc.score([[2, 5, cfg["vocab_size"]]], share_prefixes=True)
