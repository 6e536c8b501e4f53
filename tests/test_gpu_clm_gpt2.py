"""b2t_clm_gpt2_score_f16 / _tree_f16 / _tree_cached_f16 (csrc/causal_lm_gpt2.hip) on the MI355X, driven through the C ABI:
against the float64 restatement of the contract (ref_logp_gpt2 of tests/test_clm_gpt2_host.py, on the GPU here), the bit
identities of the OPT paths (tree = flat = cached, read-only and updating, both B2T_CLM_TRUNK_ATTN settings, the forced tile
modes, alone = in a batch), saturated pre-activations, the full widths of GPT-2 XL and GPT-2 small, the edges of the tree and
cache paths, the picks of gpt2_lm_decode against HF fp32 and the service.

Conventions as in the sibling files: every call (_call, Rig) gets a fresh workspace of exactly the size the library asks for
(the OPT size functions'), filled with 0xFF, with canaries behind it, behind both outputs and around the cache.

The bound is the project's: max |dlogp| <= min(3 x e16, 1e-2) against the fp16-rounded restatement, e16 = max |rounded -
unrounded restatement| of the case (restatement against restatement, never the kernels), after 0 < e16 <= 1e-2 / 3.  Planted in
the rounded restatement the bound separates ReLU for GELU (log-probs move by 0.87 - 1.00), the cubic term dropped (0.079 -
0.110) and x * sigmoid(1.702 x) (0.044 - 0.050).  It does NOT separate the erf GELU from the tanh form: that difference is
2.8e-3 - 3.1e-3 here, the size of the fp16 rounding of the activations themselves (e16 2.5e-3 - 2.9e-3); the loader refuses
"gelu" by name instead.
The measured ratios and the planted bugs this file was checked against are in NOTES.md ("LLM")."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import dict_rule  # noqa: F401  (Rig uses it)
from test_clm_gpt2_host import TINY, gelu_new, gpt2_state, ref_logp_gpt2, tiny_gpt2
from test_clm_llama_host import hf_logp, tiny_seqs
from test_gpu_clm_cache import SETTINGS, Rig, _same_bytes
from test_gpu_clm_llama import GOLD, _HfScorer, _pack, _prod_list, _same, _tiles
from test_gpu_clm_tree import _ListDecoder

pytestmark = pytest.mark.gpu
LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128)   # 563 rows: crosses the 128- and 256-row tile boundaries; 128 = n_positions
# the sequences' seed: the first of 3, 4, ... at which e16 of all three models meets the bound's precondition e16 <= 1e-2 / 3
# (seed 3 gives 3.5e-3 on the d 320 model: one token's rounding, a property of the restatement alone)
CONTRACT_SEED = 4
BOUND_CAP = 1e-2


def _call(sc, seqs, tree=False, mode=None, with_tok=True):
    """(scores, per-sequence token log-probs) of one flat or tree GPT-2 C ABI call."""
    import torch
    import b2t_native as N
    lib = N.load()
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    if tree:
        nodes = R.tree_plan(ids, off)[2]
        need = lib.b2t_clm_tree_ws_bytes(C.byref(sc.desc), nodes, M, S)
    else:
        need = lib.b2t_clm_ws_bytes(C.byref(sc.desc), M, S)
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
            rc = lib.b2t_clm_gpt2_score_tree_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                                 tok.data_ptr() if with_tok else None, C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == nodes
        else:
            rc = lib.b2t_clm_gpt2_score_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
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


class _Gpt2Lib:
    """The library as Rig (tests/test_gpu_clm_cache.py) drives it, its cached call routed to GPT-2's; the size functions and
    the cache are the OPT family's either way."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def b2t_clm_score_tree_cached_f16(self, *args):
        return self._lib.b2t_clm_gpt2_score_tree_cached_f16(*args)


def _rigs(sc, cap):
    rigs = [Rig(sc, cap, s) for s in SETTINGS]
    for rig in rigs:
        rig.lib = _Gpt2Lib(rig.lib)
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
    dims = R.gpt2_dims(cfg)
    return R.Gpt2Scorer(dims, R.gpt2_device_layout(st, dims), "cuda")


_TINY = {}


def _tiny(name):
    """(Gpt2Scorer, HF fp32 CPU model, GPU state dict, dims) of a tiny model, cached."""
    if name not in _TINY:
        model, cfg = tiny_gpt2(name)
        st = gpt2_state(model)
        sc = _scorer(st, cfg)
        _TINY[name] = (sc, model, {k: v.cuda() for k, v in st.items()}, dict(sc.dims))
    return _TINY[name]


def _contract_seqs(V):
    seqs = tiny_seqs(V, seed=CONTRACT_SEED, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate


def _against_contract(tag, got, st, dims, seqs, act=gelu_new):
    """Prints e16, the error and their ratio, then asserts 0 < e16 <= 1e-2 / 3 and max |dlogp| <= min(3 e16, 1e-2)."""
    ref = np.concatenate(ref_logp_gpt2(st, dims, seqs, True, act))
    exact = np.concatenate(ref_logp_gpt2(st, dims, seqs, False, act))
    g = np.concatenate(got)
    assert g.shape == ref.shape and np.isfinite(g).all()
    e16, err = float(np.abs(ref - exact).max()), float(np.abs(g - ref).max())
    print(f"CLM gpt2 contract {tag}: tokens {len(g)} max |dlogp| {err:.3e}  e16 {e16:.3e}  ratio {err / e16:.3f}  "
          f"bound {min(3 * e16, BOUND_CAP):.3e}  (min logp {ref.min():.2f})")
    assert 0 < e16 <= BOUND_CAP / 3, (tag, e16)
    assert err <= min(3 * e16, BOUND_CAP), (tag, err, e16)
    return err, e16


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_against_the_contract(name):
    """Flat == tree == cached (read-only and updating, B2T_CLM_TRUNK_ATTN 0 and 1) byte for byte; B2T_CLM_GEMM_256 = 0 and 2
    give the default's bytes on all three paths; within min(3 e16, 1e-2) of the rounded float64 restatement.  The bound does
    not separate the erf GELU from the tanh form (2.8e-3 - 3.1e-3 in the restatement, the size of e16 itself); it separates
    ReLU (0.87 - 1.00), a dropped cubic term (0.079 - 0.110) and x sigmoid(1.702 x) (0.044 - 0.050).

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, _, st, dims = _tiny(name)
    seqs = _contract_seqs(dims["vocab"])
    assert max(map(len, seqs)) == dims["max_pos"] == 128
    fs, got = _flat_and_tree(sc, seqs)
    _against_contract(name, got, st, dims, seqs)
    for mode in ("0", "2"):
        for tree in (False, True):
            s, t = _call(sc, seqs, tree, mode)
            assert s.tobytes() == fs.tobytes() and _same(t, got), (mode, tree)
    # the cached call: a shared context primed by one call, then a list behind it, on every tile mode
    rng = np.random.default_rng(dims["vocab"])
    ctx = [2] + [int(x) for x in rng.integers(4, dims["vocab"], 40)]
    lst = [ctx + [int(x) for x in rng.integers(4, dims["vocab"], int(n))] for n in (5, 12, 1, 30, 12)]
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [ctx], what=f"{name} prime", flat=False)
    for mode in (None, "0", "2"):
        for update in (0, 1):
            for plan in _check(rigs, sc, lst, mode, update, what=f"{name} mode {mode}"):
                assert plan["reused"] == 40


def test_saturated_pre_activations():
    """The d 128 model with c_fc.bias scaled by 40: pre-activations beyond +-20 on both sides, where exp(2u) overflows to inf
    and underflows to 0.  Every output finite (gelu_new -> v on the positive side, -0.0 / 0 on the negative side), the paths
    bit-identical, and within the same bound of the restatement."""
    import torch
    model, cfg = tiny_gpt2("hd64")
    st = gpt2_state(model)
    for l in range(2):
        k = f"transformer.h.{l}.mlp.c_fc.bias"
        st[k] = (st[k] * 40).half().float()
    sc = _scorer(st, cfg)
    g = {k: v.cuda() for k, v in st.items()}
    dims = dict(sc.dims)
    seqs = _contract_seqs(dims["vocab"])
    seen = []

    def spy(v):
        seen.append((float(v.min()), float(v.max())))
        return gelu_new(v)
    ref_logp_gpt2(g, dims, seqs[:4], True, spy)
    assert all(lo < -20 and hi > 20 for lo, hi in seen) and len(seen) == 2, seen
    # the kernel's own form at those magnitudes, in fp32: no NaN, the sign kept
    v = torch.tensor([-100.0, -60.0, -20.0, 20.0, 60.0, 100.0])
    th = 1 - 2 / (torch.exp(2 * 0.7978845608028654 * (v + 0.044715 * v ** 3)) + 1)
    assert torch.equal(0.5 * v * (1 + th), torch.tensor([-0.0, -0.0, -0.0, 20.0, 60.0, 100.0]))
    fs, got = _flat_and_tree(sc, seqs)
    print(f"CLM gpt2 saturation: fc1 pre-activations of the restatement span {seen}")
    _against_contract("saturated hd64", got, g, dims, seqs)
    for mode in ("0", "2"):
        s, t = _call(sc, seqs, False, mode)
        assert s.tobytes() == fs.tobytes() and _same(t, got), mode
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [seqs[5][:20]], what="saturated prime", flat=False)
    for plan in _check(rigs, sc, seqs[-3:-1], what="saturated cached"):
        assert plan["reused"] == 19


# ---- full widths ------------------------------------------------------------------------------------------------------------
WIDTHS = {"gpt2-xl": (1600, 25, 6400), "gpt2": (768, 12, 3072)}
V_GPT2 = 50257


def _wide_state(d, H, F, V, seed):
    """One GPT-2 layer of that width plus the head, in the tiny models' weight recipe (CPU tensors)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g)
    h16 = lambda t: t.half().float()
    st = {"transformer.wte.weight": h16(rn(V, d) * 2.0 / d ** 0.5), "transformer.wpe.weight": h16(rn(128, d) / d ** 0.5)}
    for ln in ("transformer.h.0.ln_1", "transformer.h.0.ln_2", "transformer.ln_f"):
        st[ln + ".weight"], st[ln + ".bias"] = h16(1 + 0.2 * rn(d)), h16(0.3 * rn(d))
    for name, n_in, n_out in (("attn.c_attn", d, 3 * d), ("attn.c_proj", d, d), ("mlp.c_fc", d, F), ("mlp.c_proj", F, d)):
        st[f"transformer.h.0.{name}.weight"] = h16(rn(n_in, n_out) / n_in ** 0.5)
        st[f"transformer.h.0.{name}.bias"] = h16(0.3 * rn(n_out))
    return st


@pytest.mark.parametrize("width", list(WIDTHS))
def test_full_width_layer_and_head_on_every_tile_rule(width):
    """One layer plus the head at the widths of GPT-2 XL (n_embd 1600: N = 1600 and 4800 end in a partial 128- and 256-tile,
    K = 6400, head dim 64 x 25) and GPT-2 small (768), vocab 50257 (the last 64-column group has 17 columns), about 600
    tokens: B2T_CLM_GEMM_256 = 0, unset and 2 give the same bytes on the flat and the tree path, within the bound."""
    d, H, F = WIDTHS[width]
    assert 1600 % 128 and 4800 % 256 and V_GPT2 % 64 == 17
    st = _wide_state(d, H, F, V_GPT2, seed=d)
    cfg = dict(model_type="gpt2", n_embd=d, n_head=H, n_layer=1, n_positions=128, n_inner=None, vocab_size=V_GPT2,
               activation_function="gelu_new", layer_norm_epsilon=1e-5)
    sc = _scorer(st, cfg)
    st = {k: v.cuda() for k, v in st.items()}
    assert sc.dims["ffn_dim"] == F
    seqs = _prod_list(V_GPT2, seed=1, cands=24)
    seqs[3] = seqs[2][:9] + seqs[3][9:]          # a shared prefix
    seqs[5][-1] = V_GPT2 - 1                     # a target in the 17-column group
    assert 500 <= sum(map(len, seqs)) <= 700
    base = None
    for mode in ("0", None, "2"):
        s, t = _flat_and_tree(sc, seqs, mode)
        if base is None:
            base = (s, t)
        assert s.tobytes() == base[0].tobytes() and _same(t, base[1]), mode
    _against_contract(width, base[1], st, dict(sc.dims), seqs)


# ---- edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_block_edges_on_the_tree_and_cache_paths(name):
    """The first owned position of the later candidates, and the cache's R, at 31, 32, 33, 63, 64, 65 (read-only near and far
    behind R, then updating); a path of exactly n_positions = 128 with R = 126."""
    sc, _, _, dims = _tiny(name)
    V = dims["vocab"]
    rng = np.random.default_rng(dims["d_model"])
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    chain = [2] + r(127)
    for Rr in (31, 32, 33, 63, 64, 65):
        _flat_and_tree(sc, [chain[:Rr] + r(int(n)) for n in rng.integers(1, 40, 8)])      # first owned position Rr
        rigs = _rigs(sc, 128)
        for plan in _check(rigs, sc, [chain[:Rr + 1]], what=f"{name} prime {Rr}", flat=False):
            assert plan["n_after"] == Rr + 1
        near = [chain[:Rr + 1] + r(n) for n in (20, 45, 1, 7)]
        far = [chain[:Rr + 30] + r(n) for n in (20, 30, 1)] + [chain[:Rr + 30]]
        for tag, seqs in (("near", near), ("far", far)):
            for plan in _check(rigs, sc, seqs, update=0, what=f"{name} R {Rr} {tag}"):
                assert plan["reused"] == Rr
        _check(rigs, sc, far, what=f"{name} R {Rr} far, updating", flat=False)
        for plan in _check(rigs, sc, far, what=f"{name} R {Rr} far again", flat=False):
            assert plan["reused"] == Rr + 29
    rigs = _rigs(sc, 128)
    _check(rigs, sc, [chain[:127]], what="prime 127", flat=False)
    seqs = [chain, chain[:127] + r(1), chain[:127]]
    assert max(map(len, seqs)) == 128 == dims["max_pos"]
    for plan in _check(rigs, sc, seqs, what=f"{name} n_positions"):
        assert plan["reused"] == 126 and plan["rows"] == 3


def test_small_caps_changing_contexts_and_odd_lists():
    """Caps of trunk - 1 and 1; the context replaced, halved, emptied and restored; a forest, duplicates, a lone sequence,
    one-token sequences."""
    sc, _, _, dims = _tiny("hd80")
    V = dims["vocab"]
    rng = np.random.default_rng(7)
    r = lambda n: [int(x) for x in rng.integers(4, V, n)]
    ctx = [2] + r(69)
    lst = lambda c: [c + t for t in (r(9), r(12), r(3))]
    for cap in (69, 1):
        rigs = _rigs(sc, cap)
        for plan in _check(rigs, sc, lst(ctx), what=f"cap {cap}"):
            assert plan["trunk"] == 70 and plan["n_after"] == cap
        for plan in _check(rigs, sc, lst(ctx), what=f"cap {cap} again", flat=False):
            assert plan["common"] == cap and plan["reused"] == cap - 1
    rigs = _rigs(sc, 128)
    other = ctx[:35] + r(35)
    for tag, c, common in (("first", ctx, 0), ("replaced", other, 35), ("half", other[:35], 35), ("emptied", [2], 1),
                           ("restored", ctx, 1), ("diverging early", ctx[:10] + r(60), 10), ("restored again", ctx, 10)):
        for plan in _check(rigs, sc, lst(c), what=f"context {tag}", flat=tag in ("first", "replaced")):
            assert plan["common"] == common and plan["n_after"] == len(c), (tag, plan)
    a = [2] + r(40)
    rigs = _rigs(sc, 128)
    for plan in _check(rigs, sc, [a, a[:10] + r(5)], update=0, what="read-only, empty cache"):
        assert (plan["trunk"], plan["reused"]) == (10, 0)
    for plan in _check(rigs, sc, [a], what="lone"):
        assert (plan["reused"], plan["rows"], plan["n_after"]) == (0, 41, 41)
    for plan in _check(rigs, sc, [a], what="lone again"):
        assert (plan["reused"], plan["rows"]) == (40, 1)
    for plan in _check(rigs, sc, [a, a, a], what="all equal"):
        assert (plan["trunk"], plan["rows"]) == (41, 1)
    b = a[:20] + r(10)
    for plan in _check(rigs, sc, [a, b, a, a + r(2), b], what="duplicates"):
        assert (plan["trunk"], plan["reused"], plan["n_after"]) == (20, 19, 20)
    for plan in _check(rigs, sc, [a, [3] + r(9), a[:7] + r(3), [3]], what="forest"):
        assert (plan["trunk"], plan["reused"], plan["n_after"]) == (0, 0, 0)
    assert all(rig.n == 0 for rig in rigs)
    for plan in _check(rigs, sc, [a + r(3), a + r(4)], what="after the forest"):
        assert (plan["reused"], plan["n_after"]) == (0, 41)
    for plan in _check(rigs, sc, [[2], [2]], what="one token"):
        assert (plan["trunk"], plan["common"], plan["reused"], plan["rows"]) == (1, 1, 0, 1)
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])
    _flat_and_tree(sc, [[10 * i + j for j in range(1, 6)] for i in range(1, 9)])          # no sharing
    s, t = _call(sc, [[2], [5, 6]], False)
    assert s[0] == 0.0 and t[0].tolist() == [0.0]


@pytest.mark.parametrize("name", list(TINY))
def test_score_alone_equals_score_in_a_batch(name):
    sc, _, _, dims = _tiny(name)
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


# ---- picks and the service --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_picks_on_the_recorded_lists_equal_hf_fp32(name):
    """gpt2_lm_decode on the recorded n-best lists, with and without a context string: the Gpt2Scorer (flat and sharing
    prefixes) picks the sentence the HF fp32 model's scores pick."""
    sc, model, _, dims = _tiny(name)
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tk = R.WordTokenizer(vocab_size=dims["vocab"], bos_id=2, pad_id=1)
    hfs = _HfScorer(model)
    seen = set()
    for c in gold["decode"]:
        kw = dict(length_penalty=c["length_penalty"], alpha=c["alpha"], returnConfidence=c["confidence"],
                  current_context_str=c["context"])
        theirs = R.gpt2_lm_decode(hfs, tk, "cpu", c["nbest"], 0.35, **kw)
        for tree in (False, True):
            sc.share_prefixes = tree
            ours = R.gpt2_lm_decode(sc, tk, "cuda", c["nbest"], 0.35, **kw)
            assert ours[0] == theirs[0], (name, c["case"], c["context"], tree)
        seen.add(bool(c["context"] and c["context"].split()))
    sc.share_prefixes = False
    assert seen == {True, False}
    # and the scorer's numbers are HF's to fp16 precision on one of those lists
    ids = tk([e[0] for e in gold["decode"][0]["nbest"] if e[0].strip()])["input_ids"]
    got, hf = np.concatenate(sc.token_logprobs(ids)), np.concatenate(hf_logp(model, ids))
    assert np.abs(got - hf).max() <= BOUND_CAP


def test_service_end_to_end_with_a_gpt2_scorer(tmp_path):
    """build_scorer on a GPT-2 directory gives a Gpt2Scorer; LocalLMService with do_opt = 1 over three sentences with a growing
    context: with a context cache the replies are, field by field, those of a scorer without, and from the second sentence on
    the context is reused."""
    import evaluate_model_helpers as H
    from remote_lm import LocalLMService
    model, cfg = tiny_gpt2("hd64")
    model.save_pretrained(str(tmp_path))
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(vocab_size=cfg["vocab_size"], bos_id=2, pad_id=1)
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies, reused = {}, {}
    for cache_tokens in (0, 128):
        sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto", context_cache_tokens=cache_tokens)
        assert type(sc) is R.Gpt2Scorer
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
    print(f"CLM gpt2 service: reused per sentence {reused[128]}")
    assert reused[0] == [None, None, None]
    assert reused[128][0] == 0 and 0 < reused[128][1] < reused[128][2], reused
    # the scorer's surface: the ABI's bytes, last_stats, the length penalty
    sc = R.build_scorer(str(tmp_path), device="cuda")
    seqs = tiny_seqs(cfg["vocab_size"], seed=8, lens=(1, 9, 40))
    s, t = _call(sc, seqs, False)
    for tree in (False, True):
        assert _same(sc.token_logprobs(seqs, share_prefixes=tree), t)
        assert sc.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
        assert sc.score(seqs, 0.25, share_prefixes=tree).tobytes() == (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    with pytest.raises(RuntimeError, match="b2t_clm_gpt2_score_f16.*max_pos"):
        sc.score([[2] * 129])
    with pytest.raises(RuntimeError, match="b2t_clm_gpt2_score_tree_f16.*outside"):
        sc.score([[2, 5, cfg["vocab_size"]]], share_prefixes=True)
