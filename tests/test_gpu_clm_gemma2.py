"""b2t_clm_gemma2_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_gemma2.hip) on the MI355X,
driven through the C ABI: against the float64 restatement of the contract (ref_logp_gemma2 of tests/test_clm_gemma2_host.py, on
the GPU here) in both formats, the bit identities (tree = flat, the forced tile modes, alone = in a batch, the cached call under
both settings of B2T_CLM_TRUNK_ATTN), planted differences in the descriptor and the norm weights, and the Python surface.

Conventions as in tests/test_gpu_clm_olmo2.py: every call (_call) gets a fresh workspace of exactly the size the library asks
for (the b2t_clm_gemma2_* size functions'), filled with 0xFF, with canaries behind it and behind both outputs.

The bounds are the project's: fp16 within min(3 x e16, 1e-2) of the fp16-rounded restatement, bf16 within 3 x e_bf16 after
e_bf16 <= 0.1, e16 and e_bf16 being what the contract's roundings alone do to the log-probs of the case (restatement against
restatement, never the kernels).  The tiny models have head dims 256 and 128, an attention output (512 columns) wider than the
residual (128, 192), caps of 2.0 / 3.0 that both matter (tests/test_clm_gemma2_host.py measures it) and a q scale that is not
head_dim^-0.5.  The measured ratios are in NOTES.md ("LLM")."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import llm_rescore as R
from test_clm_gemma2_host import E_BF16_MAX, TINY, gemma2_state, ref_logp_gemma2, tiny_gemma2
from test_clm_llama_host import tiny_seqs
from test_gpu_clm_cache import SETTINGS, _same_bytes
from test_gpu_clm_llama import _call as _family_call, _prod_list, _same
from test_gpu_clm_llama_cache import FamilyLib, Rig

pytestmark = pytest.mark.gpu
LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # 692 rows: crosses the 128- and the 256-row tile boundaries


# one Gemma-2 C ABI call in the scorer's dtype: tests/test_gpu_clm_llama.py's _call, which takes the entry points, the sizes and
# their extra arguments from the scorer, on a scorer that must be of this family
_call = functools.partial(_family_call, family="gemma2")


def _flat_and_tree(sc, seqs, mode=None):
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


def _scorer(st, cfg, fmt, **over):
    """The scorer of a state dict; `over` replaces entries of the dims (the descriptor's q scale and caps)."""
    dims = R.gemma2_dims(cfg) | over
    return R.Gemma2Scorer(dims, R.gemma2_device_layout(st, dims, R.rope_inv_freq(cfg), dtype=fmt), "cuda", dtype=fmt)


_TINY, _REF = {}, {}


def _tiny(name, fmt):
    """(scorer in fmt, GPU state dict, reference dims, inv_freq, config) of a tiny model with fmt-valued weights, cached."""
    if (name, fmt) not in _TINY:
        _, cfg, st, rd, inv = gemma2_state(name, fmt=fmt)
        _TINY[name, fmt] = (_scorer(st, cfg, fmt), {k: v.cuda() for k, v in st.items()}, rd, inv, cfg)
    return _TINY[name, fmt]


def _contract_seqs(V):
    seqs = tiny_seqs(V, seed=3, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate


def _refs(name, fmt):
    """(rounded, unrounded) restatement of _contract_seqs, computed once per model and format and left unchanged."""
    if (name, fmt) not in _REF:
        _, st, rd, inv, _ = _tiny(name, fmt)
        seqs = _contract_seqs(rd["vocab"])
        _REF[name, fmt] = (np.concatenate(ref_logp_gemma2(st, rd, inv, seqs, fmt)), np.concatenate(ref_logp_gemma2(st, rd, inv, seqs)))
    return _REF[name, fmt]


def _bound(fmt, e):
    if fmt == "float16":
        assert e > 0
        return min(3 * e, 1e-2)
    assert 0 < e <= E_BF16_MAX, e
    return 3 * e


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_against_the_contract(name, fmt):
    """Flat and tree (bit-identical) against the rounded float64 restatement, fp16: max |dlogp| <= min(3 e16, 1e-2); bf16:
    <= 3 e_bf16 after e_bf16 <= 0.1.  B2T_CLM_GEMM_256 = 0 and 2 give the default's bytes on both paths.

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, st, rd, inv, _ = _tiny(name, fmt)
    seqs = _contract_seqs(rd["vocab"])
    assert sum(LENS) == 692 and len(seqs) == len(LENS) + 3
    fs, got = _flat_and_tree(sc, seqs)
    ref, exact = _refs(name, fmt)
    g = np.concatenate(got)
    assert g.shape == ref.shape
    e, err = float(np.abs(ref - exact).max()), float(np.abs(g - ref).max())
    print(f"CLM gemma2 contract {name} {fmt}: tokens {len(g)} max |dlogp| {err:.3e}  e {e:.3e}  ratio {err / e:.3f}  "
          f"(max |logp| {np.abs(ref).max():.2f})")
    assert err <= _bound(fmt, e), (name, err, e)
    for mode in ("0", "2"):
        for tree in (False, True):
            s, t = _call(sc, seqs, tree, mode)
            assert s.tobytes() == fs.tobytes() and _same(t, got), (mode, tree)


def test_edge_cases_covered():
    assert {c["head_dim"] for c in TINY.values()} == {128, 256}
    for c in TINY.values():
        assert c["num_attention_heads"] * c["head_dim"] > c["hidden_size"]      # the attention output is wider than the residual
        assert c["query_pre_attn_scalar"] != c["head_dim"] and c["num_attention_heads"] // c["num_key_value_heads"] == 2
        assert c["vocab_size"] % 64 and c["intermediate_size"] % 128


def _planted(name, what, change=None, **over):
    """The scorer of a changed state dict (change) or descriptor (over: entries of the dims) leaves the bound around the
    unchanged model's restatement, and follows the changed model's restatement within its bound: the kernels read that."""
    _, cfg, st, rd, inv = gemma2_state(name)
    st2 = change(st) if change else st
    rd2 = rd | over
    seqs = tiny_seqs(rd["vocab"], seed=5, lens=(17, 64, 65))
    g1, g2 = ({k: v.cuda() for k, v in s.items()} for s in (st, st2))
    ref1, exact1 = (np.concatenate(ref_logp_gemma2(g1, rd, inv, seqs, f)) for f in ("float16", None))
    ref2, exact2 = (np.concatenate(ref_logp_gemma2(g2, rd2, inv, seqs, f)) for f in ("float16", None))
    base = np.concatenate(_flat_and_tree(_tiny(name, "float16")[0], seqs)[1])
    got = np.concatenate(_flat_and_tree(_scorer(st2, cfg, "float16", **over), seqs)[1])
    b1, b2 = _bound("float16", float(np.abs(ref1 - exact1).max())), _bound("float16", float(np.abs(ref2 - exact2).max()))
    off = float(np.abs(got - ref1).max())
    print(f"CLM gemma2 planted {name} {what}: against the unchanged restatement {off:.3f} (bound {b1:.3e}), against its own "
          f"{np.abs(got - ref2).max():.3e} (bound {b2:.3e})")
    assert np.abs(base - ref1).max() <= b1
    assert off > b1, (off, b1)
    assert np.abs(got - ref2).max() <= b2


@pytest.mark.parametrize("cap", ["attn_cap", "final_cap"])
@pytest.mark.parametrize("name", list(TINY))
def test_a_cap_of_zero_is_off(name, cap):
    _planted(name, f"{cap} = 0 in the descriptor", **{cap: 0.0})


@pytest.mark.parametrize("name", list(TINY))
def test_exchanged_feedforward_norms_leave_the_bound(name):
    def swap(st):
        out = dict(st)
        for k in st:
            if "pre_feedforward_layernorm" in k:
                o = k.replace("pre_feedforward_layernorm", "post_feedforward_layernorm")
                out[k], out[o] = st[o], st[k]
        return out
    _planted(name, "pre- and post-feedforward norm weights exchanged", swap)


@pytest.mark.parametrize("name", list(TINY))
def test_w_minus_one_as_the_weight_leaves_the_bound(name):
    """1 + (w - 1) = w: what a kernel that multiplied by w alone would compute from the unchanged weights."""
    _planted(name, "w - 1 as every norm weight",
             lambda st: {k: ((v - 1).half().float() if k.endswith("norm.weight") or "layernorm" in k else v) for k, v in st.items()})


@pytest.mark.parametrize("name", list(TINY))
def test_q_scale_of_head_dim_leaves_the_bound(name):
    _planted(name, "q scale head_dim^-0.5", q_scale=TINY[name]["head_dim"] ** -0.5)


# ---- bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_score_alone_equals_score_in_a_batch(name, fmt):
    sc, _, rd, _, _ = _tiny(name, fmt)
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
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])                               # one-token sequences: no head rows


# ---- the cached call --------------------------------------------------------------------------------------------------------
class Gemma2Rig(Rig):
    """Rig sizes its slab rows by d_model / n_heads; it is built on the Llama shape of width Hq hd, whose cache rows have
    Gemma-2's size, then pointed at the scorer and at Gemma-2's calls."""

    def __init__(self, sc, cap, setting):
        import b2t_native as N
        wide = N.ClmLlamaDesc.from_buffer_copy(sc.desc)
        wide.d_model = sc.dims["n_heads"] * sc.dims["head_dim"]
        super().__init__(types.SimpleNamespace(dims=dict(sc.dims, d_model=wide.d_model), desc=wide), cap, setting)
        assert self.lib.b2t_clm_gemma2_cache_kv_bytes(C.byref(sc.desc), sc._g2, cap) == self.kv.numel() * 2
        self.sc, self.lib = sc, FamilyLib(self.lib, sc, "gemma2")


def _rigs(sc, cap):
    return [Gemma2Rig(sc, cap, s) for s in SETTINGS]


@pytest.mark.parametrize("name", list(TINY))
def test_cached_session_of_three_growing_contexts(name):
    """Three 20-candidate lists behind a context of 30 tokens that grows by the first candidate of the call before: cached =
    tree = flat byte for byte, read-only and updating, B2T_CLM_TRUNK_ATTN 0 and 1, the tile rule changing from call to call."""
    import bench_llm_rescore as B
    sc, _, rd, _, _ = _tiny(name, "float16")
    V, max_pos = rd["vocab"], sc.dims["max_pos"]
    rigs = _rigs(sc, max_pos)
    rng = np.random.default_rng(V)
    ctx, prev = [int(x) for x in rng.integers(4, V, 30)], None
    for k, mode in enumerate(("0", None, "2")):
        seqs = B.nbest_list(rng, V, 20, ctx)
        assert max(map(len, seqs)) <= max_pos
        tree = _call(sc, seqs, True, mode)
        _same_bytes(_call(sc, seqs, False, mode), tree, f"{name} call {k}: flat against tree")
        for rig in rigs:
            for update in (0, 1):
                s, t, plan = rig.call(seqs, mode, update)
                _same_bytes((s, t), tree, f"{name} call {k}: cached (update {update}, trunk attention {rig.setting}) against tree")
            assert plan["trunk"] >= len(ctx) + 1
            if prev is not None:
                assert plan["common"] == prev and plan["reused"] == prev - 1 >= 30
            last = plan
        prev = last["n_after"]
        ctx = [int(x) for x in seqs[0][1:]]
    assert last["reused"] >= 32     # the third call reused a whole 32-key block: stage B ran under B2T_CLM_TRUNK_ATTN = 1


@pytest.mark.parametrize("name", list(TINY))
def test_cached_reuse_below_at_and_above_the_block_edges(name):
    """R = 31, 32, 33, 64: a cache primed with R + 1 positions, then a list behind them, read-only and updating, under both
    settings of B2T_CLM_TRUNK_ATTN (stage B off and on): byte-identical to the tree call."""
    sc, _, rd, _, _ = _tiny(name, "float16")
    assert SETTINGS == ("0", "1")
    rng = np.random.default_rng(len(name))
    r = lambda n: [int(x) for x in rng.integers(4, rd["vocab"], n)]
    chain = [2] + r(79)
    for Rr in (31, 32, 33, 64):
        seqs = [chain[:Rr + 1] + r(n) for n in (20, 45, 1, 7)]
        tree = _call(sc, seqs, True)
        for rig in _rigs(sc, 80):
            s, t, plan = rig.call([chain[:Rr + 1]])
            assert plan["n_after"] == Rr + 1
            for update in (0, 1):
                s, t, plan = rig.call(seqs, None, update)
                assert plan["reused"] == Rr
                _same_bytes((s, t), tree, f"{name} R {Rr}: cached (update {update}, trunk attention {rig.setting}) against tree")


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorer_surface_on_the_gpu(tmp_path):
    import torch
    model, cfg = tiny_gemma2("hd256", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto")
    assert isinstance(sc, R.Gemma2Scorer) and sc.dtype is torch.bfloat16 and sc._family == "gemma2"
    sbf = R.build_scorer(str(tmp_path), device="cuda", dtype="bfloat16")
    s16 = R.build_scorer(str(tmp_path), device="cuda")
    assert isinstance(s16, R.Gemma2Scorer) and s16.dtype is torch.float16 and sbf.dtype is torch.bfloat16
    assert _same(sbf.token_logprobs(seqs), sc.token_logprobs(seqs))
    for scorer in (sc, s16):
        s, t = _call(scorer, seqs, False)
        for tree in (False, True):
            assert _same(scorer.token_logprobs(seqs, share_prefixes=tree), t)
            assert scorer.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
            assert scorer.score(seqs, 0.25, share_prefixes=tree).tobytes() == \
                (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    assert not _same(sc.token_logprobs(seqs), s16.token_logprobs(seqs))       # two formats, two functions
    shared = R.build_scorer(str(tmp_path), device="cuda", share_prefixes=True)
    assert shared.share_prefixes and _same(shared.token_logprobs(seqs), s16.token_logprobs(seqs))
    assert shared.last_stats["nodes"] == 48
    # the context cache in fp16: the second call reuses the first one's trunk, the scores are the uncached scorer's
    with pytest.raises(ValueError, match="follow-up"):
        R.build_scorer(str(tmp_path), device="cuda", dtype="auto", context_cache_tokens=64)
    sc64 = R.build_scorer(str(tmp_path), device="cuda", context_cache_tokens=64)
    rng = np.random.default_rng(3)
    ctx = [2] + list(rng.integers(4, V, 40))
    for k in range(2):
        lst = [ctx + list(rng.integers(4, V, int(n))) for n in (5, 9, 3)]
        got = sc64.token_logprobs(lst)
        assert _same(got, s16.token_logprobs(lst, share_prefixes=True))
        assert sc64.last_stats["reused"] == (0 if k == 0 else 40)
    assert sc64.last_stats["reused"] > 0 and sc64.cache_len == 41
