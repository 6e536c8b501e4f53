"""b2t_clm_qwen3_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_qwen3.hip) on the MI355X,
driven through the C ABI: against the float64 restatement of the contract with the q / k norm inserted (ref_logp_qwen3 of
tests/test_clm_qwen3_host.py, on the GPU here) in both formats, the bit identities of the Llama paths (tree = flat, the forced
tile modes, alone = in a batch, the cached call), a planted difference in the norm weights, and the Python surface.

Conventions as in tests/test_gpu_clm_llama.py: every call (_call) gets a fresh workspace of exactly the size the library asks
for (the Llama size functions'), filled with 0xFF, with canaries behind it and behind both outputs.

The bounds are the project's: fp16 within min(3 x e16, 1e-2) of the fp16-rounded restatement, bf16 within 3 x e_bf16 after
e_bf16 <= 0.1, e16 and e_bf16 being what the contract's roundings alone do to the log-probs of the case (restatement against
restatement, never the kernels).  The two tiny models have QKV widths 640 and 384: the last 256-column tile has waves beyond
N, which must reach the epilogue's barrier; a 256-tile holds a q head beside a k head with other norm weights and v slices
beside normed ones; group sizes 3 and 4; head dims 128 (the norm's sum crosses two waves through LDS) and 64.  The measured
ratios are in NOTES.md ("LLM")."""
import functools

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import dict_rule  # noqa: F401  (Rig uses it)
from test_clm_llama_host import tiny_seqs
from test_clm_qwen3_host import E_BF16_MAX, TINY, qwen3_state, ref_logp_qwen3, tiny_qwen3
from test_gpu_clm_cache import SETTINGS, _same_bytes
from test_gpu_clm_llama import _call as _family_call, _prod_list, _same
from test_gpu_clm_llama_cache import FamilyLib, Rig

pytestmark = pytest.mark.gpu
LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # 692 rows: crosses the 128- and the 256-row tile boundaries


# one Qwen3 C ABI call in the scorer's dtype: tests/test_gpu_clm_llama.py's _call, which takes the entry points, the sizes and
# their extra arguments from the scorer, on a scorer that must be of this family
_call = functools.partial(_family_call, family="qwen3")


def _flat_and_tree(sc, seqs, mode=None):
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


def _scorer(st, cfg, fmt):
    dims = R.llama_dims(cfg)
    return R.LlamaScorer(dims, R.llama_device_layout(st, dims, R.rope_inv_freq(cfg), dtype=fmt), "cuda", dtype=fmt)


_TINY, _REF = {}, {}


def _tiny(name, fmt):
    """(scorer in fmt, GPU state dict, reference dims, inv_freq) of a tiny model with fmt-valued weights, cached."""
    if (name, fmt) not in _TINY:
        _, cfg, st, rd, inv = qwen3_state(name, fmt=fmt)
        _TINY[name, fmt] = (_scorer(st, cfg, fmt), {k: v.cuda() for k, v in st.items()}, rd, inv)
    return _TINY[name, fmt]


def _contract_seqs(V):
    seqs = tiny_seqs(V, seed=3, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate


def _refs(name, fmt):
    """(rounded, unrounded) restatement of _contract_seqs, computed once per model and format."""
    if (name, fmt) not in _REF:
        _, st, rd, inv = _tiny(name, fmt)
        seqs = _contract_seqs(rd["vocab"])
        _REF[name, fmt] = (np.concatenate(ref_logp_qwen3(st, rd, inv, seqs, fmt)), np.concatenate(ref_logp_qwen3(st, rd, inv, seqs)))
    return _REF[name, fmt]


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_against_the_contract(name, fmt):
    """Flat and tree (bit-identical) against the rounded float64 restatement, fp16: max |dlogp| <= min(3 e16, 1e-2); bf16:
    <= 3 e_bf16 after e_bf16 <= 0.1.  B2T_CLM_GEMM_256 = 0 and 2 give the default's bytes on both paths.

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, st, rd, inv = _tiny(name, fmt)
    seqs = _contract_seqs(rd["vocab"])
    fs, got = _flat_and_tree(sc, seqs)
    ref, exact = _refs(name, fmt)
    g = np.concatenate(got)
    assert g.shape == ref.shape
    e, err = float(np.abs(ref - exact).max()), float(np.abs(g - ref).max())
    print(f"CLM qwen3 contract {name} {fmt}: tokens {len(g)} max |dlogp| {err:.3e}  e {e:.3e}  ratio {err / e:.3f}  "
          f"(max |logp| {np.abs(ref).max():.2f})")
    if fmt == "float16":
        assert e > 0 and err <= min(3 * e, 1e-2), (name, err, e)
    else:
        assert 0 < e <= E_BF16_MAX, (name, e)
        assert err <= 3 * e, (name, err, e)
    for mode in ("0", "2"):
        for tree in (False, True):
            s, t = _call(sc, seqs, tree, mode)
            assert s.tobytes() == fs.tobytes() and _same(t, got), (mode, tree)


def test_edge_cases_covered():
    widths = {(c["num_attention_heads"] + 2 * c["num_key_value_heads"]) * c["head_dim"] for c in TINY.values()}
    assert widths == {640, 384} and all(w % 256 for w in widths)       # the last 256-tile has waves beyond N
    assert {c["num_attention_heads"] // c["num_key_value_heads"] for c in TINY.values()} == {3, 4}
    assert {c["head_dim"] for c in TINY.values()} == {64, 128}
    assert all(c["head_dim"] * c["num_attention_heads"] == c["hidden_size"] for c in TINY.values())


@pytest.mark.parametrize("name,which", [("hd128", "q_norm"), ("hd64", "k_norm")])
def test_a_planted_difference_in_the_norm_weights_shows(name, which):
    """Layer 1's q_norm (k_norm) weight doubled: the restatement moves by far more than the bound, and the kernels follow it --
    they read the weights of that layer and of that head kind."""
    _, cfg, st, rd, inv = qwen3_state(name)
    key = f"model.layers.1.self_attn.{which}.weight"
    st2 = dict(st, **{key: st[key] * 2})
    seqs = tiny_seqs(rd["vocab"], seed=5, lens=(17, 64, 65))
    g2 = {k: v.cuda() for k, v in st2.items()}
    ref2 = np.concatenate(ref_logp_qwen3(g2, rd, inv, seqs, "float16"))
    exact2 = np.concatenate(ref_logp_qwen3(g2, rd, inv, seqs))
    base = np.concatenate(_flat_and_tree(_tiny(name, "float16")[0], seqs)[1])
    got = np.concatenate(_flat_and_tree(_scorer(st2, cfg, "float16"), seqs)[1])
    e16 = float(np.abs(ref2 - exact2).max())
    moved = float(np.abs(got - base).max())
    print(f"CLM qwen3 planted {name} {which}: scores moved by {moved:.3f}, e16 {e16:.3e}, against the restatement {np.abs(got - ref2).max():.3e}")
    assert np.abs(got - ref2).max() <= min(3 * e16, 1e-2)
    assert moved > 10 * min(3 * e16, 1e-2)     # measured in the restatement: 1.84 (hd128, q_norm), 1.61 (hd64, k_norm)


# ---- bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_score_alone_equals_score_in_a_batch(name, fmt):
    sc, _, rd, _ = _tiny(name, fmt)
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


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_tree_equals_flat_at_the_block_edges(name, fmt):
    """The first owned position of the later candidates at 31, 32, 33, 63, 64, 65, on every tile path."""
    sc, _, rd, _ = _tiny(name, fmt)
    rng = np.random.default_rng(5)
    r = lambda n: list(rng.integers(4, rd["vocab"], n))
    for own in (31, 32, 33, 63, 64, 65):
        ctx = [2] + r(own - 1)
        seqs = [ctx + r(int(n)) for n in rng.integers(1, 40, 12)]
        base = _flat_and_tree(sc, seqs)
        for mode in ("0", "2"):
            s, t = _flat_and_tree(sc, seqs, mode)
            assert s.tobytes() == base[0].tobytes() and _same(t, base[1]), (own, mode)
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])                               # one-token sequences
    _flat_and_tree(sc, [[2] + r(5), [3] + r(5), [2, 5, 7], [3, 5]])             # a forest


# ---- the cached call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_cached_session_of_three_growing_contexts(name):
    """Three 20-candidate lists behind a context of 30 tokens that grows by the first candidate of the call before: cached = tree = flat byte for
    byte, read-only and updating, B2T_CLM_TRUNK_ATTN 0 and 1, the tile rule changing from call to call.  Rig checks rows, reused
    and n against the dictionary rule, the canaries around the cache, and that a read-only call leaves it alone."""
    import bench_llm_rescore as B
    sc, _, rd, _ = _tiny(name, "float16")
    V, max_pos = rd["vocab"], sc.dims["max_pos"]
    rigs = [Rig(sc, max_pos, s) for s in SETTINGS]
    for rig in rigs:
        rig.lib = FamilyLib(rig.lib, sc, "qwen3")
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


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorer_surface_on_the_gpu(tmp_path):
    import torch
    model, cfg = tiny_qwen3("hd128", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto")
    assert isinstance(sc, R.LlamaScorer) and sc.dtype is torch.bfloat16 and sc._family == "qwen3"
    s16 = R.build_scorer(str(tmp_path), device="cuda")
    assert s16.dtype is torch.float16 and s16._family == "qwen3"
    for scorer in (sc, s16):
        s, t = _call(scorer, seqs, False)
        for tree in (False, True):
            assert _same(scorer.token_logprobs(seqs, share_prefixes=tree), t)
            assert scorer.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
            assert scorer.score(seqs, 0.25, share_prefixes=tree).tobytes() == \
                (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    assert not _same(sc.token_logprobs(seqs), s16.token_logprobs(seqs))       # two formats, two functions
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
