"""b2t_clm_phi3_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_phi3.hip) on the MI355X, driven
through the C ABI: against the float64 restatement of the contract (ref_logp_phi3 of tests/test_clm_phi3_host.py, on the GPU
here) in both formats, the bit identities (tree = flat, the forced tile modes, alone = in a batch, the cached call under both
settings of B2T_CLM_TRUNK_ATTN), planted differences in the rotary table, the descriptor and the fused QKV weight, and the
Python surface.

Conventions as in tests/test_gpu_clm_olmo2.py: every call (_call) gets a fresh workspace of exactly the size the library asks
for (the b2t_clm_phi3_* size functions'), filled with 0xFF, with canaries behind it and behind both outputs.

The bounds are the project's: fp16 within min(3 x e16, 1e-2) of the fp16-rounded restatement, bf16 within 3 x e_bf16 after
e_bf16 <= 0.1, e16 and e_bf16 being what the contract's roundings alone do to the log-probs of the case (restatement against
restatement, never the kernels).  The tiny models are tests/test_clm_phi3_host.py's: head dim 96 with and without grouped
queries, 96 of 128 dims rotated under LongRoPE, head dim 128, and a head dim of its own (2 heads of 128 on a residual of 192).
The measured ratios are in NOTES.md ("LLM")."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import llm_rescore as R
from test_clm_llama_host import tiny_seqs
from test_clm_phi3_host import E_BF16_MAX, HEAD_DIM, TINY, phi3_state, ref_logp_phi3, tiny_phi3
from test_gpu_clm_cache import SETTINGS, _same_bytes
from test_gpu_clm_llama import _call as _family_call, _prod_list, _same
from test_gpu_clm_llama_cache import FamilyLib, Rig

pytestmark = pytest.mark.gpu
LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # 692 rows: crosses the 32-key block and the 128- / 256-row tiles


# one Phi-3 C ABI call in the scorer's dtype: tests/test_gpu_clm_llama.py's _call, which takes the entry points, the sizes and
# their extra arguments from the scorer, on a scorer that must be of this family
_call = functools.partial(_family_call, family="phi3")


def _flat_and_tree(sc, seqs, mode=None):
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


def _scorer(st, cfg, fmt, rope=None, **over):
    """The scorer of a state dict; `over` replaces entries of the dims (the descriptor's rotary dims), `rope` the table's
    (inv_freq, attention factor)."""
    dims = R.phi3_dims(cfg) | over
    return R.Phi3Scorer(dims, R.phi3_device_layout(st, dims, rope or R.phi3_rope(cfg), dtype=fmt), "cuda", dtype=fmt)


_TINY, _REF = {}, {}


def _tiny(name, fmt):
    """(scorer in fmt, GPU state dict, reference dims, (inv_freq, attention factor), config) of a tiny model with fmt-valued
    weights, cached."""
    if (name, fmt) not in _TINY:
        _, cfg, st, rd, rope = phi3_state(name, fmt=fmt)
        _TINY[name, fmt] = (_scorer(st, cfg, fmt), {k: v.cuda() for k, v in st.items()}, rd, rope, cfg)
    return _TINY[name, fmt]


def _contract_seqs(V):
    seqs = tiny_seqs(V, seed=3, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate


def _refs(name, fmt):
    """(rounded, unrounded) restatement of _contract_seqs, computed once per model and format and left unchanged."""
    if (name, fmt) not in _REF:
        _, st, rd, rope, _ = _tiny(name, fmt)
        seqs = _contract_seqs(rd["vocab"])
        _REF[name, fmt] = (np.concatenate(ref_logp_phi3(st, rd, rope, seqs, fmt)), np.concatenate(ref_logp_phi3(st, rd, rope, seqs)))
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
    sc, st, rd, rope, _ = _tiny(name, fmt)
    assert sc.desc.max_pos >= max(LENS) and sc._phi3.head_dim == HEAD_DIM[name]
    seqs = _contract_seqs(rd["vocab"])
    assert sum(LENS) == 692 and len(seqs) == len(LENS) + 3
    fs, got = _flat_and_tree(sc, seqs)
    ref, exact = _refs(name, fmt)
    g = np.concatenate(got)
    assert g.shape == ref.shape
    e, err = float(np.abs(ref - exact).max()), float(np.abs(g - ref).max())
    print(f"CLM phi3 contract {name} {fmt}: tokens {len(g)} max |dlogp| {err:.3e}  e {e:.3e}  ratio {err / e:.3f}  "
          f"(max |logp| {np.abs(ref).max():.2f})")
    assert err <= _bound(fmt, e), (name, err, e)
    for mode in ("0", "2"):
        for tree in (False, True):
            s, t = _call(sc, seqs, tree, mode)
            assert s.tobytes() == fs.tobytes() and _same(t, got), (mode, tree)


def test_edge_cases_covered():
    assert {HEAD_DIM[n] for n in TINY} == {96, 128}
    c = TINY["hd96gqa"]
    assert c["num_attention_heads"] // c["num_key_value_heads"] == 4
    assert (c["num_attention_heads"] + c["num_key_value_heads"]) * 96 % 64 == 32      # v shares a 64-column group with k
    p = TINY["partial"]
    assert p["partial_rotary_factor"] * 128 == 96 and p["rope_parameters"]["short_factor"] != p["rope_parameters"]["long_factor"]
    assert p["tie_word_embeddings"] and not TINY["hd96"]["tie_word_embeddings"]
    w = TINY["wide"]
    assert w["num_attention_heads"] * w["head_dim"] > w["hidden_size"]       # the attention output is wider than the residual
    for c in TINY.values():
        assert c["vocab_size"] % 64 and c["intermediate_size"] % 128


# ---- planted changes ------------------------------------------------------------------------------------------------------
def _planted(name, what, change=None, cfg_change=None, rope2=None, **over):
    """The scorer of a changed state dict (change), config (cfg_change), table (rope2) or descriptor (over: entries of the dims)
    leaves the bound around the unchanged model's restatement, and follows the changed model's restatement within its bound:
    the kernels read that."""
    _, cfg, st, rd, rope = phi3_state(name)
    st2 = change(st) if change else st
    cfg2 = cfg_change(json.loads(json.dumps(cfg))) if cfg_change else cfg
    rope2 = rope2(cfg2) if rope2 else R.phi3_rope(cfg2)
    rd2 = rd | over
    seqs = tiny_seqs(rd["vocab"], seed=5, lens=(17, 64, 65))
    g1, g2 = ({k: v.cuda() for k, v in s.items()} for s in (st, st2))
    ref1, exact1 = (np.concatenate(ref_logp_phi3(g1, rd, rope, seqs, f)) for f in ("float16", None))
    ref2, exact2 = (np.concatenate(ref_logp_phi3(g2, rd2, rope2, seqs, f)) for f in ("float16", None))
    base = np.concatenate(_flat_and_tree(_tiny(name, "float16")[0], seqs)[1])
    got = np.concatenate(_flat_and_tree(_scorer(st2, cfg2, "float16", rope2, **over), seqs)[1])
    b1, b2 = _bound("float16", float(np.abs(ref1 - exact1).max())), _bound("float16", float(np.abs(ref2 - exact2).max()))
    off = float(np.abs(got - ref1).max())
    print(f"CLM phi3 planted {name} {what}: against the unchanged restatement {off:.3f} (bound {b1:.3e}), against its own "
          f"{np.abs(got - ref2).max():.3e} (bound {b2:.3e})")
    assert np.abs(base - ref1).max() <= b1
    assert off > b1, (off, b1)
    assert np.abs(got - ref2).max() <= b2


def test_one_short_factor_changes_the_scores():
    def change(cfg):
        cfg["rope_parameters"]["short_factor"][3] *= 2.0
        return cfg
    _planted("partial", "short_factor[3] doubled", cfg_change=change)


def test_rotary_dims_of_the_descriptor_are_read():
    """96 -> 128 rotated dims with a table of 64 frequencies: the descriptor's field, not the model's shape, decides."""
    full = lambda cfg: (R.phi3_rope(cfg | {"partial_rotary_factor": 1.0, "rope_parameters": {"rope_type": "default",
                                                                                             "rope_theta": 10000.0}})[0],
                        R.phi3_rope(cfg)[1])
    _planted("partial", "rotary_dims 128 in the descriptor", rope2=full, rotary_dims=128)


def test_one_k_row_of_qkv_proj_changes_the_scores():
    """hd96gqa: q | k is 480 columns wide; the row is in the k head, in the 64-column group that also holds v columns."""
    def change(st):
        out = dict(st)
        w = st["model.layers.0.self_attn.qkv_proj.weight"].clone()
        w[4 * 96 + 70] = -w[4 * 96 + 70]
        out["model.layers.0.self_attn.qkv_proj.weight"] = w
        return out
    assert 448 <= 4 * 96 + 70 < 480
    _planted("hd96gqa", "row 454 of layer 0's qkv_proj negated", change)


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
CACHED = ("hd96", "hd96gqa", "partial")


def _rigs(sc, cap):
    assert sc.dims["d_model"] // sc.dims["n_heads"] == sc.dims["head_dim"]
    rigs = [Rig(sc, cap, s) for s in SETTINGS]
    for rig in rigs:
        assert rig.lib.b2t_clm_phi3_cache_kv_bytes(C.byref(sc.desc), sc._phi3, cap) == rig.kv.numel() * 2
        rig.lib = FamilyLib(rig.lib, sc, "phi3")
    return rigs


@pytest.mark.parametrize("name", CACHED)
def test_cached_session_of_four_growing_contexts(name):
    """Four 20-candidate lists behind a context of 30 tokens that grows by the first candidate of the call before, past 64
    tokens: cached = tree = flat byte for byte, read-only and updating, B2T_CLM_TRUNK_ATTN 0 and 1, the tile rule changing from
    call to call.  Rig checks rows, reused and n against the dictionary rule and cache_plan, the canaries around the cache, and
    that a read-only call leaves it as it was."""
    import bench_llm_rescore as B
    sc, _, rd, _, _ = _tiny(name, "float16")
    V, max_pos = rd["vocab"], sc.dims["max_pos"]
    rigs = _rigs(sc, max_pos)
    rng = np.random.default_rng(V)
    ctx, prev = [int(x) for x in rng.integers(4, V, 30)], None
    for k, mode in enumerate(("0", None, "2", None)):
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
    assert len(ctx) > 64 and last["reused"] >= 32     # whole 32-key blocks were reused: stage B ran under B2T_CLM_TRUNK_ATTN = 1


@pytest.mark.parametrize("name", CACHED)
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


def test_wide_model_behind_the_context_cache():
    """`wide` (Hq hd = 256 on a residual of 192; Rig sizes its rows by d_model / n_heads, so the scorer's own cache drives it):
    three calls behind a growing context, the last two reusing more than a 32-key block, under both settings of
    B2T_CLM_TRUNK_ATTN: the bytes of the uncached tree call."""
    from test_gpu_clm_cache import _trunk
    _, cfg, st, rd, _ = phi3_state("wide")
    dims = R.phi3_dims(cfg)
    arrays = R.phi3_device_layout(st, dims, R.phi3_rope(cfg))
    plain = _tiny("wide", "float16")[0]
    for setting in SETTINGS:
        sc = R.Phi3Scorer(dims, arrays, "cuda", context_cache_tokens=128)
        rng = np.random.default_rng(7)
        ctx, held = [2] + [int(x) for x in rng.integers(4, rd["vocab"], 40)], 0     # held: positions the cache holds
        for k in range(3):
            lst = [ctx + [int(x) for x in rng.integers(4, rd["vocab"], int(n))] for n in (5, 19, 3, 11)]
            with _trunk(setting):
                got = sc.token_logprobs(lst)
            assert _same(got, plain.token_logprobs(lst, share_prefixes=True)), (setting, k)
            assert sc.last_stats["reused"] == max(held - 1, 0) and sc.cache_len >= len(ctx)
            ctx, held = lst[0], sc.cache_len
        assert sc.last_stats["reused"] >= 32


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorer_surface_on_the_gpu(tmp_path):
    import torch
    model, cfg = tiny_phi3("partial", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto")
    assert isinstance(sc, R.Phi3Scorer) and sc.dtype is torch.bfloat16 and sc._family == "phi3"
    sbf = R.build_scorer(str(tmp_path), device="cuda", dtype="bfloat16")
    s16 = R.build_scorer(str(tmp_path), device="cuda")
    assert isinstance(s16, R.Phi3Scorer) and s16.dtype is torch.float16 and sbf.dtype is torch.bfloat16
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
