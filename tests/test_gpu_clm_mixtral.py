"""b2t_clm_mixtral_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_mixtral.hip, csrc/clm_moe.h) on
the MI355X, driven through the C ABI: against the float64 restatement of the contract (ref_logp_mixtral_fmt of
tests/test_clm_mixtral_host.py, on the GPU here) in both formats, the bit identities (tree = flat = cached, the forced tile
modes, alone = in a batch, a growing context), the shapes where the grouping can go wrong, and the Python surface.

How a kernel whose router makes discrete choices is compared with a restatement: the flat call writes the experts it chose
(b2t_clm_moe_t.route_out), and the rounded restatement is run with those routes forced, its weights still computed from its
own logits.  The log-probs must then be within the project's bound -- fp16 min(3 x e16, 1e-2), bf16 3 x e_bf16 after
e_bf16 <= 0.1, e being what the contract's roundings alone do to the log-probs of the case (restatement against restatement on
the unrounded restatement's routes, never the kernels).  Where the kernel's choice differs from the forced restatement's own
free choice, the restatement's logits of the two experts exchanged at that place must be within 3 x e_router of each other,
e_router being the largest difference between the rounded and the unrounded restatement's router logits.

Conventions as in tests/test_gpu_clm_olmo2.py: every call (_call) gets a fresh workspace of exactly the size the library asks
for, filled with 0xFF, with canaries behind it, behind both outputs and behind route_out.  The measured ratios are in NOTES.md
("LLM")."""
import ctypes as C

import numpy as np
import pytest

import llm_rescore as R
from test_clm_cache_host import dict_rule  # noqa: F401  (Rig uses it)
from test_clm_llama_host import hf_inv_freq, state_of, tiny_seqs
from test_clm_mixtral_host import (E_BF16_MAX, SEED, contract_seqs, fused_state, mixtral_ref_dims, ref_logp_mixtral_fmt,
                                   router_figures, tiny_mixtral)
from test_gpu_clm_cache import SETTINGS, _same_bytes
from test_gpu_clm_llama import _pack, _prod_list, _same, _tiles
from test_gpu_clm_llama_cache import FamilyLib, Rig

pytestmark = pytest.mark.gpu


def _call(sc, seqs, tree=False, mode=None, with_tok=True, routes=False, finite=True):
    """(scores, per-sequence token log-probs[, route_out as [n_layers][rows][top_k]]) of one Mixtral C ABI call in the scorer's
    dtype."""
    import torch
    import b2t_native as N
    lib = N.load()
    assert sc._family == "mixtral"
    sfx = "bf16" if sc.dtype is torch.bfloat16 else "f16"
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    moe = N.ClmMoe(sc._moe.n_experts, sc._moe.top_k, sc._moe.router_w_host, sc._moe.gate_up_stride, sc._moe.down_stride, None)
    rows = R.tree_plan(ids, off)[2] if tree else M
    if tree:
        need = lib.b2t_clm_mixtral_tree_ws_bytes(C.byref(sc.desc), C.byref(moe), rows, M, S)
    else:
        need = lib.b2t_clm_mixtral_ws_bytes(C.byref(sc.desc), C.byref(moe), M, S)
    assert need > 0
    nr = sc.dims["n_layers"] * rows * moe.top_k
    rout = torch.full((nr + 64,), -7, dtype=torch.int32, device="cuda")
    if routes:
        moe.route_out = rout.data_ptr()
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
            rc = getattr(lib, "b2t_clm_mixtral_score_tree_" + sfx)(C.byref(sc.desc), C.byref(moe), ids.ctypes.data, off.ctypes.data,
                                                                   S, scores.data_ptr(), tok.data_ptr() if with_tok else None,
                                                                   C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == rows
        else:
            rc = getattr(lib, "b2t_clm_mixtral_score_" + sfx)(C.byref(sc.desc), C.byref(moe), ids.ctypes.data, off.ctypes.data, S,
                                                              scores.data_ptr(), tok.data_ptr() if with_tok else None,
                                                              ws.data_ptr(), need, stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], canary), "wrote behind the workspace"
    assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all() and (rout[nr:] == -7).all()
    s, t = scores[:S].cpu().numpy(), tok[:M].cpu().numpy()
    if finite:
        assert np.isfinite(s).all() and np.isfinite(t).all(), "non-finite output"
    del ws
    out = (s, [t[off[i]:off[i + 1]] for i in range(S)])
    if routes:
        r = rout[:nr].cpu().numpy().reshape(sc.dims["n_layers"], rows, moe.top_k)
        assert (r >= 0).all() and (r < moe.n_experts).all()
        assert all(len(set(x)) == moe.top_k for x in r.reshape(-1, moe.top_k)), "an expert chosen twice for one row"
        return out + (r,)
    assert (rout == -7).all()
    return out


def _flat_and_tree(sc, seqs, mode=None):
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


def _scorer(st, cfg, fmt):
    dims = R.mixtral_dims(cfg)
    return R.MixtralScorer(dims, R.mixtral_device_layout(st, dims, R.rope_inv_freq(cfg), dtype=fmt), "cuda", dtype=fmt)


_MODELS = {}


def _model(fmt="float16", change=None, **over):
    """(scorer in fmt, GPU state dict in the fused spelling, reference dims, inv_freq, config) of tiny_mixtral(**over) with
    fmt-valued weights, cached; `change` (a name and a function) edits the state dict first."""
    key = (fmt, change[0] if change else None, tuple(sorted(over.items())))
    if key not in _MODELS:
        model, cfg = tiny_mixtral(fmt=fmt, seed=over.pop("seed", SEED[fmt]), **over)
        st = fused_state(state_of(model, cfg["tie_word_embeddings"]), cfg)
        if change:
            st = change[1](st)
        _MODELS[key] = (_scorer(st, cfg, fmt), {k: v.cuda() for k, v in st.items()}, mixtral_ref_dims(cfg), hf_inv_freq(model), cfg)
    return _MODELS[key]


def _bound(fmt, e):
    if fmt == "float16":
        assert e > 0
        return min(3 * e, 1e-2)
    assert 0 < e <= E_BF16_MAX, e
    return 3 * e


def _against_the_forced_restatement(what, sc, st, rd, inv, seqs, fmt, modes=(None,), max_share=None):
    """The flat call's log-probs against the rounded restatement forced to the call's routes, and the call's routes against
    that restatement's free choice (the module's docstring); then every mode in `modes` and the tree call give the same bytes.
    Returns (routes, share of (layer, row) pairs where kernel and restatement choose differently)."""
    s0, got, routes = _call(sc, seqs, False, modes[0], routes=True)
    _, _, e, e_router, share, _, _, _ = router_figures(st, rd, inv, seqs, fmt)
    ref, lg, free = ref_logp_mixtral_fmt(st, rd, inv, seqs, fmt, routes=routes)
    g, ref = np.concatenate(got), np.concatenate(ref)
    err = float(np.abs(g - ref).max())
    differ = routes != free                                            # [layers][rows][k]
    pick = lambda ids: np.take_along_axis(lg, ids, -1)
    gaps = np.abs(pick(routes) - pick(free))[differ]
    pairs = float(differ.any(-1).mean())
    print(f"CLM mixtral {what} {fmt}: tokens {len(g)} max |dlogp| {err:.3e}  e {e:.3e}  ratio {err / e:.3f}  e_router {e_router:.3e}  "
          f"pairs routed differently {int(differ.any(-1).sum())} of {differ.any(-1).size} ({pairs:.4f}), largest gap among them "
          f"{gaps.max() if gaps.size else 0.0:.3e} = {(gaps.max() if gaps.size else 0.0) / e_router:.3f} e_router")
    assert err <= _bound(fmt, e), (what, err, e)
    assert not gaps.size or gaps.max() <= 3 * e_router, (what, gaps.max(), e_router)
    if max_share is not None:
        assert pairs <= max_share, (what, pairs)
    for mode in modes:
        for tree in (False, True):
            if (mode, tree) != (modes[0], False):
                s, t = _call(sc, seqs, tree, mode)
                assert s.tobytes() == s0.tobytes() and _same(t, got), (what, mode, tree)
    return routes, pairs


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_tiny_model_against_the_contract(fmt):
    """d 128, F 192 (expert strides 512 and 256 rows against 2F = 384 and d = 128), 4 experts, top-2, 2 layers, 418 rows with
    shared prefixes and a duplicate: log-probs within the bound of the forced restatement, routes that differ from its free
    choice only across gaps of at most 3 e_router and in at most 1 % of the (layer, row) pairs; tree and B2T_CLM_GEMM_256 = 0 / 2
    give the same bytes.

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, st, rd, inv, cfg = _model(fmt)
    seqs = contract_seqs(rd["vocab"])
    routes, _ = _against_the_forced_restatement("contract", sc, st, rd, inv, seqs, fmt, modes=(None, "0", "2"), max_share=0.01)
    assert routes.shape == (2, 418, 2) and len({tuple(r) for r in routes.reshape(-1, 2)}) == 12   # every ordered pair of experts


# ---- the shapes where the grouping can go wrong ---------------------------------------------------------------------------------
def test_eight_experts_three_rows_leave_experts_without_a_row():
    """One 3-token sequence over 8 experts, top-2: at most 6 experts get a row, so at least two segments are empty and every
    other holds one or two rows in a block of 256."""
    sc, st, rd, inv, _ = _model(num_local_experts=8)
    routes, _ = _against_the_forced_restatement("8 experts, 3 rows", sc, st, rd, inv, [[2, 17, 250]], "float16", modes=(None, "0", "2"))
    for l in range(2):
        assert len(set(routes[l].reshape(-1))) <= 6


def test_two_experts_top_two_every_segment_is_every_row():
    """2 experts, top-2, 300 rows: both segments hold all 300 rows -- two 256-row blocks with a padded tail each."""
    sc, st, rd, inv, _ = _model(num_local_experts=2)
    seqs = tiny_seqs(rd["vocab"], seed=4, lens=(129, 64, 100, 7))
    assert sum(map(len, seqs)) == 300
    routes, _ = _against_the_forced_restatement("2 experts top-2, 300 rows", sc, st, rd, inv, seqs, "float16", modes=(None, "0", "2"))
    assert (np.sort(routes, -1) == [0, 1]).all() and len({tuple(r) for r in routes.reshape(-1, 2)}) == 2


def test_top_one_weight_is_exactly_one():
    """4 experts, top-1: the weight is exp(0) / exp(0) = 1, so the layer adds the chosen expert's output itself."""
    sc, st, rd, inv, _ = _model(num_experts_per_tok=1)
    seqs = tiny_seqs(rd["vocab"], seed=6, lens=(33, 65, 130))
    routes, _ = _against_the_forced_restatement("top-1", sc, st, rd, inv, seqs, "float16", modes=(None, "2"))
    assert routes.shape == (2, 228, 1) and len(set(routes.reshape(-1))) == 4


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_head_dim_128(fmt):
    sc, st, rd, inv, _ = _model(fmt, hidden_size=256, num_attention_heads=2, num_key_value_heads=2)
    assert rd["d_model"] // rd["n_heads"] == 128
    seqs = tiny_seqs(rd["vocab"], seed=7, lens=(1, 31, 64, 65))
    _against_the_forced_restatement("head dim 128", sc, st, rd, inv, seqs, fmt, modes=(None, "2"))


def test_identical_router_rows_never_give_the_higher_index_first():
    """Experts 1 and 3 with the same router row have the same logit bit for bit (one order of summation per row), and a tie
    goes to the lower index: 3 never appears without 1 chosen before it."""
    def same_rows(st):
        out = dict(st)
        for l in range(2):
            w = st[f"model.layers.{l}.mlp.gate.weight"].clone()
            w[3] = w[1]
            out[f"model.layers.{l}.mlp.gate.weight"] = w
        return out
    sc, st, rd, inv, _ = _model(change=("router rows 1 = 3", same_rows))
    seqs = tiny_seqs(rd["vocab"], seed=9, lens=(17, 64, 129))
    _, _, routes = _call(sc, seqs, False, routes=True)
    flat = routes.reshape(-1, 2)
    has3 = (flat == 3).any(-1)
    assert has3.any() and (flat[has3] == [1, 3]).all(), flat[has3][:5]
    assert (flat[:, 0] != 3).all()
    _flat_and_tree(sc, seqs)


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_one_full_width_layer_on_both_tiles(fmt):
    """d 512, F 448, 8 experts, top-2, one layer, 640 rows: 1280 entries in segments of one or two blocks, the gate / up GEMM
    with N = 896 and the down GEMM with K = 448 (7 k tiles) on both tiles, against the forced restatement."""
    sc, st, rd, inv, _ = _model(fmt, n_layers=1, hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=448,
                                num_local_experts=8)
    seqs = tiny_seqs(rd["vocab"], seed=12, lens=(129, 128, 127, 65, 64, 63, 33, 31))
    assert sum(map(len, seqs)) == 640
    routes, _ = _against_the_forced_restatement("full width", sc, st, rd, inv, seqs, fmt, modes=("0", "2", None))
    counts = np.bincount(routes.reshape(-1), minlength=8)
    assert counts.sum() == 1280 and (counts > 0).all()


def test_nan_logits_stay_out_of_the_addresses():
    """A router of NaNs in layer 0: every comparison is false, so every row takes experts 0 and 1; the NaN shows in the
    scores, the canaries stay."""
    import torch

    def nan_router(st):
        return dict(st, **{"model.layers.0.mlp.gate.weight": torch.full_like(st["model.layers.0.mlp.gate.weight"], float("nan"))})
    sc, _, rd, _, _ = _model(change=("NaN router", nan_router))
    seqs = tiny_seqs(rd["vocab"], seed=2, lens=(5, 40))
    s, t, routes = _call(sc, seqs, False, routes=True, finite=False)
    assert (routes[0] == [0, 1]).all() and np.isnan(s).all()


# ---- bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_score_alone_equals_score_in_a_batch(fmt):
    sc, _, rd, _, _ = _model(fmt)
    V = rd["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=60)
    s0, t0 = _call(sc, [probe], False)
    for pos in (0, 30, 60):
        batch = others[:pos] + [probe] + others[pos:]
        for tree in (False, True):
            s, t = _call(sc, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(sc, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])                               # one-token sequences: no head rows


def _rigs(sc, cap):
    rigs = [Rig(sc, cap, s) for s in SETTINGS]
    for rig in rigs:
        rig.lib = FamilyLib(rig.lib, sc, "mixtral")
    return rigs


def test_cached_session_of_three_growing_contexts():
    """Three 20-candidate lists behind a context of 30 tokens that grows by the first candidate of the call before: cached =
    tree = flat byte for byte, read-only and updating, B2T_CLM_TRUNK_ATTN 0 and 1, the tile rule changing from call to call; the
    scores across the cached calls are the flat call's."""
    import bench_llm_rescore as B
    sc, _, rd, _, _ = _model()
    V, max_pos = rd["vocab"], sc.dims["max_pos"]
    rigs = _rigs(sc, max_pos)
    rng = np.random.default_rng(V)
    ctx, prev = [int(x) for x in rng.integers(4, V, 30)], None
    for k, mode in enumerate(("0", None, "2")):
        seqs = B.nbest_list(rng, V, 20, ctx)
        assert max(map(len, seqs)) <= max_pos
        tree = _call(sc, seqs, True, mode)
        _same_bytes(_call(sc, seqs, False, mode), tree, f"call {k}: flat against tree")
        for rig in rigs:
            for update in (0, 1):
                s, t, plan = rig.call(seqs, mode, update)
                _same_bytes((s, t), tree, f"call {k}: cached (update {update}, trunk attention {rig.setting}) against tree")
            assert plan["trunk"] >= len(ctx) + 1
            if prev is not None:
                assert plan["common"] == prev and plan["reused"] == prev - 1 >= 30
            last = plan
        prev = last["n_after"]
        ctx = [int(x) for x in seqs[0][1:]]
    assert last["reused"] >= 32     # the third call reused a whole 32-key block


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorer_surface_on_the_gpu(tmp_path):
    import torch
    model, cfg = tiny_mixtral(fmt="bfloat16", seed=SEED["bfloat16"])
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto")
    assert isinstance(sc, R.MixtralScorer) and sc.dtype is torch.bfloat16 and sc._family == "mixtral"
    s16 = R.build_scorer(str(tmp_path), device="cuda")
    assert isinstance(s16, R.MixtralScorer) and s16.dtype is torch.float16
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
