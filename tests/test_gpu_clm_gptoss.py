"""b2t_clm_gptoss_score_f16 / _tree_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_gptoss.hip, csrc/clm_gptoss.h) on the MI355X, driven
through the C ABI: against the float64 restatement of the contract (ref_logp_gptoss of tests/test_clm_gptoss_host.py, on the GPU
here) in both formats, the edges of the sliding window, the sinks, the tree path with the window inside the shared trunk, the
shapes where the grouping can go wrong, the clamps, one layer at the gpt-oss-20b widths, the bit identities and the Python
surface.

The comparison is tests/test_gpu_clm_mixtral.py's: the flat call writes the experts it chose (route_out) and the rounded
restatement is run with those routes forced.  The log-probs must then be within the project's bound -- fp16 min(3 x e16, 1e-2),
bf16 3 x e_bf16 after e_bf16 <= 0.1, e being what the contract's roundings alone do (restatement against restatement, never the
kernels).  Where the kernel's choice differs from the forced restatement's own free choice, the restatement's logits of the
experts exchanged must be within 3 x e_router of each other, and that may happen in at most max(1 %, 3 x share_ref) of the
(layer, row) pairs, share_ref being the share that the rounded restatement itself routes unlike the unrounded one.

Every call (_call) gets a fresh workspace of exactly the size the library asks for, filled with 0xFF, with canaries behind it,
behind both outputs and behind route_out.  The measured ratios are in NOTES.md ("LLM")."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_gptoss_host import (E_BF16_MAX, ROUTER_SCALE, gptoss_config, gptoss_figures, mxfp4_state, random_state, ref_logp_gptoss,
                                  tiny_gptoss, _planted_clamp)
from test_clm_llama_host import state_of, tiny_seqs
from test_clm_mixtral_host import contract_seqs
from test_gpu_clm_llama import GOLD, _pack, _prod_list, _same, _tiles
from test_gpu_clm_tree import _ListDecoder

pytestmark = pytest.mark.gpu


def _call(sc, seqs, tree=False, mode=None, with_tok=True, routes=False, finite=True):
    """(scores, per-sequence token log-probs[, route_out as [n_layers][rows][top_k]]) of one gpt-oss C ABI call in the scorer's
    dtype."""
    import torch
    import b2t_native as N
    lib = N.load()
    assert sc._family == "gptoss"
    sfx = "bf16" if sc.dtype is torch.bfloat16 else "f16"
    ids, off = _pack(seqs)
    M, S, CAN = int(off[-1]), len(seqs), 4096
    o = sc._oss
    oss = N.ClmGptOss(o.head_dim, o.swiglu_limit, o.n_experts, o.top_k, o.gate_up_stride, o.down_stride, None, o.layers_host)
    rows = R.tree_plan(ids, off)[2] if tree else M
    if tree:
        need = lib.b2t_clm_gptoss_tree_ws_bytes(C.byref(sc.desc), C.byref(oss), rows, M, S)
    else:
        need = lib.b2t_clm_gptoss_ws_bytes(C.byref(sc.desc), C.byref(oss), M, S)
    assert need > 0
    nr = sc.dims["n_layers"] * rows * oss.top_k
    rout = torch.full((nr + 64,), -7, dtype=torch.int32, device="cuda")
    if routes:
        oss.route_out = rout.data_ptr()
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
            rc = getattr(lib, "b2t_clm_gptoss_score_tree_" + sfx)(C.byref(sc.desc), C.byref(oss), ids.ctypes.data, off.ctypes.data,
                                                                  S, scores.data_ptr(), tok.data_ptr() if with_tok else None,
                                                                  C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == rows
        else:
            rc = getattr(lib, "b2t_clm_gptoss_score_" + sfx)(C.byref(sc.desc), C.byref(oss), ids.ctypes.data, off.ctypes.data, S,
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
        r = rout[:nr].cpu().numpy().reshape(sc.dims["n_layers"], rows, oss.top_k)
        assert (r >= 0).all() and (r < oss.n_experts).all()
        assert all(len(set(x)) == oss.top_k for x in r.reshape(-1, oss.top_k)), "an expert chosen twice for one row"
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
    dims = R.gptoss_dims(cfg)
    return R.GptOssScorer(dims, R.gptoss_device_layout(st, dims, R.gptoss_rope(cfg), dtype=fmt), "cuda", dtype=fmt)


_MODELS = {}


def _model(fmt="float16", change=None, n_layers=2, seed=0, router_scale=ROUTER_SCALE, **over):
    """(scorer in fmt, GPU state dict, dims, rope, config) of random_state for TINY with `over`, fmt-valued weights, cached;
    `change` (a name and a function) edits the state dict first.  router_scale = 1 (the grouping tests) makes the rows' routes
    as varied as the experts allow: the router's bias then no longer outweighs its weights, more pairs are routed unlike the
    unrounded restatement, and the allowance max(1 %, 3 share_ref) follows."""
    key = (fmt, change[0] if change else None, n_layers, seed, router_scale, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _MODELS:
        cfg = gptoss_config(n_layers, **over)[1]
        st = random_state(cfg, fmt, seed, router_scale, device="cuda")
        if change:
            st = change[1](st)
        _MODELS[key] = (_scorer(st, cfg, fmt), st, R.gptoss_dims(cfg), R.gptoss_rope(cfg), cfg)
    return _MODELS[key]


def _bound(fmt, e):
    if fmt == "float16":
        assert e > 0
        return min(3 * e, 1e-2)
    assert 0 < e <= E_BF16_MAX, e
    return 3 * e


def _against_the_forced_restatement(what, sc, st, rd, rope, seqs, fmt, modes=(None,), opts=()):
    """The flat call's log-probs against the rounded restatement forced to the call's routes, and the call's routes against that
    restatement's free choice (the module's docstring); then every mode in `modes` and the tree call give the same bytes.
    Returns (routes, the flat call's (scores, log-probs))."""
    s0, got, routes = _call(sc, seqs, False, modes[0], routes=True)
    e, e_router, share_ref, _, _ = gptoss_figures(st, rd, rope, seqs, fmt)
    ref, lg, free, _ = ref_logp_gptoss(st, rd, rope, seqs, fmt, routes=routes, opts=opts)
    g, ref = np.concatenate(got), np.concatenate(ref)
    err = float(np.abs(g - ref).max())
    differ = routes != free                                            # [layers][rows][k]
    pick = lambda ids: np.take_along_axis(lg, ids, -1)
    gaps = np.abs(pick(routes) - pick(free))[differ]
    pairs = float(differ.any(-1).mean())
    gmax = float(gaps.max()) if gaps.size else 0.0
    gap_r = gmax / e_router if e_router > 0 else (0.0 if gmax == 0 else float("inf"))     # a router without weights has e_router 0
    print(f"CLM gptoss {what} {fmt}: tokens {len(g)} max |dlogp| {err:.3e}  e {e:.3e}  ratio {err / e:.3f}  e_router {e_router:.3e}  "
          f"share_ref {share_ref:.4f}  pairs routed differently {int(differ.any(-1).sum())} of {differ.any(-1).size} ({pairs:.4f}), "
          f"largest gap among them {gap_r:.3f} e_router")
    assert err <= _bound(fmt, e), (what, err, e)
    assert not gaps.size or gaps.max() <= 3 * e_router, (what, gaps.max(), e_router)
    assert pairs <= max(0.01, 3 * share_ref), (what, pairs, share_ref)
    for mode in modes:
        for tree in (False, True):
            if (mode, tree) != (modes[0], False):
                s, t = _call(sc, seqs, tree, mode)
                assert s.tobytes() == s0.tobytes() and _same(t, got), (what, mode, tree)
    return routes, (s0, got)


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_tiny_model_against_the_contract(fmt):
    """d 192, 4 / 2 heads of 64, F 64 (expert strides 256 against 2F = 128 and d = 192), 8 experts top-4, layer 0 sliding at W = 40
    and layer 1 full, 418 rows with shared prefixes and a duplicate: within the bound of the forced restatement; tree and
    B2T_CLM_GEMM_256 = 0 / 2 give the same bytes."""
    sc, st, rd, rope, cfg = _model(fmt, sliding_window=40)
    assert rd["windows"] == [40, 0]
    seqs = contract_seqs(rd["vocab"])
    routes, _ = _against_the_forced_restatement("contract", sc, st, rd, rope, seqs, fmt, modes=(None, "0", "2"))
    assert routes.shape == (2, 418, 4) and len({tuple(r) for r in routes.reshape(-1, 4)}) > 1


# ---- the window ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 31, 32, 33, 128])
def test_window_edges(W):
    """One sliding layer of window W, sequences of W - 1, W, W + 1, W + 33 and 300 tokens in one batch: the first masked key, the
    first skipped block and a window that is a whole number of blocks or one key more or less."""
    sc, st, rd, rope, _ = _model(n_layers=1, sliding_window=W, layer_types=["sliding_attention"])
    assert rd["windows"] == [W]
    lens = [n for n in (W - 1, W, W + 1, W + 33, 300) if n > 0]
    seqs = tiny_seqs(rd["vocab"], seed=W, lens=lens)
    _against_the_forced_restatement(f"window {W}", sc, st, rd, rope, seqs, "float16", modes=(None,))


def test_window_at_least_the_sequence_is_full_attention():
    """The same weights with sliding layers of W = 300 >= the longest sequence and with full layers give the same bytes; a
    window of 150 changes the 300-token sequence alone."""
    seqs = tiny_seqs(300, seed=5, lens=(300, 129, 33))
    outs = {}
    for name, over in (("full", dict(layer_types=["full_attention"] * 2)), ("300", dict(sliding_window=300, layer_types=["sliding_attention"] * 2)),
                       ("150", dict(sliding_window=150, layer_types=["sliding_attention"] * 2))):
        sc = _model(**over)[0]
        outs[name] = _flat_and_tree(sc, seqs)
    assert outs["full"][0].tobytes() == outs["300"][0].tobytes() and _same(outs["full"][1], outs["300"][1])
    assert _same(outs["150"][1][1:], outs["full"][1][1:]) and outs["150"][1][0][:151].tobytes() == outs["full"][1][0][:151].tobytes()
    assert np.abs(outs["150"][1][0][151:] - outs["full"][1][0][151:]).max() > 1e-2


def test_blocks_in_front_of_the_window_are_not_read():
    """One sliding layer of W = 32 and a first token whose embedding row is Inf, so that its q, k and v are NaN.  A query at
    position i >= 64 starts its key loop at block (i & ~31) / 32 - 1 >= 1 and never meets key 0: its log-prob is finite and, in a
    one-layer model, byte for byte that of the same sequence behind a sound first token.  Queries that still run block 0 meet
    0 x NaN in P.V and are NaN, masked or not: skipping a block is not the same as masking it for operands that are not finite."""
    def inf_row(st):
        k = "model.embed_tokens.weight"
        w = st[k].clone()
        w[5] = float("inf")
        return dict(st, **{k: w})
    over = dict(n_layers=1, sliding_window=32, layer_types=["sliding_attention"])
    bad, good = _model(change=("Inf row", inf_row), **over)[0], _model(**over)[0]
    tail = [int(t) if t != 5 else 6 for t in tiny_seqs(300, seed=21, lens=(200,))[0][1:]]     # token 5 is the planted row
    for tree in (False, True):
        _, (t_bad,) = _call(bad, [[5] + tail], tree, finite=False)
        _, (t_good,) = _call(good, [[2] + tail], tree)
        assert np.isnan(t_bad[1:33]).all()                       # these queries see key 0
        assert np.isfinite(t_bad[65:]).all() and t_bad[65:].tobytes() == t_good[65:].tobytes(), tree


# ---- the sinks -------------------------------------------------------------------------------------------------------------
def _sinks(value):
    import torch
    return (f"sinks {value}", lambda st: {k: (torch.full_like(v, value) if k.endswith("sinks") else v) for k, v in st.items()})


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_sinks_at_the_extremes(fmt):
    """Sinks of +30 (the attention output is nearly 0) and of -1e4 (a plain softmax) are held to the contract, and -1e4 equals,
    to the bound, the restatement without a sink."""
    seqs = tiny_seqs(300, seed=6, lens=(1, 17, 64, 65, 100))
    sc, st, rd, rope, _ = _model(fmt, change=_sinks(30.0), sliding_window=40)
    _against_the_forced_restatement("sinks +30", sc, st, rd, rope, seqs, fmt)
    sc, st, rd, rope, _ = _model(fmt, change=_sinks(-1e4), sliding_window=40)
    routes, (_, got) = _against_the_forced_restatement("sinks -1e4", sc, st, rd, rope, seqs, fmt)
    e = gptoss_figures(st, rd, rope, seqs, fmt)[0]
    plain = ref_logp_gptoss(st, rd, rope, seqs, fmt, routes=routes, opts=("no_sink",))[0]
    err = float(np.abs(np.concatenate(got) - np.concatenate(plain)).max())
    print(f"CLM gptoss sinks -1e4 against the restatement without a sink {fmt}: {err:.3e} ratio {err / e:.3f}")
    assert err <= _bound(fmt, e)


# ---- the tree -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_tree_with_the_window_inside_the_trunk(fmt):
    """Candidates behind a shared prefix: of 100 tokens (the window of 40 cuts inside the shared trunk), and of 31, 32, 33, 39, 40
    and 41 tokens, so that the first owned position sits on either side of a block boundary and of the window; duplicates and a
    lone sequence.  All byte-identical to the flat call; the 100-token case is held to the contract."""
    sc, st, rd, rope, _ = _model(fmt, sliding_window=40)
    V = rd["vocab"]
    rng = np.random.default_rng(11)
    for n_ctx in (100, 31, 32, 33, 39, 40, 41):
        ctx = [2] + [int(x) for x in rng.integers(4, V, n_ctx - 1)]
        seqs = [ctx + [int(x) for x in rng.integers(4, V, int(n))] for n in (1, 5, 9, 30, 64)]
        seqs += [list(seqs[1]), ctx + seqs[3][n_ctx:n_ctx + 10]]                  # a duplicate, and a prefix of a candidate
        ids, off = _pack(seqs)
        assert R.tree_plan(ids, off)[2] < len(ids) - 4 * (n_ctx - 1)
        if n_ctx == 100:
            _against_the_forced_restatement("tree behind 100 shared tokens", sc, st, rd, rope, seqs, fmt)
        else:
            _flat_and_tree(sc, seqs)
    _flat_and_tree(sc, [tiny_seqs(V, seed=2, lens=(150,))[0]])
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])                                 # one-token sequences: no head rows


# ---- the shapes where the grouping can go wrong ---------------------------------------------------------------------------------
def test_thirty_two_experts_three_rows_leave_most_segments_empty():
    """One 3-token sequence over 32 experts, top-4: at most 12 experts get a row, so at least 20 segments are empty."""
    sc, st, rd, rope, _ = _model(num_local_experts=32, router_scale=1.0)
    routes, _ = _against_the_forced_restatement("32 experts, 3 rows", sc, st, rd, rope, [[2, 17, 250]], "float16", modes=(None, "0", "2"))
    for l in range(2):
        assert len(set(routes[l].reshape(-1))) <= 12


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_128_experts(fmt):
    """128 experts, top-4, 228 rows: both halves of the router's lanes, 128 segments of which most hold a few rows."""
    sc, st, rd, rope, _ = _model(fmt, num_local_experts=128, router_scale=1.0)
    seqs = tiny_seqs(rd["vocab"], seed=6, lens=(33, 65, 130))
    routes, _ = _against_the_forced_restatement("128 experts", sc, st, rd, rope, seqs, fmt, modes=(None, "2"))
    assert routes.shape == (2, 228, 4) and (routes >= 64).any() and (routes < 64).any() and len(set(routes.reshape(-1))) > 40


def test_top_k_is_every_expert():
    """8 experts, top-8: every segment holds every row."""
    sc, st, rd, rope, _ = _model(num_experts_per_tok=8)
    seqs = tiny_seqs(rd["vocab"], seed=4, lens=(129, 64, 100, 7))
    routes, _ = _against_the_forced_restatement("top-8 of 8, 300 rows", sc, st, rd, rope, seqs, "float16", modes=(None, "0", "2"))
    assert (np.sort(routes, -1) == np.arange(8)).all()


def test_bias_alone_decides_and_ties_go_to_the_lower_index():
    """Router weights zero: the logits are the bias, so every row's routes are the bias's top-k in order; equal biases go to the
    lower index, a pair of equal entries at ids 63 and 64 (the two halves of the router's lanes) included."""
    import torch

    def planted(st):
        out = dict(st)
        for l in range(2):
            out[f"model.layers.{l}.mlp.router.weight"] = torch.zeros_like(st[f"model.layers.{l}.mlp.router.weight"])
            b = st[f"model.layers.{l}.mlp.router.bias"].clone().clamp(-1.0, 1.0)
            b[63] = b[64] = 3.0          # the largest, twice
            b[100] = b[7] = 2.0          # then another pair
            out[f"model.layers.{l}.mlp.router.bias"] = b
        return out
    sc, st, rd, rope, _ = _model(change=("bias decides", planted), num_local_experts=128)
    seqs = tiny_seqs(rd["vocab"], seed=9, lens=(17, 64, 129))
    _, _, routes = _call(sc, seqs, False, routes=True)
    assert (routes == [63, 64, 7, 100]).all()
    _against_the_forced_restatement("bias decides", sc, st, rd, rope, seqs, "float16")


def test_combine_is_in_order_of_choice():
    """bfloat16, router weights zero and biases that make every row choose [5, 6, 2, 1] with equal weights for 5 and 6, whose
    down biases are +2^100 and -2^100 (either absorbs an expert's own output in fp32 as in float64): in order of choice the two cancel exactly before experts 2 and 1 are added, and the result is
    the restatement's; in expert order (1, 2, 5, 6) the sum of experts 1 and 2 would be absorbed by 2^100 and lost."""
    import torch

    def planted(st):
        out = dict(st)
        for l in range(2):
            p = f"model.layers.{l}.mlp."
            out[p + "router.weight"] = torch.zeros_like(st[p + "router.weight"])
            b = torch.full_like(st[p + "router.bias"], -4.0)
            b[5], b[6], b[2], b[1] = 3.0, 3.0, 2.0, 1.0
            out[p + "router.bias"] = b
            db = st[p + "experts.down_proj_bias"].clone()
            db[5], db[6] = 2.0 ** 100, -2.0 ** 100
            out[p + "experts.down_proj_bias"] = db
        return out
    sc, st, rd, rope, _ = _model("bfloat16", change=("order of choice", planted))
    seqs = tiny_seqs(rd["vocab"], seed=9, lens=(17, 64, 129))
    routes, _ = _against_the_forced_restatement("order of choice", sc, st, rd, rope, seqs, "bfloat16", modes=(None, "2"))
    assert (routes == [5, 6, 2, 1]).all()
    swapped = ref_logp_gptoss(st, rd, rope, seqs, "bfloat16", routes=routes[..., [3, 2, 0, 1]])[0]
    exact = ref_logp_gptoss(st, rd, rope, seqs, "bfloat16", routes=routes)[0]
    assert max(np.abs(a - b).max() for a, b in zip(swapped, exact)) > 0.1     # the order is visible in this model


def test_nan_logits_stay_out_of_the_addresses():
    """A router bias of NaNs in layer 0: the routes are distinct and in range (_call checks), the canaries stay, the NaN shows
    in the scores."""
    import torch

    def nan_router(st):
        k = "model.layers.0.mlp.router.bias"
        return dict(st, **{k: torch.full_like(st[k], float("nan"))})
    for ne in (8, 128):
        sc, _, rd, _, _ = _model(change=("NaN router", nan_router), num_local_experts=ne)
        seqs = tiny_seqs(rd["vocab"], seed=2, lens=(5, 40))
        s, t, routes = _call(sc, seqs, False, routes=True, finite=False)
        assert np.isnan(s).all()
        s2, t2 = _call(sc, seqs, True, finite=False)
        assert np.isnan(s2).all()


# ---- the clamps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_clamped_activations(fmt):
    """Expert biases planted so that more than 10 % of the gates and of the ups hit the limit (measured in the restatement): held
    to the contract, and away from the restatement without the clamp."""
    sc, st, rd, rope, _ = _model(fmt, change=("planted clamp", _planted_clamp), sliding_window=40)
    seqs = tiny_seqs(rd["vocab"], seed=3, lens=(17, 33, 100))
    routes, (_, got) = _against_the_forced_restatement("clamps", sc, st, rd, rope, seqs, fmt, modes=(None, "2"))
    ref, _, _, (sg, su) = ref_logp_gptoss(st, rd, rope, seqs, fmt, routes=routes)
    assert sg > 0.1 and su > 0.1, (sg, su)
    unclamped = ref_logp_gptoss(st, rd, rope, seqs, fmt, routes=routes, opts=("no_clamp",))[0]
    e = gptoss_figures(st, rd, rope, seqs, fmt)[0]
    assert np.abs(np.concatenate(got) - np.concatenate(unclamped)).max() > 10 * _bound(fmt, e)


# ---- one layer at the gpt-oss-20b widths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_one_full_width_layer_on_both_tiles(fmt):
    """d 2880, 64 / 8 heads of 64, F 2880, 32 experts top-4, one sliding layer of 128, vocab 515, 302 rows: d and F are 45 k tiles
    and 11.25 tiles of 256, the gate / up GEMM has N = 5760, on both tiles."""
    sc, st, rd, rope, _ = _model(fmt, n_layers=1, hidden_size=2880, num_attention_heads=64, num_key_value_heads=8, intermediate_size=2880,
                                 num_local_experts=32, sliding_window=128, layer_types=["sliding_attention"], vocab_size=515, router_scale=1.0)
    seqs = tiny_seqs(rd["vocab"], seed=12, lens=(160, 65, 33, 31, 13))
    assert sum(map(len, seqs)) == 302
    routes, _ = _against_the_forced_restatement("full width", sc, st, rd, rope, seqs, fmt, modes=("0", "2"))
    assert len(set(routes.reshape(-1))) > 16
    _MODELS.clear()     # gigabytes


# ---- bit identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_score_alone_equals_score_in_a_batch(fmt):
    sc, _, rd, _, _ = _model(fmt, sliding_window=16)
    V = rd["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=99)
    s0, t0 = _call(sc, [probe], False)
    for pos in (0, 50, 99):
        batch = others[:pos] + [probe] + others[pos:]
        assert len(batch) == 100
        for tree in (False, True):
            s, t = _call(sc, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(sc, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorer_surface_plain_and_mxfp4(tmp_path):
    """build_scorer on a saved tiny checkpoint in the plain spelling and on the same model in the MXFP4 spelling (the expert
    matrices first made MXFP4-representable): the same bytes; dtype auto / default; last_stats; the length penalty; the cache
    refusal."""
    import torch
    from safetensors.torch import save_file
    model, cfg = tiny_gptoss(fmt="bfloat16")
    plain, packed = mxfp4_state(state_of(model, False))
    model.load_state_dict(plain)
    model.to(torch.bfloat16).save_pretrained(str(tmp_path / "plain"))
    os.makedirs(tmp_path / "mxfp4")
    with open(tmp_path / "mxfp4" / "config.json", "w") as f:
        json.dump(cfg | {"dtype": "bfloat16"}, f)
    save_file({k: (v if v.dtype == torch.uint8 else v.to(torch.bfloat16)).contiguous() for k, v in packed.items()},
              str(tmp_path / "mxfp4" / "model.safetensors"))
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    sc = R.build_scorer(str(tmp_path / "plain"), device="cuda", dtype="auto")
    assert isinstance(sc, R.GptOssScorer) and sc.dtype is torch.bfloat16 and sc._family == "gptoss"
    s16 = R.build_scorer(str(tmp_path / "plain"), device="cuda")
    assert isinstance(s16, R.GptOssScorer) and s16.dtype is torch.float16
    for scorer in (sc, s16):
        s, t = _call(scorer, seqs, False)
        for tree in (False, True):
            assert _same(scorer.token_logprobs(seqs, share_prefixes=tree), t)
            assert scorer.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
            assert scorer.score(seqs, 0.25, share_prefixes=tree).tobytes() == \
                (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    assert not _same(sc.token_logprobs(seqs), s16.token_logprobs(seqs))       # two formats, two functions
    for dt, twin in (("auto", sc), (None, s16)):
        mx = R.build_scorer(str(tmp_path / "mxfp4"), device="cuda", dtype=dt)
        assert mx.dtype is twin.dtype and _same(mx.token_logprobs(seqs), twin.token_logprobs(seqs))
    with pytest.raises(ValueError, match="context cache"):
        R.build_scorer(str(tmp_path / "plain"), device="cuda", context_cache_tokens=64)
    with pytest.raises(RuntimeError, match="b2t_clm_gptoss_score_bf16.*max_pos"):
        sc.score([[2] * 513])


def test_service_end_to_end_with_a_gptoss_scorer(tmp_path):
    """LocalLMService with do_opt = 1 over three sentences with a growing context (far longer than the window of 16): a scorer
    with share_prefixes gives the replies, field by field, of one without."""
    import torch
    import evaluate_model_helpers as H
    from remote_lm import LocalLMService
    model, cfg = tiny_gptoss(fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(vocab_size=cfg["vocab_size"], bos_id=2, pad_id=1)
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies = {}
    for share in (False, True):
        sc = R.build_scorer(str(tmp_path), device="cuda", dtype="auto", share_prefixes=share)
        assert type(sc) is R.GptOssScorer
        ctx, replies[share] = "well then " * 12, []
        for nbest in lists:
            r = LocalLMService(_ListDecoder(nbest), acoustic_scale=0.3, alpha=0.5, nbest=100, decode_fn=lambda *a: None,
                               llm=(sc, tok), do_opt=1, top_candidates_to_augment=20)
            r.set("contextual_decoding_current_context", ctx)
            t0 = H.get_current_redis_time_ms(r)
            H.reset_remote_language_model(r, t0)
            r.xadd("remote_lm_finalize", {"done": 0})
            reply = r.streams["remote_lm_output_final"][-1][1]
            replies[share].append(reply)
            ctx = ctx + " " + reply[b"lm_response_final"].decode()
        assert sc.last_stats["tokens"] > 20 * 24 and (sc.last_stats["nodes"] < sc.last_stats["tokens"]) == share
    for a, b in zip(replies[False], replies[True]):
        assert set(a) == set(b) and b"scoring" in a and a[b"lm_response_final"]
        for k in a:
            assert a[k] == b[k], k
