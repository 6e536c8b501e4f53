"""b2t_clm_gptoss_mx_score_f16 / _tree_f16 / _bf16 / _tree_bf16 and b2t_clm_mxfp4_unpack_f16 / _bf16 (csrc/causal_lm_gptoss_mx.hip, the
packed form of the grouped tile in csrc/clm_gemm.h) on the MI355X.  The contract is not a tolerance: the calls on the experts
kept in MXFP4 give the BYTES -- scores, token log-probs, route_out -- of the b2t_clm_gptoss_* calls on the same checkpoint
expanded by the dense loader, flat and tree, fp16 and bf16, on both tiles.  The reference of every model test here is therefore
the dense scorer of the same state dict, which tests/test_gpu_clm_gptoss.py holds to the float64 restatement; the reference of the
unpack table is llm_rescore.mxfp4_dequant(...).to(dtype), the loader's own expansion.

The checkpoints are packed_state's (tests/test_clm_gptoss_mx_host.py): uniform random nibbles and scale bytes uniform in [110, 130]
per block, so that neighbouring blocks of a row and of a k tile differ; the host file checks that the restatement stays finite
on them.  Every call (_call, the rig of tests/test_gpu_clm_gptoss.py with the mx array added) gets a fresh workspace of exactly the
size the library asks for, filled with 0xFF, with canaries behind it and behind the outputs; the packed arrays of a scorer under
test are sub-views inside larger allocations filled with 0xFF (_guarded): a scale byte of 0xFF is NaN, so a read beyond a row's
or an array's end that reaches an MFMA shows in the bytes.

None of this runs without the feature: the symbols, the keyword and the scorer do not exist before it.  What each planted change
of the unpack or of the fetch fails is listed in NOTES.md ("LLM")."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_gptoss_host import gptoss_config
from test_clm_gptoss_mx_host import expert_bytes, packed_state, save_checkpoint
from test_clm_llama_host import tiny_seqs
from test_clm_mixtral_host import contract_seqs
from test_gpu_clm_llama import GOLD, _pack, _prod_list, _same, _tiles
from test_gpu_clm_tree import _ListDecoder

pytestmark = pytest.mark.gpu
GUARD = 4096


def _call(sc, seqs, tree=False, mode=None, with_tok=True):
    """(scores, per-sequence token log-probs, route_out [n_layers][rows][top_k]) of one C ABI call of a GptOssScorer (the dense
    entry points) or a GptOssMxScorer (the mx ones) in the scorer's dtype."""
    import torch
    import b2t_native as N
    lib = N.load()
    assert sc._family in ("gptoss", "gptoss_mx")
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
    oss.route_out = rout.data_ptr()
    canary = torch.randint(0, 256, (CAN,), dtype=torch.uint8, device="cuda")
    ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
    ws[:need] = 0xFF
    ws[need:] = canary
    scores = torch.full((S + 64,), 12345.0, device="cuda")
    tok = torch.full((M + 64,), 12345.0, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    extra = (sc._mx,) if sc._family == "gptoss_mx" else ()
    name = f"b2t_clm_{sc._family}_score_" + ("tree_" if tree else "") + sfx
    with _tiles(mode):
        if tree:
            nn = C.c_longlong(-1)
            rc = getattr(lib, name)(C.byref(sc.desc), C.byref(oss), *extra, ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                    tok.data_ptr() if with_tok else None, C.byref(nn), ws.data_ptr(), need, stream)
            assert rc != 0 or nn.value == rows
        else:
            rc = getattr(lib, name)(C.byref(sc.desc), C.byref(oss), *extra, ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                    tok.data_ptr() if with_tok else None, ws.data_ptr(), need, stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws[need:], canary), "wrote behind the workspace"
    assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all() and (rout[nr:] == -7).all()
    s, t = scores[:S].cpu().numpy(), tok[:M].cpu().numpy()
    assert np.isfinite(s).all() and np.isfinite(t).all(), "non-finite output"
    r = rout[:nr].cpu().numpy().reshape(sc.dims["n_layers"], rows, oss.top_k)
    assert (r >= 0).all() and (r < oss.n_experts).all()
    return s, [t[off[i]:off[i + 1]] for i in range(S)], r


def _guarded(sc):
    """Moves the scorer's packed arrays into the middle of larger allocations filled with 0xFF and points the mx array at them."""
    import torch
    sc._guards = []
    for k in [k for k in sc.w if k.endswith(sc._PACKED)]:
        t = sc.w[k]
        buf = torch.full((t.numel() + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        buf[GUARD:GUARD + t.numel()] = t.reshape(-1)
        sc.w[k] = buf[GUARD:GUARD + t.numel()].view(t.shape)
        sc._guards.append(buf)
    sc._point({})
    assert sc._mx[0].gate_up_s == sc.w["layers.0.gate_up_s"].data_ptr() == sc._guards[1].data_ptr() + GUARD
    return sc


_MODELS = {}


def _pair(fmt="float16", n_layers=2, seed=0, router_scale=0.125, **over):
    """(the dense scorer, the mx scorer with guarded arrays, dims) of packed_state for TINY with `over`, cached"""
    key = (fmt, n_layers, seed, router_scale, tuple(sorted((k, str(v)) for k, v in over.items())))
    if key not in _MODELS:
        cfg = gptoss_config(n_layers, **over)[1]
        st = packed_state(cfg, fmt, seed, router_scale, device="cuda")
        dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
        dense = R.GptOssScorer(dims, R.gptoss_device_layout(st, dims, rope, dtype=fmt), "cuda", dtype=fmt)
        mx = _guarded(R.GptOssMxScorer(dims, R.gptoss_mx_device_layout(st, dims, rope, dtype=fmt), "cuda", dtype=fmt))
        assert mx.expert_bytes() == n_layers * expert_bytes(dims) and not [k for k in mx.w if k.endswith(("gate_up_w", "down_w"))]
        _MODELS[key] = (dense, mx, dims)
    return _MODELS[key]


def _identical(what, dense, mx, seqs, modes=("0", "2")):
    """The dense flat call under the first mode is the reference; the mx calls, flat and tree, under every mode give its bytes in
    scores, token log-probs and (flat) route_out; the tree's route_out is the dense tree call's."""
    s0, t0, r0 = _call(dense, seqs, False, modes[0])
    _, _, rt0 = _call(dense, seqs, True, modes[0])
    assert len({tuple(x) for x in r0.reshape(-1, r0.shape[-1])}) > 1 or r0.shape[1] == 1
    for mode in modes:
        for tree in (False, True):
            s, t, r = _call(mx, seqs, tree, mode)
            assert s.tobytes() == s0.tobytes() and _same(t, t0), (what, mode, tree, float(np.abs(s - s0).max()))
            assert r.tobytes() == (rt0 if tree else r0).tobytes(), (what, mode, tree)
    print(f"CLM gptoss mx {what} {str(mx.dtype)[6:]}: {sum(map(len, seqs))} tokens, {r0.shape[1]} rows, experts in use "
          f"{len(set(r0.reshape(-1)))}, sum of scores {float(s0.sum()):.4f}: {2 * len(modes)} mx calls identical to the dense call")
    return s0, t0, r0


# ---- the unpack table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_unpack_table(fmt):
    """b2t_clm_mxfp4_unpack_* over all 16 codes x every scale byte whose 16 values are finite in the dtype, equal to
    mxfp4_dequant(...).to(dtype) bit for bit, the signs of zero included.  A row is one block of 32 nibbles (i + shift) % 16, one
    row per scale byte and shift, so every nibble position of a 4-byte piece sees every code under every scale byte.  fp16: scale
    bytes 102 to 104 put 0.5, 1.5 and 3 ulp of the subnormals on the rounding boundary, the bytes below 100 give signed zeros
    and 141 to 143 still have finite rows; bf16: every byte up to 252, the subnormals of bytes 0 and 1 included, is exact."""
    import torch
    import b2t_native as N
    lib = N.load()
    wdt = R.clm_dtype(fmt)
    code = (torch.arange(32)[None, :] + torch.arange(16)[:, None]) % 16                        # [shift][i]
    row = (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8)                               # [16][16 bytes], low nibble first
    blocks = row[None].expand(256, 16, 16).reshape(4096, 1, 16).contiguous()
    scales = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 16).reshape(4096, 1).contiguous()
    want = R.mxfp4_dequant(blocks, scales).to(wdt)                                             # [4096][32]
    ok = torch.isfinite(want.float()).reshape(256, -1).all(-1)
    n_ok = int(ok.sum())
    assert n_ok == {"float16": 141, "bfloat16": 253}[fmt] and bool(ok[:n_ok].all())             # 0 .. 140, 0 .. 252
    if fmt == "float16":
        sub = want.reshape(256, 16, 32)[103].float().abs()
        assert set(sub.unique().tolist()) == {u * 2.0 ** -24 for u in (0, 1, 2, 3, 4, 6)}          # 0.5 and 1.5 ulp went to even
    q = torch.full((blocks.numel() + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    s = torch.full((scales.numel() + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    q[GUARD:-GUARD], s[GUARD:-GUARD] = blocks.reshape(-1).cuda(), scales.reshape(-1).cuda()
    out = torch.full((4096 * 32 + 256,), -2, dtype=torch.int16, device="cuda")
    rc = getattr(lib, "b2t_clm_mxfp4_unpack_" + ("bf16" if fmt == "bfloat16" else "f16"))(
        q.data_ptr() + GUARD, s.data_ptr() + GUARD, 4096, 32, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert (out[4096 * 32:] == -2).all()
    got = out[:4096 * 32].cpu().reshape(256, 16 * 32)
    ref = want.view(torch.int16).reshape(256, 16 * 32)
    bad = [(b, int((got[b] != ref[b]).sum())) for b in range(n_ok) if not torch.equal(got[b], ref[b])]
    assert not bad, (fmt, "scale bytes with wrong bits (byte, elements)", bad[:20])
    assert (ref[:n_ok] == -32768).any() and (ref[:n_ok] == 0).any()                            # both zeros are in the table


# ---- byte identity of the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_tiny_model_is_the_dense_model_to_the_byte(fmt):
    """d 192, F 64, 8 experts top-4, two layers, 418 rows with shared prefixes and a duplicate: the gate / up GEMM has K = 192 (3 k
    tiles of 2 scale blocks, 96-byte rows, 6 scale bytes a row), the down GEMM K = 64 (one k tile, 32-byte rows); 2F = 128 and
    d = 192 are both padded to 256 rows.  Flat and tree, B2T_CLM_GEMM_256 = 0 and 2."""
    dense, mx, dims = _pair(fmt, sliding_window=40)
    assert (dims["d_model"], dims["ffn_dim"]) == (192, 64)
    _, _, routes = _identical("tiny", dense, mx, contract_seqs(dims["vocab"]))
    assert routes.shape == (2, 418, 4)


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_two_k_tiles_in_the_down_gemm(fmt):
    """F = 128: the down GEMM has two k tiles (64-byte rows, 4 scale bytes), 2F = 256 fills the gate / up stride exactly."""
    dense, mx, dims = _pair(fmt, seed=1, intermediate_size=128)
    assert R.mixtral_strides(dims) == (256, 256)
    _identical("F 128", dense, mx, tiny_seqs(dims["vocab"], seed=4, lens=(1, 17, 64, 65, 100, 130)))


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_128_experts(fmt):
    """128 experts, top-4, on the tiny widths, 228 rows: most segments hold a few rows, many none."""
    dense, mx, dims = _pair(fmt, num_local_experts=128, router_scale=1.0)
    _, _, routes = _identical("128 experts", dense, mx, tiny_seqs(dims["vocab"], seed=6, lens=(33, 65, 130)))
    assert len(set(routes.reshape(-1))) > 40


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_one_full_width_layer_on_both_tiles(fmt):
    """One layer at the gpt-oss-20b widths: d = F = 2880 (45 k tiles, 1440-byte rows of nibbles and 90 scale bytes a row, neither a
    multiple of 128; 11.25 tiles of 256), 32 experts top-4, vocab 515, on both tiles: 3 rows, so that most segments are empty,
    and 302 rows, so that most are full."""
    dense, mx, dims = _pair(fmt, n_layers=1, hidden_size=2880, num_attention_heads=64, num_key_value_heads=8, intermediate_size=2880,
                            num_local_experts=32, sliding_window=128, layer_types=["sliding_attention"], vocab_size=515, router_scale=1.0)
    assert mx.expert_bytes() == 32 * (5888 * (1440 + 90) + 3072 * (1440 + 90))
    _, _, few = _identical("full width, 3 rows", dense, mx, [[2, 17, 250]])
    assert len(set(few.reshape(-1))) <= 12
    seqs = tiny_seqs(dims["vocab"], seed=12, lens=(160, 65, 33, 31, 13))
    assert sum(map(len, seqs)) == 302
    _, _, many = _identical("full width, 302 rows", dense, mx, seqs)
    assert len(set(many.reshape(-1))) > 16
    _MODELS.clear()     # gigabytes


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_score_alone_equals_score_in_a_batch(fmt):
    dense, mx, dims = _pair(fmt, sliding_window=16)
    V = dims["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=99)
    s0, t0, _ = _call(mx, [probe], False)
    d0 = _call(dense, [probe], False)
    assert s0.tobytes() == d0[0].tobytes() and _same(t0, d0[1])
    for pos in (0, 50, 99):
        batch = others[:pos] + [probe] + others[pos:]
        assert len(batch) == 100
        for tree in (False, True):
            s, t, _ = _call(mx, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(mx, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()


# ---- the public surface -----------------------------------------------------------------------------------------------------------
def test_scorer_surface(tmp_path):
    """build_scorer(dir, expert_weights="mxfp4") on a saved checkpoint against the default build of the same directory: dtype None,
    "bfloat16" and "auto", share_prefixes both ways: score, token_logprobs and last_stats are identical; w holds uint8 experts of
    the derived size and no dense ones; the device memory the weights take shrinks accordingly; the cache stays refused."""
    import torch
    cfg = gptoss_config()[1]
    save_checkpoint(str(tmp_path / "mx"), cfg, packed_state(cfg, "bfloat16", seed=5))
    seqs = tiny_seqs(cfg["vocab_size"], seed=8, lens=(1, 9, 40))
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        for share in (False, True):
            dense = R.build_scorer(str(tmp_path / "mx"), device="cuda", dtype=dt, share_prefixes=share)
            mx = R.build_scorer(str(tmp_path / "mx"), device="cuda", dtype=dt, share_prefixes=share, expert_weights="mxfp4")
            assert type(dense) is R.GptOssScorer and type(mx) is R.GptOssMxScorer and mx.dtype is dense.dtype is want
            a, b = dense.token_logprobs(seqs), mx.token_logprobs(seqs)
            assert _same(a, b) and all(np.isfinite(t).all() for t in b) and mx.last_stats == dense.last_stats == \
                {"tokens": 50, "nodes": 48 if share else 50}
            assert mx.score(seqs, 0.25).tobytes() == dense.score(seqs, 0.25).tobytes() and mx.last_stats == dense.last_stats
            for tree in (False, True):
                assert _same(mx.token_logprobs(seqs, share_prefixes=tree), a)
            held = {k: v for k, v in mx.w.items() if k.endswith(("_q", "_s"))}
            assert len(held) == 8 and all(v.dtype is torch.uint8 and v.is_cuda for v in held.values())
            assert sum(v.numel() for v in held.values()) == 2 * expert_bytes(mx.dims) == mx.expert_bytes()
            assert not [k for k in mx.w if k.endswith(("gate_up_w", "down_w"))]
            size = lambda sc: sum(v.numel() * v.element_size() for v in {v.data_ptr(): v for v in sc.w.values()}.values())
            dense_experts = sum(v.numel() * 2 for k, v in dense.w.items() if k.endswith(("gate_up_w", "down_w")))
            assert size(dense) - size(mx) == dense_experts - mx.expert_bytes() and dense_experts * 17 == mx.expert_bytes() * 64
    with pytest.raises(ValueError, match="context cache"):
        R.build_scorer(str(tmp_path / "mx"), device="cuda", context_cache_tokens=64, expert_weights="mxfp4")
    with pytest.raises(RuntimeError, match="b2t_clm_gptoss_mx_score_tree_bf16.*max_pos"):     # the last scorer shares prefixes
        mx.score([[2] * 513])


def test_service_end_to_end(tmp_path):
    """LocalLMService with do_opt = 1 over three sentences with a growing context: the service takes whatever scorer it is given,
    and with the mx scorer its replies are, field by field, those with the dense scorer of the same checkpoint."""
    import evaluate_model_helpers as H
    from remote_lm import LocalLMService
    cfg = gptoss_config()[1]
    save_checkpoint(str(tmp_path / "mx"), cfg, packed_state(cfg, "bfloat16", seed=6))
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    tok = R.WordTokenizer(vocab_size=cfg["vocab_size"], bos_id=2, pad_id=1)
    lists = [gold["decode"][i]["nbest"] for i in (0, 1, 0)]
    replies = {}
    for experts in ("dense", "mxfp4"):
        sc = R.build_scorer(str(tmp_path / "mx"), device="cuda", dtype="auto", share_prefixes=True, expert_weights=experts)
        ctx, replies[experts] = "well then " * 12, []
        for nbest in lists:
            r = LocalLMService(_ListDecoder(nbest), acoustic_scale=0.3, alpha=0.5, nbest=100, decode_fn=lambda *a: None,
                               llm=(sc, tok), do_opt=1, top_candidates_to_augment=20)
            r.set("contextual_decoding_current_context", ctx)
            t0 = H.get_current_redis_time_ms(r)
            H.reset_remote_language_model(r, t0)
            r.xadd("remote_lm_finalize", {"done": 0})
            reply = r.streams["remote_lm_output_final"][-1][1]
            replies[experts].append(reply)
            ctx = ctx + " " + reply[b"lm_response_final"].decode()
        assert sc.last_stats["tokens"] > 20 * 24 and sc.last_stats["nodes"] < sc.last_stats["tokens"]
    for a, b in zip(replies["dense"], replies["mxfp4"]):
        assert set(a) == set(b) and b"scoring" in a and a[b"lm_response_final"]
        for k in a:
            assert a[k] == b[k], k
