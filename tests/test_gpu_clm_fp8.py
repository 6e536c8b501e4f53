"""b2t_clm_llama_fp8_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 and b2t_clm_fp8_unpack_f16 / _bf16
(csrc/causal_lm_llama_fp8.hip, the packed form of the plain tile in csrc/clm_gemm.h) on the MI355X.  The contract is not a
tolerance: the calls on the projections kept in block-scaled FP8 give the BYTES -- scores and token log-probs -- of the
b2t_clm_llama_* / b2t_clm_qwen3_* calls on the same checkpoint expanded by the dense reading, flat, tree and cached, fp16 and
bf16, on both tiles.  The reference of every model test here is therefore the dense scorer of the same state dict, whose
families tests/test_gpu_clm_llama.py and tests/test_gpu_clm_qwen3.py hold to the float64 restatement; the reference of the
unpack table is torch's (q.float() * s).to(dtype).

The checkpoints are fp8_state's (tests/test_clm_fp8_host.py): codes uniform over the 254 that are no NaN, a different scale
2^U(-9, -5) in every block; the host file checks that the restatement stays finite on them.  Every call (the rig of
tests/test_gpu_clm_llama.py) gets a fresh workspace of exactly the size the library asks for, filled with 0xFF, with canaries
behind it and behind the outputs; the packed arrays of a scorer under test are sub-views inside larger allocations (_guarded),
the codes' filled with 0xFF, a NaN code, and the scales' with fp32 NaN: a read beyond a row's, a block's or an array's end that
reaches an MFMA shows in the bytes.

None of this runs without the feature: the symbols, the keyword and the scorer do not exist before it.  What each planted change
of the unpack or of the fetch fails is listed in NOTES.md ("LLM")."""
import ctypes as C
import os

import numpy as np
import pytest

import llm_rescore as R
from test_clm_fp8_host import MODELS, fp8_state, model_cfg, plain_of, save_fp8, weight_bytes
from test_clm_llama_host import _save_word_tokenizer, tiny_seqs
from test_clm_mixtral_host import contract_seqs
from test_gpu_clm_cache import SETTINGS, _same_bytes
from test_gpu_clm_llama import _call, _prod_list, _same
from test_gpu_clm_llama_cache import FamilyLib, Rig

pytestmark = pytest.mark.gpu
GUARD = 4096


def _guarded(sc):
    """Moves the scorer's packed arrays into the middle of larger allocations -- 0xFF bytes around the codes, fp32 NaN around the
    scales -- and points the descriptor at them."""
    import torch
    sc._guards = []
    for k in [k for k in sc.w if k.endswith(sc._OWN_ARRAYS)]:
        t = sc.w[k]
        nb = t.numel() * t.element_size()
        buf = torch.full((nb + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        if t.dtype is torch.float32:
            buf.view(torch.float32)[:] = float("nan")
        buf[GUARD:GUARD + nb] = t.reshape(-1).view(torch.uint8)
        sc.w[k] = buf[GUARD:GUARD + nb].view(t.dtype).view(t.shape)
        sc._guards.append(buf)
    sc._point({})
    assert sc._fp8_layers[0].qkv_s == sc.w["layers.0.qkv_s"].data_ptr() == sc._guards[1].data_ptr() + GUARD
    return sc


_PAIRS = {}


def _pair(name, fmt="float16", seed=0):
    """(the dense scorer, the packed scorer with guarded arrays, dims) of fp8_state for the model `name` in its block, cached"""
    key = (name, fmt, seed)
    if key not in _PAIRS:
        cfg, block = model_cfg(name), MODELS[name]
        st = fp8_state(cfg, fmt, seed, block, device="cuda")
        dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
        dense = R.LlamaScorer(dims, R.llama_device_layout(R.fp8_dense_state(st, dims, block, fmt), dims, inv, dtype=fmt), "cuda", dtype=fmt)
        packed = _guarded(R.Fp8LlamaScorer(dims, R.llama_fp8_device_layout(st, dims, inv, fmt, block), "cuda", dtype=fmt))
        assert packed.weight_bytes() == weight_bytes(dims, block[1]) and packed.block_k == block[1]
        assert not [k for k in packed.w if k.endswith(("qkv_w", "o_w", "gate_up_w", "down_w"))]
        assert dense._family == ("qwen3" if name == "qwen3" else "llama") and packed._family == "llama_fp8"
        _PAIRS[key] = (dense, packed, dims)
    return _PAIRS[key]


# ---- the unpack table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block_k", [64, 128])
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_unpack_table(fmt, block_k):
    """b2t_clm_fp8_unpack_* over all 254 codes under every scale of a list, equal to torch's (q.float() * s).to(dtype) bit for
    bit, the signs of zero included.  K = 256; row r holds the codes shifted by r, so every byte position of an 8-byte piece sees
    every code; a group of 32 rows has one scale in every column block, and there is one group for every K / block_k scales of the
    list: 1.0; 1.337 * 2^-14, whose results are fp16 subnormals; random 24-bit mantissas; and, in bf16 alone, 1.1 * 2^-120, whose
    products are fp32 subnormals, and 150.0, which overflows fp16."""
    import torch
    import b2t_native as N
    lib = N.load()
    wdt = R.clm_dtype(fmt)
    K, nkb = 256, 256 // block_k
    g = torch.Generator().manual_seed(11)
    col = [1.0, 1.337 * 2.0 ** -14] + torch.exp2(-12 + 16 * torch.rand(10, generator=g, dtype=torch.float64)).tolist()
    if fmt == "bfloat16":
        col += [1.1 * 2.0 ** -120, 150.0]
    col += [1.0] * (-len(col) % nkb)
    s = torch.tensor(col, dtype=torch.float64).float().reshape(-1, nkb)                  # [groups][K / block_k]
    groups = s.shape[0]
    assert (s[1:, :].view(torch.int32) & 0xFFF != 0).sum() >= 8                          # full mantissas
    ok = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.int64)
    rows = 32 * groups
    q = ok[(torch.arange(K)[None, :] + torch.arange(rows)[:, None] * 9) % 254].to(torch.uint8)   # 32 rows x 256 columns see every code
    for grp in range(groups):
        for kb in range(nkb):
            assert len(set(q[32 * grp:32 * grp + 32, kb * block_k:(kb + 1) * block_k].flatten().tolist())) == 254
    want = (q.view(torch.float8_e4m3fn).float() * s.repeat_interleave(32, 0).repeat_interleave(block_k, 1)).to(wdt)
    assert torch.isfinite(want.float()).all()
    f = want.float().abs()
    if fmt == "float16":
        assert ((f > 0) & (f < 2.0 ** -14)).any() and (want.view(torch.int16) == -32768).any() and (want.view(torch.int16) == 0).any()
    else:
        assert ((f > 0) & (f < 2.0 ** -126)).any() and float(f.max()) > 65504      # 448 * 150 = 67200, in bf16 67072
    qd = torch.full((q.numel() + 2 * GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
    sd = torch.full((s.numel() + 2 * GUARD // 4,), float("nan"), dtype=torch.float32, device="cuda")
    qd[GUARD:-GUARD], sd[GUARD // 4:-GUARD // 4] = q.reshape(-1).cuda(), s.reshape(-1).cuda()
    out = torch.full((rows * K + 256,), -2, dtype=torch.int16, device="cuda")
    rc = getattr(lib, "b2t_clm_fp8_unpack_" + ("bf16" if fmt == "bfloat16" else "f16"))(
        qd.data_ptr() + GUARD, sd.data_ptr() + GUARD, rows, K, block_k, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, N.last_error()
    torch.cuda.synchronize()
    assert (out[rows * K:] == -2).all()
    got = out[:rows * K].cpu().reshape(rows, K)
    ref = want.view(torch.int16)
    bad = [(r // 32, col[r // 32 * nkb:(r // 32 + 1) * nkb], int((got[r] != ref[r]).sum())) for r in range(rows) if not torch.equal(got[r], ref[r])]
    assert not bad, (fmt, "rows with wrong bits (group, scales, elements)", bad[:10])


# ---- byte identity of the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_packed_model_is_the_dense_model_to_the_byte(name, fmt):
    """llama: d 256, 4 / 2 heads of 64, ffn 320 in blocks of [32, 64] -- K = 320 is 5 blocks of one k tile each, every group of 32
    stored rows has a scale row of its own.  qwen2: d 512, head dim 128, ffn 448, q / k / v biases, [64, 64] -- the bias form of
    EP_ROPE.  qwen3: d 512, 4 / 2 heads of 128, ffn 640 in the published [128, 128] -- a block spans two k tiles, a 256-wide tile
    two block rows, K = 640 is 5 blocks; EP_QKNORM_ROPE.  tiny_seqs' lengths and the contract's 418 rows with shared prefixes and a
    duplicate; flat and tree; B2T_CLM_GEMM_256 = 0 and 2.  The dense flat call under the first mode is the reference."""
    dense, packed, dims = _pair(name, fmt)
    V = dims["vocab"]
    for what, seqs in (("lens", tiny_seqs(V, seed=2)), ("contract", contract_seqs(V))):
        s0, t0 = _call(dense, seqs, False, "0", family=dense._family)
        for mode in ("0", "2"):
            for tree in (False, True):
                s, t = _call(packed, seqs, tree, mode, family="llama_fp8")
                assert s.tobytes() == s0.tobytes() and _same(t, t0), (name, fmt, what, mode, tree, float(np.abs(s - s0).max()))
        print(f"CLM fp8 {name} {fmt} {what}: {sum(map(len, seqs))} tokens, sum of scores {float(s0.sum()):.4f}: 4 packed calls "
              f"identical to the dense call")
    assert _same(packed.token_logprobs(seqs[:3]), t0[:3]) and packed.last_stats["tokens"] == sum(map(len, seqs[:3]))


# ---- the cached call ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_cached_call(name):
    """fp16: call one fills the cache with a context of 40 tokens, call two reuses it behind a context grown by the first
    candidate; both have the bytes of the dense cached calls and of the dense flat call; n_reused is the plan's (Rig.call holds
    rows, reused and n to the dictionary rule), B2T_CLM_TRUNK_ATTN 0 and 1."""
    dense, packed, dims = _pair(name, "float16")
    V = dims["vocab"]
    one = _prod_list(V, seed=3, cands=12, context=40)
    two = [one[0][:55] + s[41:] for s in _prod_list(V, seed=4, cands=12, context=40)]
    for setting in SETTINGS:
        rd, rp = Rig(dense, 96, setting), Rig(packed, 96, setting)
        rd.lib, rp.lib = FamilyLib(rd.lib, dense, dense._family), FamilyLib(rp.lib, packed, "llama_fp8")
        reused = []
        for seqs, mode in ((one, "0"), (two, "2")):
            flat = _call(dense, seqs, False, mode, family=dense._family)
            sd, td, pd = rd.call(seqs, mode, 1)
            sp, tp, pp = rp.call(seqs, mode, 1)
            assert pp == pd
            _same_bytes((sp, tp), (sd, td), f"{name}: packed cached against dense cached (trunk attention {setting})")
            _same_bytes((sp, tp), flat, f"{name}: packed cached against dense flat (trunk attention {setting})")
            reused.append(pp["reused"])
        assert reused[0] == 0 and reused[1] >= 40 and rp.chain() == rd.chain()


# ---- the dense reading and the public surface -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llama", "qwen3"])
def test_directory_scores_as_its_plain_state_dict(name, tmp_path):
    """build_scorer(dir) of the FP8 directory -- the dense reading -- scores byte for byte as a LlamaScorer built from the
    dequantised plain state dict, and so does build_scorer(dir, linear_weights="fp8"); dtype "auto" is the directory's bfloat16."""
    import torch
    cfg, block = model_cfg(name), MODELS[name]
    st = fp8_state(cfg, "bfloat16", seed=5, block=block)
    path = save_fp8(str(tmp_path / name), cfg, st, block, dtype="bfloat16")
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    seqs = tiny_seqs(cfg["vocab_size"], seed=8, lens=(1, 9, 40, 65))
    for dt in (None, "auto"):
        fmt = "bfloat16" if dt == "auto" else "float16"
        ref = R.LlamaScorer(dims, R.llama_device_layout({k: v.cuda() for k, v in plain_of(st, block, fmt).items()}, dims, inv, dtype=fmt),
                            "cuda", dtype=fmt)
        want = ref.token_logprobs(seqs)
        assert all(np.isfinite(t).all() for t in want)
        for lw in ("dense", "fp8"):
            for share in (False, True):
                sc = R.build_scorer(path, device="cuda", dtype=dt, share_prefixes=share, linear_weights=lw)
                assert type(sc) is (R.Fp8LlamaScorer if lw == "fp8" else R.LlamaScorer) and sc.dtype is getattr(torch, fmt)
                assert _same(sc.token_logprobs(seqs), want), (name, dt, lw, share)
                assert sc.last_stats == {"tokens": 115, "nodes": 112 if share else 115}     # the lists share their first token
                assert sc.score(seqs, 0.25).tobytes() == ref.score(seqs, 0.25).tobytes()
        held = {k: v for k, v in sc.w.items() if k.endswith(sc._OWN_ARRAYS)}
        assert len(held) == 16 and all(v.is_cuda for v in held.values()) and sc.weight_bytes() == weight_bytes(dims, block[1])
    cached = R.build_scorer(path, device="cuda", context_cache_tokens=64, linear_weights="fp8")
    assert _same(cached.token_logprobs(seqs[2:3]), R.build_scorer(path, device="cuda").token_logprobs(seqs[2:3]))
    assert cached.last_stats["reused"] == 0 and cached.cache_len == 40      # one sequence: all of it is the trunk
    with pytest.raises(RuntimeError, match="b2t_clm_llama_fp8_score_tree_bf16.*max_pos"):     # the last scorer shares prefixes
        sc.score([[2] * 257])


def test_build_opt_with_packed_weights(tmp_path):
    """build_opt(dir, linear_weights="fp8", share_prefixes=True): one n-best list scored as the dense scorer scores it."""
    cfg, block = model_cfg("qwen3"), MODELS["qwen3"]
    path = save_fp8(str(tmp_path / "m"), cfg, fp8_state(cfg, "bfloat16", seed=6, block=block), block)
    assert _save_word_tokenizer(path, cfg["vocab_size"]), "the tokenizers library is missing"
    packed, tok = R.build_opt(path, device="cuda", share_prefixes=True, linear_weights="fp8", dtype="auto")
    dense, _ = R.build_opt(path, device="cuda", share_prefixes=True, dtype="auto")
    assert type(packed) is R.Fp8LlamaScorer and type(dense) is R.LlamaScorer
    nbest = ["w17 w40 w5 w900 w17 w33", "w17 w40 w5 w900 w8 w33", "w17 w40 w5 w900 w17 w34", "w8 w40 w5 w900 w17 w33 w77"]
    ids = [[2] + list(tok(t)["input_ids"]) for t in nbest]
    assert ids[0][:3] == [2, 17, 40] and all(len(x) >= 7 for x in ids)
    a, b = packed.score(ids, 0.1), dense.score(ids, 0.1)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all() and len(set(a.tolist())) > 1
    assert packed.last_stats == dense.last_stats and packed.last_stats["nodes"] < packed.last_stats["tokens"]
