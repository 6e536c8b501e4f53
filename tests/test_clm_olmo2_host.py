"""Host-side checks of the OLMo-2 rescorer (csrc/causal_lm_olmo2.hip, "olmo2" in llm_rescore; no GPU): the loader's device
layout against the state dict, the refusals, the float64 restatement of the contract (ref_logp_olmo2, the reference of
tests/test_gpu_clm_olmo2.py) against HF fp32 Olmo2ForCausalLM and against the same restatement with a per-head norm, the
preconditions of the GPU bounds, the nine entry points' declarations, bindings, sizes and refusals before any device work, the
kernels of the translation unit and a scorer on the CPU.

The two tiny models (TINY) are random HF Olmo2ForCausalLM built in memory with tiny_model's recipe
(tests/test_clm_llama_host.py).  In both the q | k width (Hq + Hkv) hd (512 and 384) is greater than d (384 and 256), so the
fp32 region is wider than the o_proj / down rows that share it; the QKV widths 640 and 512, group sizes 3 and 2, head dims 128
and 64."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, _model, hf_inv_freq, hf_logp, ref_dims, state_of, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TINY = {
    "hd128": dict(hidden_size=384, num_attention_heads=3, num_key_value_heads=1, intermediate_size=320, vocab_size=1003,
                  max_position_embeddings=256, tie_word_embeddings=True, rms_norm_eps=1e-6),
    "hd64": dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=448, vocab_size=777,
                 max_position_embeddings=256, tie_word_embeddings=False, rms_norm_eps=1e-5),
}
HOST_LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
E_BF16_MAX = 0.1   # the precondition of the bf16 bound, as in tests/test_clm_llama_bf16_host.py
HF_BOUND = 8e-5    # 10 x the largest figure measured for these shapes and lengths (8.0e-6), never above 1e-4: the form of
                   # test_clm_llama_host.HF_BOUND
PER_HEAD_MIN = 0.2  # the per-head norm (Qwen3's) is another function: measured 0.71 (hd128) and 1.92 (hd64)


def tiny_olmo2(name, n_layers=2, fmt="float16", **over):
    """tiny_model's recipe (tests/test_clm_llama_host.py) for TINY[name]: (HF fp32 CPU Olmo2ForCausalLM in eval mode with random
    weights representable in fmt, its config as the dict of config.json).  Every norm weight -- q_norm [Hq hd], k_norm
    [Hkv hd], the two post-norms, the final norm -- is 1 + 0.2 N(0, 1), so no two of them are alike."""
    import torch
    import transformers
    kw = dict(TINY[name], **over)
    cfg = transformers.Olmo2Config(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = transformers.Olmo2ForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(300 + sorted(TINY).index(name))
    rdt = getattr(torch, fmt)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("norm.weight") or "layernorm" in k:
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif k.endswith(".bias"):
                v = 0.3 * torch.randn(p.shape, generator=g)
            elif "embed_tokens" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            p.copy_(v.to(rdt).float())
    return model, json.loads(cfg.to_json_string())


def ref_logp_olmo2(st, dims, inv_freq, seqs, fmt=None, per_head=False):
    """The float64 restatement of include/b2t.h's OLMo-2 contract.  fmt = None rounds nowhere; "float16" / "bfloat16" round
    where the kernels round: the residual as a GEMM operand, q (after the whole-row norm, the rotation and hd^-0.5), k (after
    norm and rotation), v, P per 32-key block, the attention output, silu(gate) * up and the final norm's output -- and never
    the o_proj / down outputs, which the post-norms read unrounded.  per_head=True takes the q / k statistic per head (Qwen3's
    norm, with the same weights): another function, which test_restatement shows."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    rnd = (lambda t: t) if fmt is None else (lambda t: t.to(R.clm_dtype(fmt)).double())
    d, Hq, Hkv, nl, V, eps = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "n_layers", "vocab", "rms_eps"))
    hd, G = d // Hq, Hq // Hkv
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["model.embed_tokens.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    ang = pos.double()[:, None] * torch.as_tensor(np.asarray(inv_freq, np.float32), device=dev).double()[None, :]
    cos, sin = torch.cos(ang), torch.sin(ang)
    if fmt is not None:
        cos, sin = cos.float().double(), sin.float().double()      # the fp32 table
    cos, sin = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]   # [M, 1, hd]
    rot = lambda t: t * cos + torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1) * sin        # HF's rotate_half
    rms = lambda t, w: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * W(w)
    lin = lambda t, p: t @ W(p + ".weight").T

    def qk(t, H, w):   # [M, H hd] -> normed [M, H, hd]
        if per_head:
            t = t.view(-1, H, hd)
            return t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * W(w).view(H, hd)
        return rms(t, w).view(-1, H, hd)
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(x)
        q = rnd(rot(qk(lin(h, p + "self_attn.q_proj"), Hq, p + "self_attn.q_norm.weight")) * hd ** -0.5)
        k = rnd(rot(qk(lin(h, p + "self_attn.k_proj"), Hkv, p + "self_attn.k_norm.weight")))
        v = rnd(lin(h, p + "self_attn.v_proj")).view(M, Hkv, hd)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)     # query head h reads kv head h // G
        o = torch.empty(M, d, dtype=torch.float64, device=dev)
        for j in range(B):                                              # one sequence at a time: these are tiny
            n = lens[j]
            sl = slice(off[j], off[j + 1])
            s = q[sl].transpose(0, 1) @ k[sl].transpose(0, 1).transpose(1, 2)      # [Hq, n, n]
            kk = torch.arange(n, device=dev)
            s = s.masked_fill((kk[None, :] > kk[:, None])[None], float("-inf"))
            nb = -(-n // 32)
            sb = F.pad(s, (0, nb * 32 - n), value=float("-inf")).view(Hq, n, nb, 32)
            mb = sb.amax(-1).cummax(-1).values
            pb = torch.exp(sb - mb[..., None])
            resc = torch.exp(mb - mb[..., -1:])[..., None]
            lsum = (pb * resc).sum((-1, -2))
            pr = (rnd(pb) * resc).view(Hq, n, nb * 32)[..., :n]
            o[sl] = ((pr @ v[sl].transpose(0, 1)) / lsum[..., None]).transpose(0, 1).reshape(n, d)
        x = x + rms(lin(rnd(o), p + "self_attn.o_proj"), p + "post_attention_layernorm.weight")
        h = rnd(x)
        gate = lin(h, p + "mlp.gate_proj")
        x = x + rms(lin(rnd(gate * torch.sigmoid(gate) * lin(h, p + "mlp.up_proj")), p + "mlp.down_proj"),
                    p + "post_feedforward_layernorm.weight")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = rnd(rms(x[src], "model.norm.weight"))
    E = st["lm_head.weight"] if "lm_head.weight" in st else st["model.embed_tokens.weight"]
    lp = ((h * E[tgt].double()).sum(-1) - torch.logsumexp(h @ E.double().T, -1)).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def olmo2_state(name, fmt="float16", **kw):
    """(model, cfg, state dict without a tied lm_head, reference dims, inv_freq)"""
    model, cfg = tiny_olmo2(name, fmt=fmt, **kw)
    return model, cfg, state_of(model, TINY[name]["tie_word_embeddings"]), ref_dims(cfg), hf_inv_freq(model)


def _maxdiff(a, b):
    return float(max(np.abs(x - y).max() for x, y in zip(a, b)))


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict(name, fmt, tmp_path):
    """Every array equals its state-dict tensor bit for bit: gate / up interleaved in blocks of 32, q / k rows and the norm
    weights NOT permuted (head dim 128 included), the two post-norms in norm1_w / norm2_w."""
    import torch
    import llm_rescore as R
    model, cfg = tiny_olmo2(name, fmt=fmt)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_olmo2_arrays(str(tmp_path), dtype=fmt)
    sd = model.state_dict()
    rd = ref_dims(cfg)
    wdt = getattr(torch, fmt)
    assert cfg["model_type"] == "olmo2" and dims == R.olmo2_dims(cfg)
    assert dims["max_pos"] == 256 and dims["tied"] is TINY[name]["tie_word_embeddings"] and "qk_norm" not in dims
    for k in ("n_layers", "d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab"):
        assert dims[k] == rd[k], k
    assert dims["rms_eps"] == TINY[name]["rms_norm_eps"]
    d, Hq, Hkv, Fd, V = rd["d_model"], rd["n_heads"], rd["n_kv_heads"], rd["ffn_dim"], rd["vocab"]
    hd = d // Hq
    assert (Hq + Hkv) * hd > d
    eq = lambda a, b: a.dtype == wdt and torch.equal(a, b.to(wdt)) and torch.equal(a.float(), b)   # bit for bit, and exact
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    if TINY[name]["tie_word_embeddings"]:
        assert arr["lm_head"] is arr["embed_tokens"]
    else:
        assert eq(arr["lm_head"][:V], sd["lm_head.weight"]) and not arr["lm_head"][V:].any()
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (256, hd // 2)
    cos, sin = R.rope_tables(hf_inv_freq(model), 256)
    assert np.array_equal(arr["rope_cos"].numpy(), cos) and np.array_equal(arr["rope_sin"].numpy(), sin)
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        assert eq(a("norm1_w"), sd[p + "post_attention_layernorm.weight"])
        assert eq(a("norm2_w"), sd[p + "post_feedforward_layernorm.weight"])
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any()
        assert eq(w[:Hq * hd], sd[p + "self_attn.q_proj.weight"])                       # checkpoint order
        assert eq(w[Hq * hd:(Hq + Hkv) * hd], sd[p + "self_attn.k_proj.weight"])
        assert eq(w[(Hq + Hkv) * hd:qw], sd[p + "self_attn.v_proj.weight"])
        assert f"layers.{l}.qkv_b" not in arr
        assert a("q_norm_w").shape == (Hq * hd,) and eq(a("q_norm_w"), sd[p + "self_attn.q_norm.weight"])
        assert a("k_norm_w").shape == (Hkv * hd,) and eq(a("k_norm_w"), sd[p + "self_attn.k_norm.weight"])
        assert eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"])
        blocks = a("gate_up_w")[:2 * Fd].view(Fd // 32, 2, 32, d)
        assert eq(blocks[:, 0].reshape(Fd, d), sd[p + "mlp.gate_proj.weight"])
        assert eq(blocks[:, 1].reshape(Fd, d), sd[p + "mlp.up_proj.weight"])
        assert eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"])
        assert not torch.equal(a("norm1_w"), a("norm2_w"))
    assert not torch.equal(arr["layers.0.q_norm_w"], arr["layers.1.q_norm_w"])
    for t in arr.values():
        assert t.is_contiguous()


def test_refusals(tmp_path):
    import llm_rescore as R
    model, cfg = tiny_olmo2("hd64", n_layers=1)
    assert cfg["model_type"] == "olmo2" and "olmo2" not in R.LLAMA_MODEL_TYPES
    with pytest.raises(ValueError, match="model_type 'olmo2'"):       # llama_dims stays as it is
        R.llama_dims(cfg)

    def both(match, c, sub):
        with pytest.raises(ValueError, match=match):
            R.olmo2_dims(c)
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(tmp_path / sub), device="cpu")
    plain = {k: v for k, v in cfg.items() if k not in ("rope_parameters", "rope_scaling")} | {"rope_theta": 10000.0}
    both("head dim", cfg | {"hidden_size": 320, "num_attention_heads": 4, "num_key_value_heads": 4}, "hd80")
    both("head dim", cfg | {"hidden_size": 256, "num_attention_heads": 8, "num_key_value_heads": 8}, "hd32")
    both("head dim", cfg | {"hidden_size": 256, "num_attention_heads": 3, "num_key_value_heads": 3}, "hdfrac")
    both("attention_bias", cfg | {"attention_bias": True}, "ab")
    both("hidden_act", cfg | {"hidden_act": "gelu"}, "act")
    both("rope_type", plain | {"rope_scaling": {"rope_type": "yarn", "factor": 2.0}}, "rope")
    both("rope_type", plain | {"rope_scaling": {"type": "linear", "factor": 2.0}}, "rope2")
    both("num_key_value_heads", cfg | {"num_key_value_heads": 3}, "kv")
    # widths: with a head dim of 64 or 128 hidden_size is a multiple of 64, so the refusal can only meet intermediate_size
    both("hidden_size 256 and intermediate_size 300 must be multiples of 64", cfg | {"intermediate_size": 300}, "ffn")
    R.olmo2_dims(plain | {"rope_scaling": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                           "high_freq_factor": 4.0, "original_max_position_embeddings": 64}})
    # the neighbours stay unsupported model types
    for mt in ("olmo", "olmo3"):
        with pytest.raises(ValueError, match=f"model_type '{mt}'"):
            R.olmo2_dims(cfg | {"model_type": mt})
        os.makedirs(tmp_path / mt)
        with open(tmp_path / mt / "config.json", "w") as f:
            json.dump(cfg | {"model_type": mt}, f)
        with pytest.raises(ValueError, match=f"model_type '{mt}' is not supported"):
            R.build_scorer(str(tmp_path / mt), device="cpu")
    # an OLMo-2 directory without weights gets as far as the weights
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    with pytest.raises(ValueError, match="follow-up"):     # bf16 with a cache stays refused
        R.build_scorer(str(bare), device="cuda", dtype="bfloat16", context_cache_tokens=64)
    # the layout: the norm weights are required, biases refused
    st = state_of(model, False)
    dims, inv = R.olmo2_dims(cfg), R.rope_inv_freq(cfg)
    for lack in ("q_norm", "k_norm", "post_feedforward_layernorm"):
        with pytest.raises(KeyError, match=lack):
            R.olmo2_device_layout({k: v for k, v in st.items() if lack not in k}, dims, inv)
    with pytest.raises(ValueError, match="q_proj.bias"):
        R.olmo2_device_layout(dict(st, **{"model.layers.0.self_attn.q_proj.bias": st["model.layers.0.self_attn.k_norm.weight"]}),
                              dims, inv)
    with pytest.raises(ValueError, match="q_norm.weight: shape"):     # a per-head (Qwen3-shaped) weight is not OLMo-2's
        R.olmo2_device_layout(dict(st, **{"model.layers.0.self_attn.q_norm.weight": st["model.layers.0.self_attn.q_norm.weight"][:64]}),
                              dims, inv)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_restatement(name):
    """Unrounded it is HF's fp32 Olmo2ForCausalLM within HF_BOUND; with a per-head q / k norm it is another function (max
    |dlogp| above 0.2); and the preconditions of the GPU bounds hold: 0 < e16, 0 < e_bf16 <= 0.1, restatement against
    restatement.  Measured on the CPU with these seeds and lengths 1..129 (hd128 / hd64): HF 8.0e-6 / 7.3e-6, per-head 0.71 /
    1.92, e16 4.9e-3 / 5.1e-3, e_bf16 4.3e-2 / 3.5e-2."""
    model, cfg, st, rd, inv = olmo2_state(name)
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_olmo2(st, rd, inv, seqs)
    hf = hf_logp(model, seqs)
    err = _maxdiff(exact, hf)
    mx = max(np.abs(b).max() for b in hf)
    moved = _maxdiff(exact, ref_logp_olmo2(st, rd, inv, seqs, per_head=True))
    e16 = _maxdiff(ref_logp_olmo2(st, rd, inv, seqs, "float16"), exact)
    print(f"CLM olmo2 restatement {name}: vs HF fp32 {err:.3e} (max |logp| {mx:.2f}), whole-row vs per-head norm {moved:.3f}, "
          f"e16 {e16:.3e}")
    assert mx > 5 and err <= HF_BOUND, (name, err)
    assert moved > PER_HEAD_MIN, moved
    assert 0 < e16, e16
    # bf16: the weights rounded to bf16 first, as the device holds them
    model, cfg, st, rd, inv = olmo2_state(name, fmt="bfloat16")
    ebf = _maxdiff(ref_logp_olmo2(st, rd, inv, seqs, "bfloat16"), ref_logp_olmo2(st, rd, inv, seqs))
    print(f"CLM olmo2 restatement {name}: e_bf16 {ebf:.3e}")
    assert 0 < ebf <= E_BF16_MAX, ebf


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")
SIZES = ("ws_bytes", "tree_ws_bytes", "cache_kv_bytes", "tree_cached_ws_bytes")


def test_entry_points_are_declared_and_bound():
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY:     # the Qwen3 twin's list
        new, twin = "b2t_clm_olmo2_" + t, "b2t_clm_qwen3_" + t
        assert decl(new) == decl(twin), new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == list(g.argtypes)
        assert f.argtypes[1] == C.POINTER(N.ClmQkNorm)
    for t in SIZES:     # the Llama twin's list
        new, twin = "b2t_clm_olmo2_" + t, "b2t_clm_llama_" + t
        assert decl(new) == decl(twin), new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype == C.c_size_t and list(f.argtypes) == list(g.argtypes)
    assert sorted(re.findall(r"\b(b2t_clm_olmo2_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) == \
        sorted("b2t_clm_olmo2_" + t for t in ENTRY + SIZES)
    assert set("b2t_clm_olmo2_" + t for t in ENTRY + SIZES) <= set(N.header_symbols())


def test_sizes_are_the_llama_sizes_plus_the_fp32_region():
    """ws = the Llama twin's + round_up(4 * round_up(rows, 256) * (Hq + Hkv) * hd, 256) on all three paths (the cached state
    sits behind it unchanged); the cache is the Llama family's; invalid arguments give 0."""
    import b2t_native as N
    lib = N.load()
    for kw in (dict(d=256, heads=4, kv=2), dict(d=384, heads=3, kv=1), dict(d=512, heads=4, kv=4)):
        desc = _model(bias=False, **kw)
        p = C.byref(desc)
        qk = (kw["heads"] + kw["kv"]) * (kw["d"] // kw["heads"])
        extra = lambda rows: -(-4 * (-(-rows // 256) * 256) * qk // 256) * 256
        for M in (1, 2, 255, 256, 257, 692, 4097):
            for n_seq in sorted({1, max(1, M // 3), M}):
                assert lib.b2t_clm_olmo2_ws_bytes(p, M, n_seq) == lib.b2t_clm_llama_ws_bytes(p, M, n_seq) + extra(M)
                for rows in sorted({1, M // 2 + 1, M}):
                    assert lib.b2t_clm_olmo2_tree_ws_bytes(p, rows, M, n_seq) == \
                        lib.b2t_clm_llama_tree_ws_bytes(p, rows, M, n_seq) + extra(rows)
                    assert lib.b2t_clm_olmo2_tree_cached_ws_bytes(p, rows, M, n_seq) == \
                        lib.b2t_clm_llama_tree_cached_ws_bytes(p, rows, M, n_seq) + extra(rows)
        for cap in (1, 8, 64):
            assert lib.b2t_clm_olmo2_cache_kv_bytes(p, cap) == lib.b2t_clm_llama_cache_kv_bytes(p, cap) > 0
        assert lib.b2t_clm_olmo2_cache_kv_bytes(p, 0) == 0 and lib.b2t_clm_olmo2_cache_kv_bytes(p, 65) == 0
    desc = _model(bias=False)
    p = C.byref(desc)
    assert lib.b2t_clm_olmo2_ws_bytes(None, 10, 1) == 0 and lib.b2t_clm_olmo2_tree_ws_bytes(None, 5, 10, 1) == 0
    assert lib.b2t_clm_olmo2_tree_cached_ws_bytes(None, 5, 10, 1) == 0 and lib.b2t_clm_olmo2_cache_kv_bytes(None, 4) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert lib.b2t_clm_olmo2_ws_bytes(p, n_tok, n_seq) == 0, (n_tok, n_seq)
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert lib.b2t_clm_olmo2_tree_ws_bytes(p, nn, nt, ns) == 0, (nn, nt, ns)
        assert lib.b2t_clm_olmo2_tree_cached_ws_bytes(p, nn, nt, ns) == 0, (nn, nt, ns)
    assert lib.b2t_clm_olmo2_ws_bytes(C.byref(_model(heads=0)), 10, 1) == 0
    assert lib.b2t_clm_olmo2_tree_ws_bytes(C.byref(_model(kv=0)), 5, 10, 1) == 0


def _qkn(n=1, q=FAKE, k=FAKE):
    import b2t_native as N
    a = (N.ClmQkNorm * max(1, n))()
    for i in range(n):
        a[i].q_norm_w, a[i].k_norm_w = q, k
    return a


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """Everything the Llama twin refuses, a null array, a null entry and a non-null qkv_b, with fake pointers and no GPU; the
    call's own messages carry its name; the workspace wanted is this family's; on the cached call the cache is left as it
    was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_olmo2_" + entry
    fn = getattr(lib, who)
    tree, cached = "tree" in entry, "cached" in entry
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]
    nb = lambda **kw: _model(bias=False, **kw)     # OLMo-2 has no q / k / v biases
    NOQ = object()

    def refused(match, desc, qkn=NOQ, ids=ok_ids, off=ok_off, own=True, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None,
                cache=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        n = len(off) - 1 if n_seq is None else n_seq
        dp = C.byref(desc) if desc is not None else None
        q = _qkn(desc.n_layers if desc is not None else 1) if qkn is NOQ else qkn
        if cached:
            cache = _cache() if cache is None else cache
            n0, ids0 = cache.n, cache._keep.copy()
            rc = fn(dp, q, C.byref(cache), update, ids.ctypes.data, off.ctypes.data, n, scores, None, None, None, ws, ws_bytes, None)
            assert cache.n == n0 and (cache._keep == ids0).all()     # a refusal leaves the cache alone
        elif tree:
            rc = fn(dp, q, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
        else:
            rc = fn(dp, q, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        if own:
            assert N.last_error().startswith(who + ":"), N.last_error()

    # the model's, as the twin words them
    refused("null model", None, own=False)
    refused("head dim 32", nb(d=256, heads=8, kv=8), own=False)
    refused("head dim 80", nb(d=320, heads=4, kv=4), own=False)
    refused("multiple of n_heads", nb(d=256, heads=3, kv=3), own=False)
    refused("multiple of n_kv_heads", nb(d=512, heads=8, kv=3), own=False)
    refused("multiples of 64", nb(d=256, heads=4, ffn=500), own=False)
    refused("bad dimensions", nb(kv=0), own=False)
    refused("bad dimensions", nb(max_pos=0), own=False)
    refused("rms_eps", nb(eps=-1.0), own=False)
    refused("rms_eps", nb(eps=float("nan")), own=False)
    refused("null weight", N.ClmLlamaDesc(0, 256, 4, 2, 512, 1000, 64, 1e-5, FAKE, FAKE, FAKE, FAKE, 0, None), own=False)
    bad = nb()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad, own=False)
    bad = nb()
    bad.layers_host[0].norm2_w = None      # the post-feedforward norm
    refused("null weight pointer in layer 0", bad, own=False)
    # the norm weights'
    refused("null qk_norm_host", nb(), qkn=None)
    refused("null q / k norm weight in layer 0", nb(), qkn=_qkn(1, q=None))
    two = _qkn(2)
    two[1].k_norm_w = None
    refused("null q / k norm weight in layer 1", nb(n_layers=2), qkn=two)
    refused("layer 0 has q / k / v biases", _model(bias=True))
    # the list's
    refused("null argument", nb(), scores=None)
    refused("null argument", nb(), ws=None)
    refused("n_seq 0", nb(), n_seq=0)
    refused("empty", nb(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", nb(), off=[1, 2, 4])
    refused("outside", nb(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", nb(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", nb(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4], cache=_cache(cap=3) if cached else None)
    # the workspace: this family's size functions; the Llama twin's size is too small
    desc = nb()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes, trunk 2
    if cached:
        need = lib.b2t_clm_olmo2_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
        assert need > lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_olmo2_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)
        # the cache's own
        refused("null cache member", desc, cache=_cache(kv=None))
        refused("above max_pos", nb(max_pos=64), cache=_cache(cap=65))
        refused(r"n 9 outside", desc, cache=_cache(cap=8, n=9))
        refused("cached token 1 has id 1000", nb(vocab=1000), cache=_cache(ids=(2, 1000)))
        rc = fn(C.byref(desc), _qkn(1), None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1, FAKE, None, None,
                None, FAKE, 1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_olmo2_score_tree_f16", N.last_error())
    elif tree:
        need = lib.b2t_clm_olmo2_tree_ws_bytes(C.byref(desc), 4, 9, 3)
        assert need > lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)
    else:
        need = lib.b2t_clm_olmo2_ws_bytes(C.byref(desc), 9, 3)
        assert need > lib.b2t_clm_llama_ws_bytes(C.byref(desc), 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_olmo2_unit_kernels_without_scratch():
    """The unit instantiates the two new epilogues (ids 10 and 11) on two tiles and the two new kernels, each in two element
    types, and nothing else: 12 kernels, ScratchSize 0."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_olmo2.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_olmo2.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_kernel" in k]
    assert len(res) == 12 and len(gemm) == 8, sorted(res)
    assert sum("ELi10E" in k for k in gemm) == 4 and sum("ELi11E" in k for k in gemm) == 4
    assert sum("ILi256ELi256E" in k for k in gemm) == 4 and sum("ILi128ELi128E" in k for k in gemm) == 4
    assert sum(k.endswith("DF16_EEvNS_7ClmGemmE") for k in gemm) == 4 and sum(k.endswith("DF16bEEvNS_7ClmGemmE") for k in gemm) == 4
    for kern in ("clm_olmo2_qknorm_rope_kernel", "clm_olmo2_postnorm_add_kernel"):
        assert sum(kern in k for k in res) == 2, (kern, sorted(res))
    assert all(v.get("ScratchSize", -1) == 0 for v in res.values()), res
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_olmo2.hip")).read()
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src        # the one tile rule
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_QKV_F32, El>)") == 1
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_F32, El>)") == 1


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_olmo2("hd128", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    sd = {k: v.float() for k, v in model.state_dict().items()}
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.Olmo2Scorer) and isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu"
        assert sc._family == "olmo2" and sc._SIZES == "b2t_clm_olmo2_" and R.LlamaScorer._SIZES == "b2t_clm_llama_"
        assert sc.desc.n_heads == 3 and sc.desc.n_kv_heads == 1 and sc.desc.d_model == 384 and sc.desc.vocab == 1003
        assert sc.desc.lm_head == sc.desc.embed_tokens and not sc.desc.layers_host[0].qkv_b
        for l in range(2):
            assert sc._qkn[l].q_norm_w == sc.w[f"layers.{l}.q_norm_w"].data_ptr()
            assert sc._qkn[l].k_norm_w == sc.w[f"layers.{l}.k_norm_w"].data_ptr()
            assert sc.w[f"layers.{l}.q_norm_w"].dtype is want and sc.w[f"layers.{l}.q_norm_w"].shape == (384,)
            assert sc.desc.layers_host[l].norm2_w == sc.w[f"layers.{l}.norm2_w"].data_ptr()
        if want is torch.bfloat16:     # a bf16 checkpoint's values are kept exactly
            assert torch.equal(sc.w["layers.1.k_norm_w"].float(), sd["model.layers.1.self_attn.k_norm.weight"])
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    # Llama arrays are not OLMo-2 arrays
    from test_clm_llama_host import tiny_model
    m2, c2 = tiny_model("llama", n_layers=1)
    d2 = R.llama_dims(c2)
    with pytest.raises(KeyError, match="q_norm_w"):
        R.Olmo2Scorer(d2, R.llama_device_layout(state_of(m2, False), d2, R.rope_inv_freq(c2)), "cpu")
