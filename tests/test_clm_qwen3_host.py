"""Host-side checks of the Qwen3 rescorer (csrc/causal_lm_qwen3.hip, "qwen3" in llm_rescore; no GPU): the loader's device
layout with the q / k norm weights against the state dict, the refusals, the float64 restatement of the contract with the
norm inserted (ref_logp_qwen3, the reference of tests/test_gpu_clm_qwen3.py) against HF fp32 Qwen3ForCausalLM, the five entry
points' declarations, bindings and refusals before any device work, the kernels of the translation unit and a scorer on the
CPU.

The two tiny models (TINY) are random HF Qwen3ForCausalLM built in memory with tiny_model's recipe
(tests/test_clm_llama_host.py).  Their QKV widths N = (Hq + 2 Hkv) hd are 640 and 384, so the last 256-column tile of the QKV
GEMM has waves beyond N (which must still reach the epilogue's barrier), one 256-tile holds a q head beside a k head with
other norm weights, v slices share a workgroup with normed slices, the group sizes are 3 and 4 and the head dims 128 and 64."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_bf16_host import ref_logp_llama_fmt
from test_clm_llama_host import FAKE, _model, hf_inv_freq, hf_logp, ref_dims, state_of, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TINY = {
    "hd128": dict(hidden_size=384, num_attention_heads=3, num_key_value_heads=1, head_dim=128, intermediate_size=320,
                  vocab_size=1003, max_position_embeddings=256, tie_word_embeddings=True, rms_norm_eps=1e-6),
    "hd64": dict(hidden_size=256, num_attention_heads=4, num_key_value_heads=1, head_dim=64, intermediate_size=448,
                 vocab_size=777, max_position_embeddings=256, tie_word_embeddings=False, rms_norm_eps=1e-6),
}
E_BF16_MAX = 0.1   # the precondition of the bf16 bound, as in tests/test_clm_llama_bf16_host.py
HF_BOUND = 1e-4    # 10 x the largest figure measured for these shapes (1.07e-5), the form of test_clm_llama_host.HF_BOUND


def tiny_qwen3(name, n_layers=2, fmt="float16", **over):
    """tiny_model's recipe (tests/test_clm_llama_host.py) for TINY[name]: (HF fp32 CPU Qwen3ForCausalLM in eval mode with random
    weights representable in fmt, its config as the dict of config.json).  q_norm / k_norm weights are 1 + 0.2 N(0, 1) like the
    other norms, different for q and k and from layer to layer."""
    import torch
    import transformers
    kw = dict(TINY[name], **over)
    cfg = transformers.Qwen3Config(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = transformers.Qwen3ForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(200 + sorted(TINY).index(name))
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


def ref_logp_qwen3(st, dims, inv_freq, seqs, fmt=None, qk_norm=True):
    """ref_logp_llama_fmt (tests/test_clm_llama_bf16_host.py) with the one insertion of include/b2t.h's Qwen3 contract: an
    RMSNorm with self_attn.q_norm.weight / k_norm.weight over the head dimension of every q and k head, in front of the
    rotation; nothing is rounded between the projection and the one rounding of q and k behind rotation and scale.  fmt = None
    rounds nowhere, "float16" / "bfloat16" round where the kernels round.  qk_norm=False leaves the norm out (then it is
    ref_logp_llama_fmt, which test_restatement checks)."""
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
        cos, sin = cos.float().double(), sin.float().double()
    cos, sin = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]   # [M, 1, hd]
    rot = lambda t: t * cos + torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1) * sin        # HF's rotate_half
    rms = lambda t, w: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * W(w)
    hnorm = rms if qk_norm else (lambda t, w: t)
    lin = lambda t, p: t @ W(p + ".weight").T + (W(p + ".bias") if p + ".bias" in st else 0.0)
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(rms(x, p + "input_layernorm.weight"))
        q = rnd(rot(hnorm(lin(h, p + "self_attn.q_proj").view(M, Hq, hd), p + "self_attn.q_norm.weight")) * hd ** -0.5)
        k = rnd(rot(hnorm(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd), p + "self_attn.k_norm.weight")))
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
        x = x + lin(rnd(o), p + "self_attn.o_proj")
        h = rnd(rms(x, p + "post_attention_layernorm.weight"))
        gate = lin(h, p + "mlp.gate_proj")
        x = x + lin(rnd(gate * torch.sigmoid(gate) * lin(h, p + "mlp.up_proj")), p + "mlp.down_proj")
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


def qwen3_state(name, fmt="float16", **kw):
    """(model, cfg, state dict without a tied lm_head, reference dims, inv_freq)"""
    model, cfg = tiny_qwen3(name, fmt=fmt, **kw)
    return model, cfg, state_of(model, TINY[name]["tie_word_embeddings"]), ref_dims(cfg), hf_inv_freq(model)


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict_permuted(name, fmt, tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_qwen3(name, fmt=fmt)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_llama_arrays(str(tmp_path), dtype=fmt)
    sd = model.state_dict()
    rd = ref_dims(cfg)
    wdt = getattr(torch, fmt)
    assert dims["qk_norm"] is True and dims["max_pos"] == 256 and dims["tied"] is TINY[name]["tie_word_embeddings"]
    for k in ("n_layers", "d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab"):
        assert dims[k] == rd[k], k
    d, Hq, Hkv, Fd, V = rd["d_model"], rd["n_heads"], rd["n_kv_heads"], rd["ffn_dim"], rd["vocab"]
    hd = d // Hq
    eq = lambda a, b: a.dtype == wdt and torch.equal(a, b.to(wdt)) and torch.equal(a.float(), b)   # bit for bit, and exact
    unperm = lambda t: torch.cat([t[:, 0:32], t[:, 64:96], t[:, 32:64], t[:, 96:128]], 1) if hd == 128 else t   # an involution
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    if TINY[name]["tie_word_embeddings"]:
        assert arr["lm_head"] is arr["embed_tokens"]
    else:
        assert eq(arr["lm_head"][:V], sd["lm_head.weight"]) and not arr["lm_head"][V:].any()
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (256, hd // 2)
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        assert eq(a("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(a("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any()
        un = unperm(w[:(Hq + Hkv) * hd].view(Hq + Hkv, hd, d)).reshape(-1, d)
        assert eq(un[:Hq * hd], sd[p + "self_attn.q_proj.weight"]) and eq(un[Hq * hd:], sd[p + "self_attn.k_proj.weight"])
        assert eq(w[(Hq + Hkv) * hd:qw], sd[p + "self_attn.v_proj.weight"])
        assert f"layers.{l}.qkv_b" not in arr
        # the norm weights: [hd], under the inverse of head_dim_perm like the rows they scale
        for f, hf in (("q_norm_w", "q_norm"), ("k_norm_w", "k_norm")):
            t = a(f)
            assert t.shape == (hd,) and t.is_contiguous()
            assert eq(unperm(t[None])[0], sd[p + f"self_attn.{hf}.weight"]), (l, f)
            inv = np.argsort(R.head_dim_perm(hd))
            assert torch.equal(t[torch.from_numpy(inv)].float(), sd[p + f"self_attn.{hf}.weight"])
        assert not torch.equal(a("q_norm_w"), a("k_norm_w"))
        assert eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"])
        blocks = a("gate_up_w")[:2 * Fd].view(Fd // 32, 2, 32, d)
        assert eq(blocks[:, 0].reshape(Fd, d), sd[p + "mlp.gate_proj.weight"])
        assert eq(blocks[:, 1].reshape(Fd, d), sd[p + "mlp.up_proj.weight"])
        assert eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"])
    assert not torch.equal(arr["layers.0.q_norm_w"], arr["layers.1.q_norm_w"])
    for t in arr.values():
        assert t.is_contiguous()


def test_refusals(tmp_path):
    import llm_rescore as R
    model, cfg = tiny_qwen3("hd64", n_layers=1)
    assert cfg["model_type"] == "qwen3" and "qwen3" in R.LLAMA_MODEL_TYPES
    assert R.llama_dims(cfg)["qk_norm"] is True

    def both(match, c, sub):
        with pytest.raises(ValueError, match=match):
            R.llama_dims(c)
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(tmp_path / sub), device="cpu")
    # a head dim of its own (Qwen3-0.6B: 1024 / 16 with head_dim 128); the message names the checkpoints
    both("head dim.*0.6B, 4B and 32B", cfg | {"hidden_size": 1024, "num_attention_heads": 16, "num_key_value_heads": 8,
                                             "head_dim": 128}, "hd")
    both("attention_bias", cfg | {"attention_bias": True}, "ab")
    # what llama_dims refuses today it refuses for qwen3
    for match, kw in (("rope_type", {"rope_scaling": {"rope_type": "yarn", "factor": 2.0}, "rope_parameters": None}),
                      ("mlp_bias", {"mlp_bias": True}), ("activation", {"hidden_act": "gelu"}),
                      ("multiples of 64", {"intermediate_size": 300}),
                      ("multiple of num_key_value_heads", {"num_key_value_heads": 3})):
        base = {k: v for k, v in cfg.items() if k != "rope_parameters"} | {"rope_theta": 10000.0}
        with pytest.raises(ValueError, match=match):
            R.llama_dims(base | {k: v for k, v in kw.items() if v is not None})
    with pytest.raises(ValueError, match="model_type 'gemma'"):
        R.llama_dims(cfg | {"model_type": "gemma"})
    # a Qwen3 directory without weights gets as far as the weights
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    with pytest.raises(ValueError, match="follow-up"):     # bf16 with a cache stays refused
        R.build_scorer(str(bare), device="cuda", dtype="bfloat16", context_cache_tokens=64)
    # the layout: norm weights are required for qwen3, refused elsewhere, and exclude q / k / v biases
    st = state_of(model, False)
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    with pytest.raises(KeyError, match="q_norm"):
        R.llama_device_layout({k: v for k, v in st.items() if "q_norm" not in k}, dims, inv)
    with pytest.raises(ValueError, match="q / k norm weights"):
        R.llama_device_layout(st, dict(dims, qk_norm=False), inv)
    with pytest.raises(ValueError, match="biases beside"):
        R.llama_device_layout(dict(st, **{"model.layers.0.self_attn.q_proj.bias": st["model.layers.0.input_layernorm.weight"]}),
                              dims, inv)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_restatement(name):
    """Unrounded it is HF's fp32 Qwen3ForCausalLM within 1e-4; without the norm it is another function (log-probs move by more
    than 1) and ref_logp_llama_fmt exactly; bf16 rounding moves it by 0 < e_bf16 <= 0.1.  Measured on the CPU with these
    seeds (hd128 / hd64, log-probs down to -14.6 / -15.8): HF 6.9e-6 / 7.0e-6, with against without 2.70 / 3.13, e16 5.8e-3 /
    8.0e-3, e_bf16 5.7e-2 / 4.7e-2."""
    model, cfg, st, rd, inv = qwen3_state(name)
    seqs = tiny_seqs(cfg["vocab_size"], seed=1)
    exact = ref_logp_qwen3(st, rd, inv, seqs)
    hf = hf_logp(model, seqs)
    err = max(np.abs(a - b).max() for a, b in zip(exact, hf))
    mx = max(np.abs(b).max() for b in hf)
    plain = ref_logp_qwen3(st, rd, inv, seqs, qk_norm=False)
    moved = max(np.abs(a - b).max() for a, b in zip(exact, plain))
    e16 = max(np.abs(a - b).max() for a, b in zip(ref_logp_qwen3(st, rd, inv, seqs, "float16"), exact))
    print(f"CLM qwen3 restatement {name}: vs HF fp32 {err:.3e} (max |logp| {mx:.2f}), with vs without norm {moved:.3f}, e16 {e16:.3e}")
    assert mx > 5 and err <= HF_BOUND, (name, err)
    assert moved > 1, moved
    assert 1e-5 < e16 < 1e-2
    for a, b in zip(plain, ref_logp_llama_fmt(st, rd, inv, seqs)):
        assert np.abs(a - b).max() < 1e-11
    # bf16: the weights rounded to bf16 first, as the device holds them
    model, cfg, st, rd, inv = qwen3_state(name, fmt="bfloat16")
    ebf = max(np.abs(a - b).max() for a, b in zip(ref_logp_qwen3(st, rd, inv, seqs, "bfloat16"), ref_logp_qwen3(st, rd, inv, seqs)))
    print(f"CLM qwen3 restatement {name}: e_bf16 {ebf:.3e}")
    assert 0 < ebf <= E_BF16_MAX, ebf


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")


def test_entry_points_are_declared_and_bound():
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY:
        new, twin = "b2t_clm_qwen3_" + t, "b2t_clm_llama_" + t
        dn, dt = decl(new), decl(twin)
        assert dn == dt[:1] + ["const b2t_clm_qknorm_t* qk_norm_host"] + dt[1:], new     # the twin's list plus the one argument
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype
        assert list(f.argtypes) == list(g.argtypes[:1]) + [C.POINTER(N.ClmQkNorm)] + list(g.argtypes[1:])
    assert not re.search(r"b2t_clm_qwen3_\w*bytes", hdr)       # no new size function
    assert sorted(re.findall(r"\b(b2t_clm_qwen3_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) == \
        sorted("b2t_clm_qwen3_" + t for t in ENTRY)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_qknorm_struct_matches_the_header(tmp_path):
    import b2t_native as N
    src = tmp_path / "lay.c"
    fs = [n for n, _ in N.ClmQkNorm._fields_]
    assert fs == ["q_norm_w", "k_norm_w"]
    body = "".join(f'printf("{f} %zu\\n", offsetof(b2t_clm_qknorm_t, {f}));' for f in fs)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){'
                   'printf("S %zu\\nL %zu\\nD %zu\\nC %zu\\n", sizeof(b2t_clm_qknorm_t), sizeof(b2t_clm_llama_layer_t), '
                   'sizeof(b2t_clm_llama_t), sizeof(b2t_clm_cache_t));' + body + "return 0;}")
    exe = tmp_path / "lay"
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["S"]) == C.sizeof(N.ClmQkNorm) == 16
    for f in fs:
        assert int(got[f]) == getattr(N.ClmQkNorm, f).offset, f
    # the structs beside it keep their layout
    assert int(got["L"]) == C.sizeof(N.ClmLlamaLayer) == 56 and int(got["D"]) == C.sizeof(N.ClmLlamaDesc) == 80
    assert int(got["C"]) == C.sizeof(N.ClmCache) == 32


def _qkn(n=1, q=FAKE, k=FAKE):
    import b2t_native as N
    a = (N.ClmQkNorm * max(1, n))()
    for i in range(n):
        a[i].q_norm_w, a[i].k_norm_w = q, k
    return a


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """Everything the Llama twin refuses, a null array, a null entry and a non-null qkv_b, with fake pointers and no GPU; the
    call's own messages carry its name; on the cached call the cache is left as it was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_qwen3_" + entry
    fn = getattr(lib, who)
    tree, cached = "tree" in entry, "cached" in entry
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]
    nb = lambda **kw: _model(bias=False, **kw)     # Qwen3 has no q / k / v biases
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
    # the workspace: the Llama size functions'
    desc = nb()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes, trunk 2
    if cached:
        need = lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)
        # the cache's own
        refused("null cache member", desc, cache=_cache(kv=None))
        refused("above max_pos", nb(max_pos=64), cache=_cache(cap=65))
        refused(r"n 9 outside", desc, cache=_cache(cap=8, n=9))
        refused("cached token 1 has id 1000", nb(vocab=1000), cache=_cache(ids=(2, 1000)))
        rc = fn(C.byref(desc), _qkn(1), None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1, FAKE, None, None,
                None, FAKE, 1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_qwen3_score_tree_f16", N.last_error())
    elif tree:
        need = lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)
    else:
        need = lib.b2t_clm_llama_ws_bytes(C.byref(desc), 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_qwen3_unit_has_four_kernels_without_scratch():
    """The unit instantiates the one new epilogue (id 6) on two tiles in two element types and nothing else; at the time of
    writing the 256-tile kernels have 223 VGPRs, the 128-tile ones 86 + 64 AGPRs, scratch 0."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_qwen3.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_qwen3.hip").items() if "clm_" in k}
    assert len(res) == 4 and all("clm_gemm_kernel" in k and "ELi6E" in k for k in res), sorted(res)
    assert sum("ILi256ELi256E" in k for k in res) == 2 and sum("ILi128ELi128E" in k for k in res) == 2
    assert sum(k.endswith("DF16_EEvNS_7ClmGemmE") for k in res) == 2 and sum(k.endswith("DF16bEEvNS_7ClmGemmE") for k in res) == 2
    assert all(v.get("ScratchSize", -1) == 0 for v in res.values()), res
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_qwen3.hip")).read()
    assert "B2T_CLM_GEMM_256" not in src and "getenv" not in src        # the one tile rule
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_QKNORM_ROPE, El>)") == 1


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_qwen3("hd128", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    sd = {k: v.float() for k, v in model.state_dict().items()}
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu" and sc._family == "qwen3"
        assert sc.desc.n_heads == 3 and sc.desc.n_kv_heads == 1 and sc.desc.d_model == 384 and sc.desc.vocab == 1003
        assert sc.desc.lm_head == sc.desc.embed_tokens and not sc.desc.layers_host[0].qkv_b
        for l in range(2):
            assert sc._qkn[l].q_norm_w == sc.w[f"layers.{l}.q_norm_w"].data_ptr()
            assert sc._qkn[l].k_norm_w == sc.w[f"layers.{l}.k_norm_w"].data_ptr()
            assert sc.w[f"layers.{l}.q_norm_w"].dtype is want
        if want is torch.bfloat16:     # a bf16 checkpoint's values are kept exactly
            inv = torch.from_numpy(np.argsort(R.head_dim_perm(128)))
            assert torch.equal(sc.w["layers.1.k_norm_w"][inv].float(), sd["model.layers.1.self_attn.k_norm.weight"])
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    # a Llama-family scorer keeps the Llama entry points
    from test_clm_llama_host import tiny_model
    m2, c2 = tiny_model("llama", n_layers=1)
    d2 = R.llama_dims(c2)
    s2 = R.LlamaScorer(d2, R.llama_device_layout(state_of(m2, False), d2, R.rope_inv_freq(c2)), "cpu")
    assert s2._family == "llama" and s2._qk == () and d2["qk_norm"] is False
