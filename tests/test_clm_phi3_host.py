"""Host-side checks of the Phi-3 rescorer (csrc/causal_lm_phi3.hip, "phi3" in llm_rescore; no GPU): the float64 restatement
of the contract (ref_logp_phi3, the reference of tests/test_gpu_clm_phi3.py) against HF's Phi3ForCausalLM evaluated in float64,
the preconditions of the GPU bounds (e16, e_bf16), that the attention factor, the short factors, the number of rotated dims and
the scale on the pass-through q dims all matter far beyond the bound, phi3_rope against HF's rotary module, the loader's device
layout against the state dict, the refusals, the descriptor's layout, the nine entry points' declarations, bindings, sizes and
refusals before any device work, the kernels of the translation unit and a scorer on the CPU.

The five tiny models (TINY) are random HF Phi3ForCausalLM built in memory with tiny_model's initialisation rule: 2 layers,
eager attention; head dim 96 with and without grouped queries (Phi-3-mini's layout; with 4 / 1 heads q | k is 480 columns wide,
so v shares a 64-column group of the QKV GEMM with k), head dim 128 with 96 rotated dims under LongRoPE (Phi-4-mini's layout:
short factors that differ from the long ones, original length 256 of 1024, attention factor sqrt(1 + ln 4 / ln 256)), head
dim 128 with the default rotation (Phi-3-medium / Phi-4), and `wide`, a head_dim field of its own with num_attention_heads *
head_dim (256) wider than hidden_size (192), which HF's Phi3Attention accepts though no published checkpoint has it."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, _model, state_of, tiny_seqs
from test_clm_mixtral_host import hf_logp_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHORT = [round(1.0 + 0.5 * i / 47, 4) for i in range(48)]
LONG = [round(2.0 + 3.0 * i / 47, 4) for i in range(48)]
TINY = {
    "hd96": dict(hidden_size=192, num_attention_heads=2, num_key_value_heads=2, intermediate_size=320, vocab_size=1003,
                 max_position_embeddings=256, tie_word_embeddings=False, rope_parameters=dict(rope_type="default", rope_theta=10000.0)),
    "hd96gqa": dict(hidden_size=384, num_attention_heads=4, num_key_value_heads=1, intermediate_size=448, vocab_size=777,
                    max_position_embeddings=4096, sliding_window=192, tie_word_embeddings=False,
                    rope_parameters=dict(rope_type="default", rope_theta=10000.0)),
    "partial": dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=192, vocab_size=515,
                    max_position_embeddings=1024, original_max_position_embeddings=256, partial_rotary_factor=0.75,
                    tie_word_embeddings=True,
                    rope_parameters=dict(rope_type="longrope", rope_theta=10000.0, short_factor=SHORT, long_factor=LONG,
                                         partial_rotary_factor=0.75, original_max_position_embeddings=256)),
    "hd128": dict(hidden_size=256, num_attention_heads=2, num_key_value_heads=1, intermediate_size=320, vocab_size=1003,
                  max_position_embeddings=256, tie_word_embeddings=True, rope_parameters=dict(rope_type="default", rope_theta=250000.0)),
    "wide": dict(hidden_size=192, num_attention_heads=2, num_key_value_heads=1, head_dim=128, intermediate_size=320, vocab_size=777,
                 max_position_embeddings=256, tie_word_embeddings=False, rope_parameters=dict(rope_type="default", rope_theta=10000.0)),
}
HEAD_DIM = {"hd96": 96, "hd96gqa": 96, "partial": 128, "hd128": 128, "wide": 128}
ROTARY = {"hd96": 96, "hd96gqa": 96, "partial": 96, "hd128": 128, "wide": 128}
MAX_POS = {"hd96": 256, "hd96gqa": 192, "partial": 256, "hd128": 256, "wide": 256}
HOST_LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
E_BF16_MAX = 0.1   # the precondition of the bf16 bound, as in tests/test_clm_llama_bf16_host.py
HF_BOUND = 1e-9    # the unrounded restatement is HF's forward evaluated in float64 (tests/test_clm_mixtral_host.py's bound)


def tiny_phi3(name, n_layers=2, fmt="float16", **over):
    """(HF fp32 CPU Phi3ForCausalLM in eval mode with random weights representable in fmt, its config as the dict of
    config.json); tiny_model's initialisation rule (tests/test_clm_llama_host.py)."""
    import torch
    import transformers
    kw = dict(TINY[name], rms_norm_eps=1e-5, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    kw.update(over)
    cfg = transformers.Phi3Config(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = transformers.Phi3ForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(700 + sorted(TINY).index(name))
    rdt = getattr(torch, fmt)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("norm.weight") or "layernorm" in k:
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif "embed_tokens" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            p.copy_(v.to(rdt).float())
    return model, json.loads(cfg.to_json_string())


def phi3_ref_dims(cfg, name):
    """What ref_logp_phi3 reads, from the config and the table above (not through llm_rescore.phi3_dims)."""
    return dict(n_layers=cfg["num_hidden_layers"], d_model=cfg["hidden_size"], n_heads=cfg["num_attention_heads"],
                n_kv_heads=cfg["num_key_value_heads"], head_dim=HEAD_DIM[name], rotary_dims=ROTARY[name],
                ffn_dim=cfg["intermediate_size"], vocab=cfg["vocab_size"], rms_eps=cfg["rms_norm_eps"])


def hf_rope(model):
    """(inv_freq, attention factor) of HF's rotary module: what phi3_rope restates"""
    re_ = model.model.rotary_emb
    return re_.inv_freq.detach().float().numpy().copy(), float(re_.attention_scaling)


def ref_logp_phi3(st, dims, rope, seqs, fmt=None, scale_pass=True):
    """The float64 restatement of include/b2t.h's Phi-3 contract from a state dict under HF's names (the fused qkv_proj and
    gate_up_proj, nothing permuted or interleaved); per sequence the log-probs (0 at the first token).  rope = (inv_freq
    [rotary_dims / 2], attention factor).  fmt = None rounds nowhere; "float16" / "bfloat16" round where the kernels round and
    nowhere else: the RMSNorm outputs; q after rotation (or pass-through) and the factor head_dim^-0.5; k after rotation (or
    pass-through); v; P per 32-key block; the attention output; silu(gate) * up -- and cos / sin are then the fp32 table's
    entries, the attention factor multiplied in fp32.  scale_pass=False leaves the pass-through q dims unscaled: another
    function, for the sensitivity test."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    rnd = (lambda t: t) if fmt is None else (lambda t: t.to(R.clm_dtype(fmt)).double())
    d, Hq, Hkv, hd, rt, nl, V, eps, Fd = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "head_dim", "rotary_dims", "n_layers",
                                                            "vocab", "rms_eps", "ffn_dim"))
    G = Hq // Hkv
    inv_freq, att = rope
    assert len(inv_freq) == rt // 2
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["model.embed_tokens.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    ang = pos.double()[:, None] * torch.as_tensor(np.asarray(inv_freq, np.float32), device=dev).double()[None, :]
    cos, sin = torch.cos(ang), torch.sin(ang)
    if fmt is None:
        cos, sin = cos * att, sin * att
    else:       # the fp32 table: the functions evaluated in double, rounded, times the factor in fp32
        a32 = torch.tensor(att, dtype=torch.float32, device=dev)
        cos, sin = (cos.float() * a32).double(), (sin.float() * a32).double()
    cos, sin = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]   # [M, 1, rt]

    def rot(t):   # the first rt dims rotated (HF's rotate_half on them), the others as they are
        a, b = t[..., :rt], t[..., rt:]
        return torch.cat([a * cos + torch.cat([-a[..., rt // 2:], a[..., :rt // 2]], -1) * sin, b], -1)
    qs = torch.full((hd,), hd ** -0.5, dtype=torch.float64, device=dev)
    if not scale_pass:
        qs[rt:] = 1.0
    rms = lambda t, w: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * W(w)
    lin = lambda t, p: t @ W(p + ".weight").T
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(rms(x, p + "input_layernorm.weight"))
        qkv = lin(h, p + "self_attn.qkv_proj")
        q = rnd(rot(qkv[:, :Hq * hd].view(M, Hq, hd)) * qs)
        k = rnd(rot(qkv[:, Hq * hd:(Hq + Hkv) * hd].view(M, Hkv, hd)))
        v = rnd(qkv[:, (Hq + Hkv) * hd:]).view(M, Hkv, hd)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)     # query head h reads kv head h // G
        o = torch.empty(M, Hq * hd, dtype=torch.float64, device=dev)
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
            o[sl] = ((pr @ v[sl].transpose(0, 1)) / lsum[..., None]).transpose(0, 1).reshape(n, Hq * hd)
        x = x + lin(rnd(o), p + "self_attn.o_proj")
        h = rnd(rms(x, p + "post_attention_layernorm.weight"))
        gu = lin(h, p + "mlp.gate_up_proj")
        gate, up = gu[:, :Fd], gu[:, Fd:]
        x = x + lin(rnd(gate * torch.sigmoid(gate) * up), p + "mlp.down_proj")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = rnd(rms(x[src], "model.norm.weight"))
    E = st["lm_head.weight"] if "lm_head.weight" in st else st["model.embed_tokens.weight"]
    logits = h @ E.double().T
    lp = (logits.gather(1, tgt[:, None])[:, 0] - torch.logsumexp(logits, -1)).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def phi3_state(name, fmt="float16", **kw):
    """(model, cfg, state dict (without lm_head where tied), reference dims, (inv_freq, attention factor) of HF's module)"""
    model, cfg = tiny_phi3(name, fmt=fmt, **kw)
    return model, cfg, state_of(model, cfg["tie_word_embeddings"]), phi3_ref_dims(cfg, name), hf_rope(model)


def _maxdiff(a, b):
    return float(max(np.abs(x - y).max() for x, y in zip(a, b)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_restatement(name):
    """Unrounded it is HF's forward evaluated in float64 within 1e-9, and the preconditions of the GPU bounds hold: 0 < e16,
    0 < e_bf16 <= 0.1, restatement against restatement.  Measured on the CPU with these seeds and lengths 1..129: see NOTES.md
    ("LLM")."""
    model, cfg, st, rd, rope = phi3_state(name)
    assert cfg["model_type"] == "phi3" and (rd["head_dim"] * rd["n_heads"] == rd["d_model"]) == (name != "wide")
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_phi3(st, rd, rope, seqs)
    hf = hf_logp_float64(model, seqs)
    err, mx = _maxdiff(exact, hf), max(np.abs(b).max() for b in hf)
    e16 = _maxdiff(ref_logp_phi3(st, rd, rope, seqs, "float16"), exact)
    print(f"CLM phi3 restatement {name}: vs HF's forward in float64 {err:.3e} (max |logp| {mx:.2f}), e16 {e16:.3e}")
    assert mx > 5 and err <= HF_BOUND, (name, err)
    assert 0 < e16, e16
    # bf16: the weights rounded to bf16 first, as the device holds them
    model, cfg, st, rd, rope = phi3_state(name, fmt="bfloat16")
    ebf = _maxdiff(ref_logp_phi3(st, rd, rope, seqs, "bfloat16"), ref_logp_phi3(st, rd, rope, seqs))
    print(f"CLM phi3 restatement {name}: e_bf16 {ebf:.3e}")
    assert 0 < ebf <= E_BF16_MAX, ebf


def test_what_phi3_adds_matters_far_beyond_the_bound():
    """On `partial`, reference against reference: without the attention factor, with the long factors, rotating all 128 dims, or
    leaving the pass-through q dims unscaled, a log-prob moves by more than 10 x the fp16 bound min(3 e16, 1e-2).  That is what
    makes meeting the contract mean that the right forward was built."""
    import llm_rescore as R
    model, cfg, st, rd, (inv, att) = phi3_state("partial")
    assert att == math.sqrt(1 + math.log(4) / math.log(256)) and len(inv) == 48 and SHORT != LONG
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_phi3(st, rd, (inv, att), seqs)
    e16 = _maxdiff(ref_logp_phi3(st, rd, (inv, att), seqs, "float16"), exact)
    bound = min(3 * e16, 1e-2)
    long_cfg = json.loads(json.dumps(cfg))
    long_cfg["rope_parameters"]["short_factor"] = LONG
    inv128 = R.phi3_rope(cfg | {"partial_rotary_factor": 1.0, "rope_parameters": {"rope_type": "default", "rope_theta": 10000.0}})[0]
    assert len(inv128) == 64
    moved = {
        "no attention factor": _maxdiff(exact, ref_logp_phi3(st, rd, (inv, 1.0), seqs)),
        "long factors": _maxdiff(exact, ref_logp_phi3(st, rd, (R.phi3_rope(long_cfg)[0], att), seqs)),
        "all 128 dims rotated": _maxdiff(exact, ref_logp_phi3(st, rd | {"rotary_dims": 128}, (inv128, att), seqs)),
        "pass-through q dims unscaled": _maxdiff(exact, ref_logp_phi3(st, rd, (inv, att), seqs, scale_pass=False)),
    }
    print(f"CLM phi3 sensitivity partial: e16 {e16:.3e}, bound {bound:.3e}; " + ", ".join(f"{k} {v:.3f}" for k, v in moved.items()))
    for k, v in moved.items():
        assert v > 10 * bound, (k, v, bound)


@pytest.mark.parametrize("name", list(TINY))
def test_phi3_rope_is_hfs(name):
    """inv_freq and the attention factor equal HF's rotary module's bit for bit, from config.json's spelling and from the older
    one (rope_scaling with type "su", rope_theta / partial_rotary_factor / original_max_position_embeddings at the top level)."""
    import llm_rescore as R
    model, cfg = tiny_phi3(name, n_layers=1)
    inv, att = hf_rope(model)
    got, gatt = R.phi3_rope(cfg)
    assert got.dtype == np.float32 and got.shape == (ROTARY[name] // 2,) and got.tobytes() == inv.tobytes() and gatt == att
    assert (att == 1.0) == (name != "partial")
    rp = dict(cfg["rope_parameters"])
    old = {k: v for k, v in cfg.items() if k != "rope_parameters"} | {"rope_theta": rp.pop("rope_theta")}
    if name == "partial":
        assert old["partial_rotary_factor"] == 0.75 and old["original_max_position_embeddings"] == 256
        old["rope_scaling"] = {"type": "su", "short_factor": rp["short_factor"], "long_factor": rp["long_factor"]}
        given = R.phi3_rope(cfg | {"rope_parameters": dict(cfg["rope_parameters"], factor=16.0)})
        assert given[1] == math.sqrt(1 + math.log(16) / math.log(256)) and given[0].tobytes() == inv.tobytes()
        assert R.phi3_rope(cfg | {"rope_parameters": dict(cfg["rope_parameters"], attention_factor=1.5)})[1] == 1.5
        assert R.phi3_rope(cfg | {"max_position_embeddings": 256})[1] == 1.0        # factor 1: no scaling
    got, gatt = R.phi3_rope(old)
    assert got.tobytes() == inv.tobytes() and gatt == att
    assert R.phi3_dims(old) == R.phi3_dims(cfg)


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict(name, fmt, tmp_path):
    """Every array equals its state-dict tensor bit for bit: qkv_proj as stored (no permutation), gate / up interleaved in
    blocks of 32 from the fused tensor's halves, the head tied or not, rows padded to 256 with zeros; the rotary tables have
    pitch rotary_dims / 2 and carry the attention factor."""
    import torch
    import llm_rescore as R
    model, cfg = tiny_phi3(name, fmt=fmt)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_phi3_arrays(str(tmp_path), dtype=fmt)
    sd = model.state_dict()
    rd = phi3_ref_dims(cfg, name)
    wdt = getattr(torch, fmt)
    assert dims == R.phi3_dims(cfg) and dims["max_pos"] == MAX_POS[name] and dims["tied"] is cfg["tie_word_embeddings"]
    for k in rd:
        assert dims[k] == rd[k], k
    d, Hq, Hkv, Fd, V, hd, rt = (rd[k] for k in ("d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab", "head_dim", "rotary_dims"))
    eq = lambda a, b: a.dtype == wdt and torch.equal(a, b.to(wdt)) and torch.equal(a.float(), b)   # bit for bit, and exact
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert not arr["embed_tokens"][V:].any()
    if cfg["tie_word_embeddings"]:
        assert arr["lm_head"] is arr["embed_tokens"]
    else:
        assert arr["lm_head"].shape == (Vp, d) and eq(arr["lm_head"][:V], sd["lm_head.weight"]) and not arr["lm_head"][V:].any()
        assert not torch.equal(arr["lm_head"], arr["embed_tokens"])
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    inv, att = hf_rope(model)
    cos, sin = R.rope_tables(inv, MAX_POS[name])
    assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (MAX_POS[name], rt // 2)
    assert np.array_equal(arr["rope_cos"].numpy(), cos * np.float32(att)) and np.array_equal(arr["rope_sin"].numpy(), sin * np.float32(att))
    assert (arr["rope_cos"][0] == np.float32(att)).all()
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        assert eq(a("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(a("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any() and eq(w[:qw], sd[p + "self_attn.qkv_proj.weight"])
        assert f"layers.{l}.qkv_b" not in arr
        dp = -(-d // 256) * 256
        assert a("o_w").shape == (dp, Hq * hd) and eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and not a("o_w")[d:].any()
        gu = a("gate_up_w")
        assert gu.shape == (-(-2 * Fd // 256) * 256, d) and not gu[2 * Fd:].any()
        blocks = gu[:2 * Fd].view(Fd // 32, 2, 32, d)
        fused = sd[p + "mlp.gate_up_proj.weight"]
        assert eq(blocks[:, 0].reshape(Fd, d), fused[:Fd]) and eq(blocks[:, 1].reshape(Fd, d), fused[Fd:])
        assert a("down_w").shape == (dp, Fd) and eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"])
    for t in arr.values():
        assert t.is_contiguous()


def test_refusals(tmp_path):
    import llm_rescore as R
    model, cfg = tiny_phi3("partial", n_layers=1)
    with pytest.raises(ValueError, match="model_type 'phi3'"):       # llama_dims stays as it is
        R.llama_dims(cfg)
    with pytest.raises(ValueError, match="rope_type 'longrope'"):    # and so does rope_inv_freq
        R.rope_inv_freq(cfg)
    n = [0]

    def both(match, c):
        with pytest.raises(ValueError, match=match):
            R.phi3_dims(c)
        n[0] += 1
        sub = tmp_path / f"r{n[0]}"
        os.makedirs(sub)
        with open(sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(sub), device="cpu")
    rp = cfg["rope_parameters"]
    plain = {k: v for k, v in cfg.items() if k not in ("rope_parameters", "partial_rotary_factor",
                                                       "original_max_position_embeddings")} | {"rope_theta": 10000.0}
    assert R.phi3_dims(plain)["rotary_dims"] == 128
    both("hidden_act", cfg | {"hidden_act": "gelu"})
    both("head_dim 32 ", plain | {"num_attention_heads": 8, "num_key_value_heads": 8})
    both("head_dim 256 ", plain | {"head_dim": 256})
    both("head_dim 80 ", plain | {"head_dim": 80})
    both("not a multiple of num_attention_heads", plain | {"num_attention_heads": 3, "num_key_value_heads": 3})
    both("partial_rotary_factor gives 95 rotary dims", plain | {"partial_rotary_factor": 0.745})
    both("partial_rotary_factor gives 0 rotary dims", plain | {"partial_rotary_factor": 0.001})
    both("partial_rotary_factor gives 192 rotary dims", plain | {"partial_rotary_factor": 1.5})
    both("hidden_size 200, intermediate_size 192, num_attention_heads \\* head_dim 256 and .* must be multiples of 64",
         plain | {"hidden_size": 200, "head_dim": 128})
    both("intermediate_size 300.* must be multiples of 64", plain | {"intermediate_size": 300})
    both("num_attention_heads \\* head_dim 288 .* must be multiples of 64", plain | {"hidden_size": 320, "num_attention_heads": 3,
                                                                                      "num_key_value_heads": 3, "head_dim": 96})
    both("num_key_value_heads", plain | {"num_attention_heads": 4, "num_key_value_heads": 3, "head_dim": 64})
    both("short_factor has 47 entries", cfg | {"rope_parameters": dict(rp, short_factor=SHORT[:47])})
    both("short_factor has 0 entries", cfg | {"rope_parameters": {k: v for k, v in rp.items() if k != "short_factor"}})
    both("rope_type 'yarn'", plain | {"rope_scaling": {"rope_type": "yarn", "factor": 2.0}})
    both("rope_type 'linear'", plain | {"rope_scaling": {"type": "linear", "factor": 2.0}})
    both("rope_type 'llama3'", plain | {"rope_scaling": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                         "high_freq_factor": 4.0, "original_max_position_embeddings": 64}})
    # max_pos: the smallest of max_position_embeddings, the window, the original length of a longrope model, and the cap
    assert R.phi3_dims(cfg)["max_pos"] == 256
    assert R.phi3_dims(cfg, max_positions=100)["max_pos"] == 100
    assert R.phi3_dims(cfg | {"sliding_window": 192})["max_pos"] == 192
    assert R.phi3_dims(cfg | {"sliding_window": 2047})["max_pos"] == 256
    big = cfg | {"max_position_embeddings": 131072, "original_max_position_embeddings": 4096,
                 "rope_parameters": dict(rp, original_max_position_embeddings=4096)}
    assert R.phi3_dims(big)["max_pos"] == 4096 and R.phi3_dims(big, max_positions=1 << 20)["max_pos"] == 4096
    assert R.phi3_dims(big | {"sliding_window": 2047})["max_pos"] == 2047
    assert R.phi3_dims(plain | {"max_position_embeddings": 131072})["max_pos"] == R.LLAMA_MAX_POSITIONS
    assert R.phi3_dims(plain | {"max_position_embeddings": 131072, "original_max_position_embeddings": 4096},
                       max_positions=1 << 20)["max_pos"] == 131072           # not longrope: the original length binds nothing
    with pytest.raises(ValueError, match="max_positions"):
        R.phi3_dims(cfg, max_positions=0)
    # the neighbours stay unsupported model types, and the refusal lists phi3 in the middle
    for mt in ("phi", "phimoe", "phi3small", "phi4_multimodal"):
        with pytest.raises(ValueError, match=f"model_type '{mt}'"):
            R.phi3_dims(cfg | {"model_type": mt})
        os.makedirs(tmp_path / mt)
        with open(tmp_path / mt / "config.json", "w") as f:
            json.dump(cfg | {"model_type": mt}, f)
        with pytest.raises(ValueError, match=f"model_type '{mt}' is not supported") as ei:
            R.build_scorer(str(tmp_path / mt), device="cpu")
        msg = str(ei.value)
        assert "(opt, gpt2, gpt_neox, llama" in msg and msg.endswith("olmo2, mixtral)") and ", gemma2, " in msg and ", phi3, " in msg
    # a Phi-3 directory without weights gets as far as the weights; bf16 with a cache is refused before that
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    with pytest.raises(ValueError, match="follow-up"):
        R.build_scorer(str(bare), device="cuda", dtype="bfloat16", context_cache_tokens=64)
    # the layout: the fused tensors are required, any bias is refused by name, shapes are checked
    st = state_of(model, True)
    dims, rope = R.phi3_dims(cfg), R.phi3_rope(cfg)
    for lack in ("qkv_proj", "gate_up_proj", "post_attention_layernorm", "input_layernorm", "o_proj", "down_proj"):
        with pytest.raises(KeyError, match=lack):
            R.phi3_device_layout({k: v for k, v in st.items() if lack not in k}, dims, rope)
    for b in ("self_attn.qkv_proj.bias", "self_attn.o_proj.bias", "mlp.gate_up_proj.bias", "mlp.down_proj.bias"):
        with pytest.raises(ValueError, match=b):
            R.phi3_device_layout(dict(st, **{"model.layers.0." + b: st["model.norm.weight"]}), dims, rope)
    with pytest.raises(ValueError, match="qkv_proj.weight: shape"):
        R.phi3_device_layout(dict(st, **{"model.layers.0.self_attn.qkv_proj.weight": st["model.layers.0.self_attn.qkv_proj.weight"][:384]}),
                             dims, rope)
    with pytest.raises(ValueError, match="inv_freq has 64 entries"):
        R.phi3_device_layout(st, dims, (np.ones(64, np.float32), 1.0))
    untied = R.phi3_device_layout(dict(st, **{"lm_head.weight": st["model.embed_tokens.weight"] * 2}), dims | {"tied": False}, rope)
    assert untied["lm_head"] is not untied["embed_tokens"]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")
SIZES = ("ws_bytes", "tree_ws_bytes", "cache_kv_bytes", "tree_cached_ws_bytes")


def _p3(hd=64, rot=None):
    import b2t_native as N
    return N.ClmPhi3(hd, hd if rot is None else rot)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_struct_layout_matches_the_header(tmp_path):
    import b2t_native as N
    src = tmp_path / "lay.c"
    fd = [n for n, _ in N.ClmPhi3._fields_]
    body = "".join(f'printf("D.{f} %zu\\n", offsetof(b2t_clm_phi3_t, {f}));' for f in fd)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){'
                   'printf("D %zu\\n", sizeof(b2t_clm_phi3_t));' + body + "return 0;}")
    exe = tmp_path / "lay"
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["D"]) == C.sizeof(N.ClmPhi3) == 8
    for f in fd:
        assert int(got["D." + f]) == getattr(N.ClmPhi3, f).offset, f
    assert fd == ["head_dim", "rotary_dims"]


def test_entry_points_are_declared_and_bound():
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY + SIZES:     # the Gemma-2 twin's list with phi3 in place of g2
        new, twin = "b2t_clm_phi3_" + t, "b2t_clm_gemma2_" + t
        want = decl(twin)
        assert want[1] == "const b2t_clm_gemma2_t* g2"
        assert decl(new) == want[:1] + ["const b2t_clm_phi3_t* phi3"] + want[2:], new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == [g.argtypes[0], C.POINTER(N.ClmPhi3)] + list(g.argtypes[2:])
    assert sorted(re.findall(r"\b(b2t_clm_phi3_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) == \
        sorted("b2t_clm_phi3_" + t for t in ENTRY + SIZES)
    assert set("b2t_clm_phi3_" + t for t in ENTRY + SIZES) <= set(N.header_symbols())


def test_sizes():
    """The workspace is the Llama layout at the same widths plus the fp32 region [round_up(rows, 256)][(Hq + Hkv) hd]; the cached
    call adds the state of stage B; the cache's bytes use the descriptor's head dim; invalid arguments give 0."""
    lib = __import__("b2t_native").load()
    al = lambda x: -(-x // 256) * 256
    for d, H, kv, hd in ((192, 2, 2, 96), (384, 4, 1, 96), (256, 2, 1, 128), (256, 4, 2, 64), (3072, 32, 32, 96)):
        desc, g = _model(bias=False, d=d, heads=H, kv=kv), _p3(hd, hd - 32)
        p = C.byref(desc)
        for M in (1, 2, 255, 256, 257, 692):
            for n_seq in sorted({1, max(1, M // 3), M}):
                for rows in sorted({1, M // 2 + 1, M}):
                    extra = al(4 * al(rows) * (H + kv) * hd)
                    got = lib.b2t_clm_phi3_tree_ws_bytes(p, g, rows, M, n_seq)
                    assert got == lib.b2t_clm_llama_tree_ws_bytes(p, rows, M, n_seq) + extra      # H hd == d: the Llama twin's widths
                    assert lib.b2t_clm_phi3_tree_cached_ws_bytes(p, g, rows, M, n_seq) == got + al(4 * rows * H * 2) + al(4 * rows * H * hd)
                assert lib.b2t_clm_phi3_ws_bytes(p, g, M, n_seq) == lib.b2t_clm_llama_ws_bytes(p, M, n_seq) + al(4 * al(M) * (H + kv) * hd)
        for cap in (1, 8, 64):
            assert lib.b2t_clm_phi3_cache_kv_bytes(p, g, cap) == desc.n_layers * cap * 2 * kv * hd * 2
        assert lib.b2t_clm_phi3_cache_kv_bytes(p, g, 0) == 0 and lib.b2t_clm_phi3_cache_kv_bytes(p, g, 65) == 0
    # a head dim of its own: d = 256 with 4 heads of 128 has the QKV rows of the Llama shape d = 512
    narrow, wide, g = _model(bias=False, d=256, heads=4, kv=2), _model(bias=False, d=512, heads=4, kv=2), _p3(128)
    a, b = lib.b2t_clm_phi3_ws_bytes(C.byref(narrow), g, 692, 12), lib.b2t_clm_phi3_ws_bytes(C.byref(wide), g, 692, 12)
    assert al(2 * 692 * 8 * 128) + al(4 * 768 * 6 * 128) < a < b
    desc, g = _model(bias=False), _p3()
    p = C.byref(desc)
    assert lib.b2t_clm_phi3_ws_bytes(None, g, 10, 1) == 0 and lib.b2t_clm_phi3_ws_bytes(p, None, 10, 1) == 0
    assert lib.b2t_clm_phi3_tree_ws_bytes(p, None, 5, 10, 1) == 0 and lib.b2t_clm_phi3_cache_kv_bytes(p, None, 4) == 0
    assert lib.b2t_clm_phi3_tree_cached_ws_bytes(None, g, 5, 10, 1) == 0
    for hd in (0, 32, 80, 256):
        assert lib.b2t_clm_phi3_ws_bytes(p, _p3(hd), 10, 1) == 0 and lib.b2t_clm_phi3_cache_kv_bytes(p, _p3(hd), 4) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert lib.b2t_clm_phi3_ws_bytes(p, g, n_tok, n_seq) == 0, (n_tok, n_seq)
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert lib.b2t_clm_phi3_tree_ws_bytes(p, g, nn, nt, ns) == 0, (nn, nt, ns)
        assert lib.b2t_clm_phi3_tree_cached_ws_bytes(p, g, nn, nt, ns) == 0, (nn, nt, ns)


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """The family's model check, the descriptor's refusals and the list's, with fake pointers and no GPU; every message but the
    flat and tree calls' "null model" carries the entry point's name; on the cached call the cache is left as it was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_phi3_" + entry
    fn = getattr(lib, who)
    tree, cached = "tree" in entry, "cached" in entry
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]
    nb = lambda **kw: _model(bias=False, **kw)
    NOG = object()

    def refused(match, desc, g=NOG, ids=ok_ids, off=ok_off, own=True, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None,
                cache=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        n = len(off) - 1 if n_seq is None else n_seq
        dp = C.byref(desc) if desc is not None else None
        g = _p3() if g is NOG else g
        if cached:
            cache = _cache() if cache is None else cache
            n0, ids0 = cache.n, cache._keep.copy()
            rc = fn(dp, g, C.byref(cache), update, ids.ctypes.data, off.ctypes.data, n, scores, None, None, None, ws, ws_bytes, None)
            assert cache.n == n0 and (cache._keep == ids0).all()     # a refusal leaves the cache alone
        elif tree:
            rc = fn(dp, g, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
        else:
            rc = fn(dp, g, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        if own:
            assert N.last_error().startswith(who + ":"), N.last_error()

    # the model's and the descriptor's (the default model: d 256, 4 heads, 2 kv heads; the default descriptor: head dim 64)
    refused("null model", None, own=cached)
    refused("null phi3 descriptor", nb(), g=None)
    for hd in (0, 32, 80, 192, 256):
        refused(f"unsupported head dim {hd} ", nb(), g=_p3(hd))
    for hd, rot in ((64, 0), (64, 1), (64, 63), (64, 66), (96, 98), (128, 95), (128, -2)):
        refused(f"rotary_dims {rot} is not an even number in \\[2, head_dim {hd}\\]", nb(d=hd * 4), g=_p3(hd, rot))
    refused("d_model 200, .* must be multiples of 64", nb(d=200))
    refused("ffn_dim 500, .* must be multiples of 64", nb(ffn=500))
    refused("n_heads \\* head_dim 288 and \\(n_heads \\+ 2 n_kv_heads\\) \\* head_dim 864 must be multiples of 64",
            nb(d=320, heads=3, kv=3), g=_p3(96))
    refused("n_heads 8 is not a multiple of n_kv_heads 3", nb(d=512, heads=8, kv=3))
    refused("layer 0 has q / k / v biases", _model(bias=True))
    two = _model(bias=False, n_layers=2)
    two.layers_host[1].qkv_b = FAKE
    refused("layer 1 has q / k / v biases", two)
    refused("bad dimensions", nb(kv=0))
    refused("bad dimensions", nb(max_pos=0))
    refused("rms_eps", nb(eps=-1.0))
    refused("null weight", N.ClmLlamaDesc(0, 256, 4, 2, 512, 1000, 64, 1e-5, FAKE, FAKE, FAKE, FAKE, 0, None))
    bad = nb()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad)
    # the list's: every accepted head dim and a partial rotation get that far
    refused("null argument", nb(), scores=None)
    refused("null argument", nb(d=192, heads=2, kv=2), g=_p3(96), ws=None)
    refused("null argument", nb(d=256, heads=2, kv=1), g=_p3(128, 96), ws=None)
    refused("null argument", nb(d=256, heads=4, kv=2), g=_p3(128, 2), ws=None)     # a head dim that is not d_model / n_heads
    refused("n_seq 0", nb(), n_seq=0)
    refused("empty", nb(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", nb(), off=[1, 2, 4])
    refused("outside", nb(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", nb(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4], cache=_cache(cap=3) if cached else None)
    # the workspace: this family's size functions
    desc, g = nb(d=192, heads=2, kv=2), _p3(96, 48)
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes, trunk 2
    if cached:
        need = lib.b2t_clm_phi3_tree_cached_ws_bytes(C.byref(desc), g, 4, 9, 3)
        refused("workspace", desc, g=g, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_phi3_tree_cached_ws_bytes(C.byref(desc), g, 3, 9, 3)
        refused("workspace", desc, g=g, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("null cache member", desc, g=g, cache=_cache(kv=None))
        refused("above max_pos", nb(max_pos=64), cache=_cache(cap=65))
        refused("cached token 1 has id 1000", nb(vocab=1000), cache=_cache(ids=(2, 1000)))
        rc = fn(C.byref(desc), g, None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1, FAKE, None, None, None,
                FAKE, 1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_phi3_score_tree_f16", N.last_error())
    elif tree:
        need = lib.b2t_clm_phi3_tree_ws_bytes(C.byref(desc), g, 4, 9, 3)
        assert need > 0
        refused("workspace", desc, g=g, ids=ids, off=off, ws_bytes=need - 1)
    else:
        need = lib.b2t_clm_phi3_ws_bytes(C.byref(desc), g, 9, 3)
        assert need > 0
        refused("workspace", desc, g=g, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_phi3_unit_kernels_without_scratch():
    """The unit instantiates the EP_QKV_F32 epilogue (11) on two tiles, the rotation kernel and the flat and tree attention at
    head dim 96, each in two element types, and the cached and trunk attention at 96 in fp16: 12 kernels.  None uses scratch,
    and none asks for more registers than a lane has.  Read from the compiler's resource report alone."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_phi3.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_phi3.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_kernel" in k]
    attn = [k for k in res if "clm_attn" in k]
    assert len(res) == 12 and len(gemm) == 4 and len(attn) == 6, sorted(res)
    assert all(re.search(r"(ELi11E|, ?11,)", k) for k in gemm), gemm
    assert all(re.search(r"(ILi96E|<96)", k) for k in attn), attn
    for kern, count in (("clm_phi3_rope_kernel", 2), ("clm_attn_kernel", 2), ("clm_attn_tree_kernel", 2),
                        ("clm_attn_tree_cached_kernel", 1), ("clm_attn_trunk_kernel", 1)):
        assert sum(kern in k for k in res) == count, (kern, sorted(res))
    for k in sorted(res):
        print(f"CLM phi3 {k[:100]}: {res[k]}")
    assert all(v.get("ScratchSize", -1) == 0 for v in res.values()), res
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_phi3.hip")).read()
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src        # the one tile rule
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_QKV_F32, El>)") == 1


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_phi3("partial", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    sd = {k: v.float() for k, v in model.state_dict().items()}
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.Phi3Scorer) and isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu"
        assert sc._family == "phi3" and sc._SIZES == "b2t_clm_phi3_" and R.LlamaScorer._SIZES == "b2t_clm_llama_"
        assert sc.desc.n_heads == 2 and sc.desc.n_kv_heads == 1 and sc.desc.d_model == 256 and sc.desc.vocab == 515
        assert sc.desc.lm_head == sc.desc.embed_tokens and not sc.desc.layers_host[0].qkv_b and sc.desc.max_pos == 256
        assert sc._phi3.head_dim == 128 and sc._phi3.rotary_dims == 96 and sc._size_args == (sc._phi3,) and sc._qk == (sc._phi3,)
        for l in range(2):
            assert sc.desc.layers_host[l].qkv_w == sc.w[f"layers.{l}.qkv_w"].data_ptr()
            assert sc.w[f"layers.{l}.qkv_w"].shape == (512, 256) and sc.w[f"layers.{l}.gate_up_w"].shape == (512, 256)
        assert sc.w["rope_cos"].shape == (256, 48)
        if want is torch.bfloat16:     # a bf16 checkpoint's values are kept exactly
            assert torch.equal(sc.w["layers.1.qkv_w"].float(), sd["model.layers.1.self_attn.qkv_proj.weight"])
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    assert R.build_scorer(str(tmp_path), device="cpu", max_positions=100).desc.max_pos == 100
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    with pytest.raises(ValueError, match="follow-up"):
        R.build_scorer(str(tmp_path), device="cuda", dtype="auto", context_cache_tokens=64)
    # Llama arrays are not Phi-3 arrays
    from test_clm_llama_host import tiny_model
    m2, c2 = tiny_model("llama", n_layers=1)
    d2 = R.llama_dims(c2)
    with pytest.raises(KeyError, match="head_dim"):
        R.Phi3Scorer(d2, R.llama_device_layout(state_of(m2, False), d2, R.rope_inv_freq(c2)), "cpu")
