"""Host-side checks of the Gemma-2 rescorer (csrc/causal_lm_gemma2.hip, "gemma2" in llm_rescore; no GPU): the float64
restatement of the contract (ref_logp_gemma2, the reference of tests/test_gpu_clm_gemma2.py) against HF's Gemma2ForCausalLM
evaluated in float64, the preconditions of the GPU bounds (e16, e_bf16), that both soft caps matter for these models, the
loader's device layout against the state dict, the refusals, the descriptor's layout, the nine entry points' declarations,
bindings, sizes and refusals before any device work, the kernels of the translation unit and a scorer on the CPU.

The two tiny models (TINY) are random HF Gemma2ForCausalLM built in memory: 2 layers (one sliding, one full), eager attention,
head dims 256 and 128 with num_attention_heads * head_dim (512) wider than hidden_size (128, 192), group size 2,
query_pre_attn_scalar different from head_dim, every norm weight 0.2 N(0, 1) -- so 1 + w and w cannot be confused -- and caps
of 2.0 / 3.0 instead of the published 50 / 30, which a tiny random model barely touches."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, _model, hf_inv_freq, state_of, tiny_seqs
from test_clm_mixtral_host import hf_logp_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TINY = {
    "hd256": dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, head_dim=256, intermediate_size=320,
                  vocab_size=777, query_pre_attn_scalar=144),
    "hd128": dict(hidden_size=192, num_attention_heads=4, num_key_value_heads=2, head_dim=128, intermediate_size=448,
                  vocab_size=1003, query_pre_attn_scalar=100),
}
COMMON = dict(max_position_embeddings=256, sliding_window=256, attn_logit_softcapping=2.0, final_logit_softcapping=3.0,
              rms_norm_eps=1e-6)
HOST_LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
E_BF16_MAX = 0.1   # the precondition of the bf16 bound, as in tests/test_clm_llama_bf16_host.py
HF_BOUND = 1e-9    # the unrounded restatement is HF's forward evaluated in float64 (tests/test_clm_mixtral_host.py's bound)
CAP_MIN = 0.1      # dropping either cap must move a log-prob by at least this much, or no tolerance would see a missing cap


def tiny_gemma2(name, n_layers=2, fmt="float16", **over):
    """(HF fp32 CPU Gemma2ForCausalLM in eval mode with random weights representable in fmt, its config as the dict of
    config.json).  Every norm weight is 0.2 N(0, 1): the model multiplies by 1 + w."""
    import torch
    import transformers
    kw = dict(TINY[name], **COMMON)
    kw.update(over)
    cfg = transformers.Gemma2Config(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = transformers.Gemma2ForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(500 + sorted(TINY).index(name))
    rdt = getattr(torch, fmt)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("norm.weight") or "layernorm" in k:
                v = 0.2 * torch.randn(p.shape, generator=g)
            elif "embed_tokens" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            p.copy_(v.to(rdt).float())
    return model, json.loads(cfg.to_json_string())


def gemma2_ref_dims(cfg):
    """What ref_logp_gemma2 reads, straight from the config (not through llm_rescore.gemma2_dims)."""
    return dict(n_layers=cfg["num_hidden_layers"], d_model=cfg["hidden_size"], n_heads=cfg["num_attention_heads"],
                n_kv_heads=cfg["num_key_value_heads"], head_dim=cfg["head_dim"], ffn_dim=cfg["intermediate_size"],
                vocab=cfg["vocab_size"], rms_eps=cfg["rms_norm_eps"], q_scale=cfg["query_pre_attn_scalar"] ** -0.5,
                attn_cap=cfg["attn_logit_softcapping"] or 0.0, final_cap=cfg["final_logit_softcapping"] or 0.0)


def ref_logp_gemma2(st, dims, inv_freq, seqs, fmt=None, w_not_1p=False):
    """The float64 restatement of include/b2t.h's Gemma-2 contract.  fmt = None rounds nowhere (the embedding's factor is then
    sqrt(d) as fp32 holds it, HF's buffer); "float16" / "bfloat16" round where the kernels round: that factor once; the two
    pre-norm outputs and the final norm's; q after rotation and scale; k after rotation; v; P per 32-key block; the attention
    output; gelu_tanh(gate) * up -- and never the o_proj / down outputs, which the post-norms read unrounded, nor the residual.
    A cap of 0 in dims is off.  w_not_1p=True multiplies by w where the model multiplies by 1 + w: another function, for the
    planted test."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    rnd = (lambda t: t) if fmt is None else (lambda t: t.to(R.clm_dtype(fmt)).double())
    d, Hq, Hkv, hd, nl, V, eps = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "head_dim", "n_layers", "vocab", "rms_eps"))
    G, c_a, c_f = Hq // Hkv, float(dims["attn_cap"]), float(dims["final_cap"])
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
    one = 0.0 if w_not_1p else 1.0
    rms = lambda t, w: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * (one + W(w))
    lin = lambda t, p: t @ W(p + ".weight").T
    gelu = lambda t: 0.5 * t * (1.0 + torch.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))
    scale = float(np.float32(float(d) ** 0.5)) if fmt is None else R.gemma2_embed_scale(d, fmt)
    x = W("model.embed_tokens.weight")[ids] * scale
    M = x.shape[0]
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(rms(x, p + "input_layernorm.weight"))
        q = rnd(rot(lin(h, p + "self_attn.q_proj").view(M, Hq, hd)) * dims["q_scale"])
        k = rnd(rot(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd)))
        v = rnd(lin(h, p + "self_attn.v_proj")).view(M, Hkv, hd)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)     # query head h reads kv head h // G
        o = torch.empty(M, Hq * hd, dtype=torch.float64, device=dev)
        for j in range(B):                                              # one sequence at a time: these are tiny
            n = lens[j]
            sl = slice(off[j], off[j + 1])
            s = q[sl].transpose(0, 1) @ k[sl].transpose(0, 1).transpose(1, 2)      # [Hq, n, n]
            if c_a > 0:
                s = c_a * torch.tanh(s / c_a)
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
        x = x + rms(lin(rnd(o), p + "self_attn.o_proj"), p + "post_attention_layernorm.weight")
        h = rnd(rms(x, p + "pre_feedforward_layernorm.weight"))
        a = rnd(gelu(lin(h, p + "mlp.gate_proj")) * lin(h, p + "mlp.up_proj"))
        x = x + rms(lin(a, p + "mlp.down_proj"), p + "post_feedforward_layernorm.weight")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = rnd(rms(x[src], "model.norm.weight"))
    logits = h @ W("model.embed_tokens.weight").T                      # the tied head
    if c_f > 0:
        logits = c_f * torch.tanh(logits / c_f)
    lp = (logits.gather(1, tgt[:, None])[:, 0] - torch.logsumexp(logits, -1)).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def gemma2_state(name, fmt="float16", **kw):
    """(model, cfg, state dict without the tied lm_head, reference dims, inv_freq)"""
    model, cfg = tiny_gemma2(name, fmt=fmt, **kw)
    return model, cfg, state_of(model, True), gemma2_ref_dims(cfg), hf_inv_freq(model)


def _maxdiff(a, b):
    return float(max(np.abs(x - y).max() for x, y in zip(a, b)))


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_restatement(name):
    """Unrounded it is HF's forward evaluated in float64 within 1e-9; dropping either cap moves a log-prob by at least 0.1;
    multiplying by w instead of 1 + w is another function; and the preconditions of the GPU bounds hold: 0 < e16,
    0 < e_bf16 <= 0.1, restatement against restatement.  Measured on the CPU with these seeds and lengths 1..129 (hd256 /
    hd128): see NOTES.md ("LLM")."""
    model, cfg, st, rd, inv = gemma2_state(name)
    assert cfg["layer_types"] == ["sliding_attention", "full_attention"] and cfg["model_type"] == "gemma2"
    assert cfg["query_pre_attn_scalar"] != cfg["head_dim"] and cfg["num_attention_heads"] * cfg["head_dim"] != cfg["hidden_size"]
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_gemma2(st, rd, inv, seqs)
    hf = hf_logp_float64(model, seqs)
    err, mx = _maxdiff(exact, hf), max(np.abs(b).max() for b in hf)
    no_a = _maxdiff(exact, ref_logp_gemma2(st, rd | {"attn_cap": 0.0}, inv, seqs))
    no_f = _maxdiff(exact, ref_logp_gemma2(st, rd | {"final_cap": 0.0}, inv, seqs))
    no_1p = _maxdiff(exact, ref_logp_gemma2(st, rd, inv, seqs, w_not_1p=True))
    e16 = _maxdiff(ref_logp_gemma2(st, rd, inv, seqs, "float16"), exact)
    print(f"CLM gemma2 restatement {name}: vs HF's forward in float64 {err:.3e} (max |logp| {mx:.2f}), without the attention cap "
          f"{no_a:.3f}, without the final cap {no_f:.3f}, w for 1 + w {no_1p:.3f}, e16 {e16:.3e}")
    assert mx > 5 and err <= HF_BOUND, (name, err)
    assert no_a >= CAP_MIN and no_f >= CAP_MIN and no_1p >= CAP_MIN, (no_a, no_f, no_1p)
    assert 0 < e16, e16
    # bf16: the weights rounded to bf16 first, as the device holds them
    model, cfg, st, rd, inv = gemma2_state(name, fmt="bfloat16")
    ebf = _maxdiff(ref_logp_gemma2(st, rd, inv, seqs, "bfloat16"), ref_logp_gemma2(st, rd, inv, seqs))
    print(f"CLM gemma2 restatement {name}: e_bf16 {ebf:.3e}")
    assert 0 < ebf <= E_BF16_MAX, ebf


# ---- the loader --------------------------------------------------------------------------------------------------------
def test_head_perm_puts_rotary_pairs_32_apart():
    import llm_rescore as R
    assert np.array_equal(R.gemma2_head_perm(128), R.head_dim_perm(128))
    for hd in (128, 256):
        p = R.gemma2_head_perm(hd)
        assert sorted(p) == list(range(hd))
        for j in range(hd // 64):     # the 64-row slice j: lane li holds dims (32 j + li, hd / 2 + 32 j + li), frequency 32 j + li
            assert np.array_equal(p[64 * j:64 * j + 32], 32 * j + np.arange(32))
            assert np.array_equal(p[64 * j + 32:64 * j + 64], hd // 2 + 32 * j + np.arange(32))
    assert list(R.gemma2_head_perm(256)[:3]) == [0, 1, 2] and list(R.gemma2_head_perm(256)[32:35]) == [128, 129, 130]


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict(name, fmt, tmp_path):
    """Every array equals its state-dict tensor bit for bit: q / k heads under gemma2_head_perm at 128 and 256, gate / up
    interleaved in blocks of 32, the tied head, the four norms as stored (no 1 added), rows padded to 256 with zeros."""
    import torch
    import llm_rescore as R
    model, cfg = tiny_gemma2(name, fmt=fmt)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_gemma2_arrays(str(tmp_path), dtype=fmt)
    sd = model.state_dict()
    rd = gemma2_ref_dims(cfg)
    wdt = getattr(torch, fmt)
    assert dims == R.gemma2_dims(cfg) and dims["max_pos"] == 256 and dims["tied"] is True
    for k in ("n_layers", "d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab", "head_dim", "rms_eps", "q_scale", "attn_cap",
              "final_cap"):
        assert dims[k] == rd[k], k
    d, Hq, Hkv, Fd, V, hd = (rd[k] for k in ("d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab", "head_dim"))
    assert Hq * hd > d
    eq = lambda a, b: a.dtype == wdt and torch.equal(a, b.to(wdt)) and torch.equal(a.float(), b)   # bit for bit, and exact
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert not arr["embed_tokens"][V:].any() and arr["lm_head"] is arr["embed_tokens"]
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (256, hd // 2)
    cos, sin = R.rope_tables(hf_inv_freq(model), 256)
    assert np.array_equal(arr["rope_cos"].numpy(), cos) and np.array_equal(arr["rope_sin"].numpy(), sin)
    hp = torch.from_numpy(R.gemma2_head_perm(hd))
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        for f, n in (("norm1_w", "input_layernorm"), ("norm2_w", "post_attention_layernorm"),
                     ("pre_ffn_norm_w", "pre_feedforward_layernorm"), ("post_ffn_norm_w", "post_feedforward_layernorm")):
            assert eq(a(f), sd[p + n + ".weight"]), f
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any()
        q, k = sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"]
        for h in range(Hq):
            assert eq(w[h * hd:(h + 1) * hd], q[h * hd:(h + 1) * hd][hp]), h
        for h in range(Hkv):
            assert eq(w[(Hq + h) * hd:(Hq + h + 1) * hd], k[h * hd:(h + 1) * hd][hp]), h
        assert eq(w[(Hq + Hkv) * hd:qw], sd[p + "self_attn.v_proj.weight"])          # v as it is
        assert f"layers.{l}.qkv_b" not in arr
        dp = -(-d // 256) * 256
        assert a("o_w").shape == (dp, Hq * hd) and eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and not a("o_w")[d:].any()
        gu = a("gate_up_w")
        assert gu.shape == (-(-2 * Fd // 256) * 256, d) and not gu[2 * Fd:].any()
        blocks = gu[:2 * Fd].view(Fd // 32, 2, 32, d)
        assert eq(blocks[:, 0].reshape(Fd, d), sd[p + "mlp.gate_proj.weight"])
        assert eq(blocks[:, 1].reshape(Fd, d), sd[p + "mlp.up_proj.weight"])
        assert a("down_w").shape == (dp, Fd) and eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"])
        assert len({a(f).data_ptr() for f in ("norm1_w", "norm2_w", "pre_ffn_norm_w", "post_ffn_norm_w")}) == 4
        assert not torch.equal(a("pre_ffn_norm_w"), a("post_ffn_norm_w"))
    for t in arr.values():
        assert t.is_contiguous()
    assert R.gemma2_embed_scale(d, fmt) == float(torch.tensor(d ** 0.5).to(wdt)) != d ** 0.5


def test_refusals(tmp_path):
    import llm_rescore as R
    model, cfg = tiny_gemma2("hd128", n_layers=1)
    with pytest.raises(ValueError, match="model_type 'gemma2'"):       # llama_dims stays as it is
        R.llama_dims(cfg)
    n = [0]

    def both(match, c):
        with pytest.raises(ValueError, match=match):
            R.gemma2_dims(c)
        n[0] += 1
        sub = tmp_path / f"r{n[0]}"
        os.makedirs(sub)
        with open(sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(sub), device="cpu")
    plain = {k: v for k, v in cfg.items() if k not in ("rope_parameters", "rope_scaling")} | {"rope_theta": 10000.0}
    R.gemma2_dims(plain)
    both("hidden_activation", cfg | {"hidden_activation": "gelu"})
    both("hidden_activation", cfg | {"hidden_activation": "silu"})
    both("attention_bias", cfg | {"attention_bias": True})
    both("rope_type", plain | {"rope_scaling": {"rope_type": "yarn", "factor": 2.0}})
    both("rope_type", plain | {"rope_scaling": {"type": "linear", "factor": 2.0}})
    both("rope_type", plain | {"rope_scaling": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                                "high_freq_factor": 4.0, "original_max_position_embeddings": 64}})
    both("head_dim 64", cfg | {"head_dim": 64})
    both("head_dim 512", cfg | {"head_dim": 512})
    both("head_dim 192", cfg | {"head_dim": 192})
    both("hidden_size 200, intermediate_size 448 and num_attention_heads \\* head_dim 512 must be multiples of 64",
         cfg | {"hidden_size": 200})
    both("intermediate_size 300 .* must be multiples of 64", cfg | {"intermediate_size": 300})
    both("tie_word_embeddings", cfg | {"tie_word_embeddings": False})
    both("use_bidirectional_attention", cfg | {"use_bidirectional_attention": True})
    both("num_key_value_heads", cfg | {"num_key_value_heads": 3})
    both("attn_logit_softcapping", cfg | {"attn_logit_softcapping": -1.0})
    # a cap of None is off; max_pos is the smallest of the three
    off = R.gemma2_dims(cfg | {"attn_logit_softcapping": None, "final_logit_softcapping": None})
    assert off["attn_cap"] == 0.0 and off["final_cap"] == 0.0
    assert R.gemma2_dims(cfg)["attn_cap"] == 2.0 and R.gemma2_dims(cfg)["final_cap"] == 3.0
    assert R.gemma2_dims(cfg | {"max_position_embeddings": 8192, "sliding_window": 4096})["max_pos"] == 4096
    assert R.gemma2_dims(cfg | {"max_position_embeddings": 8192, "sliding_window": 4096}, max_positions=100)["max_pos"] == 100
    assert R.gemma2_dims(cfg | {"max_position_embeddings": 64, "sliding_window": 4096})["max_pos"] == 64
    assert R.gemma2_dims(cfg | {"max_position_embeddings": 8192, "sliding_window": 4096}, max_positions=1 << 20)["max_pos"] == 4096
    with pytest.raises(ValueError, match="max_positions"):
        R.gemma2_dims(cfg, max_positions=0)
    # the neighbours stay unsupported model types, and the refusal lists gemma2 in the middle
    for mt in ("gemma", "gemma3", "gemma3_text", "qwen3_moe"):
        with pytest.raises(ValueError, match=f"model_type '{mt}'"):
            R.gemma2_dims(cfg | {"model_type": mt})
        os.makedirs(tmp_path / mt)
        with open(tmp_path / mt / "config.json", "w") as f:
            json.dump(cfg | {"model_type": mt}, f)
        with pytest.raises(ValueError, match=f"model_type '{mt}' is not supported") as ei:
            R.build_scorer(str(tmp_path / mt), device="cpu")
        msg = str(ei.value)
        assert "(opt, gpt2, gpt_neox, llama" in msg and msg.endswith("olmo2, mixtral)") and ", gemma2, " in msg
    # a Gemma-2 directory without weights gets as far as the weights; bf16 with a cache is refused before that
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    with pytest.raises(ValueError, match="follow-up"):
        R.build_scorer(str(bare), device="cuda", dtype="bfloat16", context_cache_tokens=64)
    # the layout: all four norms are required, biases and a head of its own refused
    st = state_of(model, True)
    dims, inv = R.gemma2_dims(cfg), R.rope_inv_freq(cfg)
    for lack in ("pre_feedforward_layernorm", "post_feedforward_layernorm", "post_attention_layernorm", "input_layernorm"):
        with pytest.raises(KeyError, match=lack):
            R.gemma2_device_layout({k: v for k, v in st.items() if lack not in k}, dims, inv)
    with pytest.raises(ValueError, match="q_proj.bias"):
        R.gemma2_device_layout(dict(st, **{"model.layers.0.self_attn.q_proj.bias": st["model.norm.weight"]}), dims, inv)
    with pytest.raises(ValueError, match="untied head"):
        R.gemma2_device_layout(dict(st, **{"lm_head.weight": st["model.embed_tokens.weight"] * 2}), dims, inv)
    with pytest.raises(ValueError, match="o_proj.weight: shape"):
        R.gemma2_device_layout(dict(st, **{"model.layers.0.self_attn.o_proj.weight": st["model.layers.0.self_attn.o_proj.weight"][:, :192]}),
                               dims, inv)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")
SIZES = ("ws_bytes", "tree_ws_bytes", "cache_kv_bytes", "tree_cached_ws_bytes")


def _g2(n_layers=1, hd=256, q_scale=0.1, attn_cap=50.0, final_cap=30.0, embed_scale=16.0, pre=FAKE, post=FAKE):
    import b2t_native as N
    layers = (N.ClmGemma2Layer * max(1, n_layers))()
    for i in range(n_layers):
        layers[i].pre_ffn_norm_w, layers[i].post_ffn_norm_w = pre, post
    g = N.ClmGemma2(hd, q_scale, attn_cap, final_cap, embed_scale, layers)
    g._keep = layers
    return g


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_struct_layouts_match_the_header(tmp_path):
    import b2t_native as N
    src = tmp_path / "lay.c"
    fl = [n for n, _ in N.ClmGemma2Layer._fields_]
    fd = [n for n, _ in N.ClmGemma2._fields_]
    body = "".join(f'printf("L.{f} %zu\\n", offsetof(b2t_clm_gemma2_layer_t, {f}));' for f in fl) + \
           "".join(f'printf("D.{f} %zu\\n", offsetof(b2t_clm_gemma2_t, {f}));' for f in fd)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){'
                   'printf("L %zu\\nD %zu\\n", sizeof(b2t_clm_gemma2_layer_t), sizeof(b2t_clm_gemma2_t));' + body + "return 0;}")
    exe = tmp_path / "lay"
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["L"]) == C.sizeof(N.ClmGemma2Layer) and int(got["D"]) == C.sizeof(N.ClmGemma2)
    for f in fl:
        assert int(got["L." + f]) == getattr(N.ClmGemma2Layer, f).offset, f
    for f in fd:
        assert int(got["D." + f]) == getattr(N.ClmGemma2, f).offset, f
    assert fl == ["pre_ffn_norm_w", "post_ffn_norm_w"]
    assert fd == ["head_dim", "q_scale", "attn_cap", "final_cap", "embed_scale", "layers_host"]


def test_entry_points_are_declared_and_bound():
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY + SIZES:     # the Llama twin's list with the descriptor after the model
        new, twin = "b2t_clm_gemma2_" + t, "b2t_clm_llama_" + t
        want = decl(twin)
        assert decl(new) == want[:1] + ["const b2t_clm_gemma2_t* g2"] + want[1:], new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == [g.argtypes[0], C.POINTER(N.ClmGemma2)] + list(g.argtypes[1:])
    assert sorted(re.findall(r"\b(b2t_clm_gemma2_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))) == \
        sorted("b2t_clm_gemma2_" + t for t in ENTRY + SIZES)
    assert set("b2t_clm_gemma2_" + t for t in ENTRY + SIZES) <= set(N.header_symbols())


def test_sizes():
    """With Hq hd == d the workspace is the Llama twin's plus an fp32 region [round_up(rows, 256)][d] and the attention output
    [round_up(rows, 256)][Hq hd]; a wider Hq hd widens the QKV rows and the attention output and nothing else; the cache's bytes
    use the real head dim; invalid arguments give 0."""
    lib = __import__("b2t_native").load()
    al = lambda x: -(-x // 256) * 256
    for d, H, kv, hd in ((512, 2, 1, 256), (512, 4, 2, 128), (128, 2, 1, 256), (192, 4, 2, 128)):
        desc, g = _model(bias=False, d=d, heads=H, kv=kv), _g2(hd=hd)
        p = C.byref(desc)
        wide = _model(bias=False, d=H * hd, heads=H, kv=kv)       # the Llama shape with the same QKV width
        for M in (1, 2, 255, 256, 257, 692):
            for n_seq in sorted({1, max(1, M // 3), M}):
                for rows in sorted({1, M // 2 + 1, M}):
                    Mp = al(rows)
                    extra = al(4 * Mp * d) + al(2 * Mp * H * hd)
                    got = lib.b2t_clm_gemma2_tree_ws_bytes(p, g, rows, M, n_seq)
                    if H * hd == d:
                        assert got == lib.b2t_clm_llama_tree_ws_bytes(p, rows, M, n_seq) + extra
                        assert lib.b2t_clm_gemma2_tree_cached_ws_bytes(p, g, rows, M, n_seq) == \
                            lib.b2t_clm_llama_tree_cached_ws_bytes(p, rows, M, n_seq) + extra
                    else:     # the narrow model needs less than the Llama shape of width Hq hd, more than the qkv rows alone
                        assert al(2 * rows * (H + 2 * kv) * hd) + extra < got < \
                            lib.b2t_clm_llama_tree_ws_bytes(C.byref(wide), rows, M, n_seq) + al(4 * Mp * H * hd) + al(2 * Mp * H * hd)
                    assert lib.b2t_clm_gemma2_tree_cached_ws_bytes(p, g, rows, M, n_seq) == \
                        got + al(4 * rows * H * 2) + al(4 * rows * H * hd)
                assert lib.b2t_clm_gemma2_ws_bytes(p, g, M, n_seq) > 0
        for cap in (1, 8, 64):
            assert lib.b2t_clm_gemma2_cache_kv_bytes(p, g, cap) == desc.n_layers * cap * 2 * kv * hd * 2
        assert lib.b2t_clm_gemma2_cache_kv_bytes(p, g, 0) == 0 and lib.b2t_clm_gemma2_cache_kv_bytes(p, g, 65) == 0
    desc, g = _model(bias=False), _g2()
    p = C.byref(desc)
    assert lib.b2t_clm_gemma2_ws_bytes(None, g, 10, 1) == 0 and lib.b2t_clm_gemma2_ws_bytes(p, None, 10, 1) == 0
    assert lib.b2t_clm_gemma2_tree_ws_bytes(p, None, 5, 10, 1) == 0 and lib.b2t_clm_gemma2_cache_kv_bytes(p, None, 4) == 0
    assert lib.b2t_clm_gemma2_tree_cached_ws_bytes(None, g, 5, 10, 1) == 0
    assert lib.b2t_clm_gemma2_ws_bytes(p, _g2(hd=64), 10, 1) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert lib.b2t_clm_gemma2_ws_bytes(p, g, n_tok, n_seq) == 0, (n_tok, n_seq)
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert lib.b2t_clm_gemma2_tree_ws_bytes(p, g, nn, nt, ns) == 0, (nn, nt, ns)
        assert lib.b2t_clm_gemma2_tree_cached_ws_bytes(p, g, nn, nt, ns) == 0, (nn, nt, ns)


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """The family's own model check (a head dim that is not d_model / n_heads is fine; 64 is not), the descriptor's refusals
    and the list's, with fake pointers and no GPU; the call's own messages carry its name; on the cached call the cache is left
    as it was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_gemma2_" + entry
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
        g = _g2(desc.n_layers if desc is not None else 1) if g is NOG else g
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

    # the model's and the descriptor's
    refused("null model", None, own=False)
    refused("null gemma2 descriptor", nb(), g=None, own=False)
    for hd in (64, 80, 192, 512, 0):
        refused(f"head dim {hd} ", nb(), g=_g2(hd=hd), own=False)
    refused("multiple of n_kv_heads", nb(d=512, heads=8, kv=3), own=False)
    refused("multiples of 64", nb(d=256, heads=4, ffn=500), own=False)
    refused("multiples of 64", nb(d=200, heads=4), own=False)
    refused("bad dimensions", nb(kv=0), own=False)
    refused("bad dimensions", nb(max_pos=0), own=False)
    refused("rms_eps", nb(eps=-1.0), own=False)
    refused("caps", nb(), g=_g2(attn_cap=-1.0), own=False)
    refused("caps", nb(), g=_g2(final_cap=-0.5), own=False)
    refused("caps", nb(), g=_g2(final_cap=float("nan")), own=False)
    refused("q_scale", nb(), g=_g2(q_scale=0.0), own=False)
    refused("embed_scale", nb(), g=_g2(embed_scale=-1.0), own=False)
    refused("null weight", N.ClmLlamaDesc(0, 256, 4, 2, 512, 1000, 64, 1e-5, FAKE, FAKE, FAKE, FAKE, 0, None), own=False)
    bad = nb()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad, own=False)
    refused("null weight pointer in layer 0", nb(), g=_g2(pre=None), own=False)
    two = _g2(2)
    two.layers_host[1].post_ffn_norm_w = None
    refused("null weight pointer in layer 1", nb(n_layers=2), g=two, own=False)
    refused("layer 0 has q / k / v biases", _model(bias=True), own=False)
    # the list's: a model whose head dim is not d_model / n_heads (256 / 4 = 64; 3 heads do not even divide 192) gets that far
    refused("null argument", nb(), scores=None)
    refused("null argument", nb(d=192, heads=3, kv=3), g=_g2(hd=128), ws=None)
    refused("n_seq 0", nb(), n_seq=0)
    refused("empty", nb(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", nb(), off=[1, 2, 4])
    refused("outside", nb(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", nb(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4], cache=_cache(cap=3) if cached else None)
    # the workspace: this family's size functions
    desc, g = nb(), _g2()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes, trunk 2
    if cached:
        need = lib.b2t_clm_gemma2_tree_cached_ws_bytes(C.byref(desc), g, 4, 9, 3)
        refused("workspace", desc, g=g, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_gemma2_tree_cached_ws_bytes(C.byref(desc), g, 3, 9, 3)
        refused("workspace", desc, g=g, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("null cache member", desc, cache=_cache(kv=None))
        refused("above max_pos", nb(max_pos=64), cache=_cache(cap=65))
        refused("cached token 1 has id 1000", nb(vocab=1000), cache=_cache(ids=(2, 1000)))
        rc = fn(C.byref(desc), g, None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1, FAKE, None, None, None,
                FAKE, 1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_gemma2_score_tree_f16", N.last_error())
    elif tree:
        need = lib.b2t_clm_gemma2_tree_ws_bytes(C.byref(desc), g, 4, 9, 3)
        assert need > 0
        refused("workspace", desc, g=g, ids=ids, off=off, ws_bytes=need - 1)
    else:
        need = lib.b2t_clm_gemma2_ws_bytes(C.byref(desc), g, 9, 3)
        assert need > 0
        refused("workspace", desc, g=g, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_gemma2_unit_kernels_without_scratch():
    """The unit instantiates the three epilogues (EP_F32 = 10, EP_GEGLU = 12, EP_HEAD_CAP = 13) on two tiles and the three new
    kernels, each in two element types; the capped flat and tree attention at head dims 128 and 256 in two element types; the
    capped cached and trunk attention at both head dims in fp16: 30 kernels.  None uses scratch -- the attention kernels at
    head dim 256 take the whole VGPR file and must not spill."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_gemma2.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_gemma2.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_kernel" in k]
    attn = [k for k in res if "clm_attn" in k]
    assert len(res) == 30 and len(gemm) == 12 and len(attn) == 12, sorted(res)
    for ep in (10, 12, 13):
        assert sum(f"ELi{ep}E" in k for k in gemm) == 4, (ep, gemm)
    for kern, count in (("clm_gemma2_embed_kernel", 2), ("clm_gemma2_rmsnorm_kernel", 2), ("clm_gemma2_postnorm_add_kernel", 2),
                        ("clm_attn_cap_kernel", 4), ("clm_attn_tree_cap_kernel", 4), ("clm_attn_tree_cached_cap_kernel", 2),
                        ("clm_attn_trunk_cap_kernel", 2)):
        assert sum(kern in k for k in res) == count, (kern, sorted(res))
    for k in attn:
        print(f"CLM gemma2 {k[:90]}: {res[k]}")
        assert res[k].get("ScratchSize", -1) == 0, (k, res[k])
    assert all(v.get("ScratchSize", -1) == 0 for v in res.values()), res
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_gemma2.hip")).read()
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src        # the one tile rule
    for ep in ("EP_GEGLU", "EP_F32", "EP_HEAD_CAP"):
        assert src.count(f"launch_gemm(g, s, &clm_gemm_tiles<{ep}, El>)") == 1
    with open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "clm_internal.h")) as f:
        assert "EP_GEGLU = 12, EP_HEAD_CAP = 13" in f.read()


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_gemma2("hd256", fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    sd = {k: v.float() for k, v in model.state_dict().items()}
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.Gemma2Scorer) and isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu"
        assert sc._family == "gemma2" and sc._SIZES == "b2t_clm_gemma2_" and R.LlamaScorer._SIZES == "b2t_clm_llama_"
        assert sc.desc.n_heads == 2 and sc.desc.n_kv_heads == 1 and sc.desc.d_model == 128 and sc.desc.vocab == 777
        assert sc.desc.lm_head == sc.desc.embed_tokens and not sc.desc.layers_host[0].qkv_b and sc.desc.max_pos == 256
        g = sc._g2
        assert g.head_dim == 256 and g.q_scale == np.float32(1 / 12) and g.attn_cap == 2.0 and g.final_cap == 3.0
        assert g.embed_scale == float(torch.tensor(128 ** 0.5).to(want))
        for l in range(2):
            assert g.layers_host[l].pre_ffn_norm_w == sc.w[f"layers.{l}.pre_ffn_norm_w"].data_ptr()
            assert g.layers_host[l].post_ffn_norm_w == sc.w[f"layers.{l}.post_ffn_norm_w"].data_ptr()
            assert sc.desc.layers_host[l].norm2_w == sc.w[f"layers.{l}.norm2_w"].data_ptr()
            assert sc.w[f"layers.{l}.qkv_w"].shape == (1024, 128) and sc.w[f"layers.{l}.o_w"].shape == (256, 512)
        if want is torch.bfloat16:     # a bf16 checkpoint's values are kept exactly
            assert torch.equal(sc.w["layers.1.post_ffn_norm_w"].float(), sd["model.layers.1.post_feedforward_layernorm.weight"])
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    # Llama arrays are not Gemma-2 arrays
    from test_clm_llama_host import tiny_model
    m2, c2 = tiny_model("llama", n_layers=1)
    d2 = R.llama_dims(c2)
    with pytest.raises(KeyError, match="head_dim"):
        R.Gemma2Scorer(d2, R.llama_device_layout(state_of(m2, False), d2, R.rope_inv_freq(c2)), "cpu")
