"""Host-side checks of the gpt-oss rescorer (csrc/causal_lm_gptoss.hip, csrc/clm_gptoss.h, "gpt_oss" in llm_rescore; no GPU): the
float64 restatement of the contract (ref_logp_gptoss, the reference of tests/test_gpu_clm_gptoss.py) against HF's
GptOssForCausalLM evaluated in float64, its sensitivity to every term the family adds, gptoss_rope against HF's rotary module, the
loader on both spellings of a checkpoint (plain and MXFP4), the refusals, the six entry points' declarations, bindings, sizes and
refusals before any device work, the kernels of the translation unit, and the precondition of the GPU test's routed-differently
share.

The tiny model (tiny_gptoss) is a random HF GptOssForCausalLM built in memory with eager attention and eager experts: d 192, 4
heads of 64 over 2 kv heads (Hq hd = 256 != d), F 64, 8 experts top-4, window 16 on layer 0 and full attention on layer 1, yarn,
vocab 300.  Sinks and every bias are N(0, 0.5), so that each matters."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_clm_llama_host import FAKE, _model, hf_logp, state_of, tiny_seqs
from test_clm_mixtral_host import E16_CAP, E_BF16_MAX, _maxdiff, contract_seqs, gap_behind_choice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

TINY = dict(hidden_size=192, num_attention_heads=4, num_key_value_heads=2, head_dim=64, intermediate_size=64, num_local_experts=8,
            num_experts_per_tok=4, sliding_window=16, vocab_size=300, max_position_embeddings=512, rms_norm_eps=1e-5)
ROUTER_SCALE = 0.125     # router weights are N(0, 1) * ROUTER_SCALE / sqrt(d) beside a bias of N(0, 0.5): see test_route_share_precondition
HOST_LENS = (1, 2, 15, 16, 17, 18, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100)
HF_MEASURED = 7.2e-15    # the largest |dlogp| of the unrounded restatement against HF's forward in float64 (NOTES.md)
HF_BOUND = 10 * HF_MEASURED
SHARE_REF_MAX = 0.02


def gptoss_config(n_layers=2, **over):
    """the config of the tiny model with `over` laid over TINY, as the dict of config.json"""
    import transformers
    cfg = transformers.GptOssConfig(num_hidden_layers=n_layers, attn_implementation="eager", **dict(TINY, **over))
    return cfg, json.loads(cfg.to_json_string())


def random_state(cfg, fmt="float16", seed=0, router_scale=ROUTER_SCALE, bias_std=0.5, device="cpu"):
    """A random gpt-oss state dict (plain spelling, fp32 values representable in fmt) for the config dict cfg, made on `device`
    without an HF module.  A matrix is N(0, 1) / sqrt(fan-in), the router's times router_scale, a norm weight 1 + 0.2 N(0, 1),
    embedding and head 2 N(0, 1) / sqrt(d); sinks and all biases are N(0, bias_std)."""
    import torch
    d, Hq, Hkv, hd, Fd, ne, V = (cfg[k] for k in ("hidden_size", "num_attention_heads", "num_key_value_heads", "head_dim",
                                                    "intermediate_size", "num_local_experts", "vocab_size"))
    g = torch.Generator(device=device).manual_seed(700 + seed)
    rdt = getattr(torch, fmt)
    rn = lambda *shape: torch.randn(shape, generator=g, device=device)
    fit = lambda v: v.to(rdt).float()
    st = {"model.embed_tokens.weight": fit(rn(V, d) * 2.0 / d ** 0.5)}
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{l}."
        st[p + "self_attn.sinks"] = fit(rn(Hq) * bias_std)
        for n, rows, cols in (("q_proj", Hq * hd, d), ("k_proj", Hkv * hd, d), ("v_proj", Hkv * hd, d), ("o_proj", d, Hq * hd)):
            st[p + f"self_attn.{n}.weight"] = fit(rn(rows, cols) / cols ** 0.5)
            st[p + f"self_attn.{n}.bias"] = fit(rn(rows) * bias_std)
        st[p + "mlp.router.weight"] = fit(rn(ne, d) * router_scale / d ** 0.5)
        st[p + "mlp.router.bias"] = fit(rn(ne) * bias_std)
        st[p + "mlp.experts.gate_up_proj"] = fit(rn(ne, d, 2 * Fd) / d ** 0.5)
        st[p + "mlp.experts.gate_up_proj_bias"] = fit(rn(ne, 2 * Fd) * bias_std)
        st[p + "mlp.experts.down_proj"] = fit(rn(ne, Fd, d) / Fd ** 0.5)
        st[p + "mlp.experts.down_proj_bias"] = fit(rn(ne, d) * bias_std)
        st[p + "input_layernorm.weight"] = fit(1 + 0.2 * rn(d))
        st[p + "post_attention_layernorm.weight"] = fit(1 + 0.2 * rn(d))
    st["model.norm.weight"] = fit(1 + 0.2 * rn(d))
    st["lm_head.weight"] = fit(rn(V, d) * 2.0 / d ** 0.5)
    return st


def tiny_gptoss(n_layers=2, fmt="float16", seed=0, router_scale=ROUTER_SCALE, bias_std=0.5, **over):
    """(HF fp32 CPU GptOssForCausalLM in eval mode, eager attention and eager experts, holding random_state's weights; its config
    as the dict of config.json)"""
    import torch
    import transformers
    cfg, cfgd = gptoss_config(n_layers, **over)
    torch.manual_seed(seed)
    model = transformers.GptOssForCausalLM(cfg).float().eval()
    model.config._experts_implementation = "eager"
    st = random_state(cfgd, fmt, seed, router_scale, bias_std)
    assert sorted(st) == sorted(model.state_dict())
    model.load_state_dict(st)
    return model, cfgd


def ref_logp_gptoss(st, dims, rope, seqs, fmt=None, routes=None, opts=()):
    """The float64 restatement of include/b2t.h's gpt-oss contract, in the style of ref_logp_mixtral_fmt
    (tests/test_clm_mixtral_host.py): fmt = None rounds nowhere; "float16" / "bfloat16" round where the kernels round -- the
    RMSNorm outputs, q, k, v, P per 32-key block, the attention output, the experts' hidden rows -- and never the router's logits,
    the weights, an expert's output or a sink.  `st` is a state dict in the plain spelling, dims = llm_rescore.gptoss_dims(cfg),
    rope = llm_rescore.gptoss_rope(cfg).  routes as in ref_logp_mixtral_fmt.  opts names terms to leave out, for the sensitivity
    tests only: "no_window", "window+1", "no_plus1", "no_clamp", "alpha1", "no_sink".
    Returns (per-sequence log-probs, router logits [n_layers][rows][n_experts], free choice [n_layers][rows][top_k], the shares
    of gate and up pre-activations that hit the clamp)."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    rnd = (lambda t: t) if fmt is None else (lambda t: t.to(R.clm_dtype(fmt)).double())
    d, Hq, Hkv, nl, V, eps, hd = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "n_layers", "vocab", "rms_eps", "head_dim"))
    ne, topk, limit = dims["n_experts"], dims["top_k"], dims["swiglu_limit"]
    alpha = 1.0 if "alpha1" in opts else 1.702
    G = Hq // Hkv
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["model.embed_tokens.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    inv_freq, att = rope
    ang = pos.double()[:, None] * torch.as_tensor(np.asarray(inv_freq, np.float32), device=dev).double()[None, :]
    cos, sin = torch.cos(ang), torch.sin(ang)
    if fmt is not None:      # the fp32 table, the factor multiplied in fp32
        f32 = torch.tensor(att, dtype=torch.float32, device=dev)
        cos, sin = (cos.float() * f32).double(), (sin.float() * f32).double()
    else:
        cos, sin = cos * att, sin * att
    cos, sin = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]   # [M, 1, hd]
    rot = lambda t: t * cos + torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], -1) * sin
    rms = lambda t, w: t * torch.rsqrt((t * t).mean(-1, keepdim=True) + eps) * W(w)
    lin = lambda t, p: t @ W(p + ".weight").T + W(p + ".bias")
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    logits_out, free_out, n_gate, n_up, n_all = [], [], 0, 0, 0
    for l in range(nl):
        p = f"model.layers.{l}."
        win = dims["windows"][l]
        if "no_window" in opts:
            win = 0
        elif "window+1" in opts and win:
            win += 1
        h = rnd(rms(x, p + "input_layernorm.weight"))
        q = rnd(rot(lin(h, p + "self_attn.q_proj").view(M, Hq, hd)) * hd ** -0.5)
        k = rnd(rot(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd)))
        v = rnd(lin(h, p + "self_attn.v_proj")).view(M, Hkv, hd)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)
        sink = W(p + "self_attn.sinks")[:, None]                                      # [Hq, 1]
        if "no_sink" in opts:
            sink = torch.full_like(sink, float("-inf"))
        o = torch.empty(M, Hq * hd, dtype=torch.float64, device=dev)
        for j in range(B):
            n = lens[j]
            sl = slice(off[j], off[j + 1])
            s = q[sl].transpose(0, 1) @ k[sl].transpose(0, 1).transpose(1, 2)      # [Hq, n, n]
            kk = torch.arange(n, device=dev)
            hidden = kk[None, :] > kk[:, None]
            if win:
                hidden = hidden | (kk[None, :] <= kk[:, None] - win)
            s = s.masked_fill(hidden[None], float("-inf"))
            nb = -(-n // 32)
            sb = F.pad(s, (0, nb * 32 - n), value=float("-inf")).view(Hq, n, nb, 32)
            mb = torch.maximum(sb.amax(-1).cummax(-1).values, sink[..., None])       # the running max starts at the sink
            pb = torch.where(sb == float("-inf"), torch.zeros_like(sb), torch.exp(sb - mb[..., None]))
            resc = torch.exp(mb - mb[..., -1:])[..., None]
            lsum = (pb * resc).sum((-1, -2)) + torch.exp(sink - mb[..., -1])         # the sink is in the denominator only
            pr = (rnd(pb) * resc).view(Hq, n, nb * 32)[..., :n]
            o[sl] = ((pr @ v[sl].transpose(0, 1)) / lsum[..., None]).transpose(0, 1).reshape(n, Hq * hd)
        x = x + lin(rnd(o), p + "self_attn.o_proj")
        h = rnd(rms(x, p + "post_attention_layernorm.weight"))
        lg = h @ W(p + "mlp.router.weight").T + W(p + "mlp.router.bias")           # [M, ne], never rounded
        work, free = lg.clone(), []
        for _ in range(topk):
            e = work.argmax(-1)
            free.append(e)
            work.scatter_(1, e[:, None], float("-inf"))
        free = torch.stack(free, 1)
        ch = free if routes is None else torch.as_tensor(np.ascontiguousarray(routes[l], dtype=np.int64), device=dev)
        sel = lg.gather(1, ch)
        wt = torch.exp(sel - sel[:, :1])
        wt = wt / wt.sum(-1, keepdim=True)
        gu, gub = W(p + "mlp.experts.gate_up_proj"), W(p + "mlp.experts.gate_up_proj_bias")
        dn, dnb = W(p + "mlp.experts.down_proj"), W(p + "mlp.experts.down_proj_bias")
        y = torch.zeros(M, d, dtype=torch.float64, device=dev)
        for j in range(topk):                                                       # in order of choice
            yj = torch.empty(M, d, dtype=torch.float64, device=dev)
            for e in range(ne):
                rows = (ch[:, j] == e).nonzero()[:, 0]
                if rows.numel():
                    g_u = h[rows] @ gu[e] + gub[e]
                    gate, up = g_u[:, ::2], g_u[:, 1::2]
                    n_gate += int((gate > limit).sum())
                    n_up += int((up.abs() > limit).sum())
                    n_all += gate.numel()
                    if "no_clamp" not in opts:
                        gate, up = gate.clamp(max=limit), up.clamp(-limit, limit)
                    one = 0.0 if "no_plus1" in opts else 1.0
                    yj[rows] = rnd((up + one) * gate * torch.sigmoid(alpha * gate)) @ dn[e] + dnb[e]
            y = wt[:, j:j + 1] * yj if j == 0 else y + wt[:, j:j + 1] * yj
        x = x + y
        logits_out.append(lg.cpu().numpy())
        free_out.append(free.cpu().numpy())
    logits_out, free_out = np.stack(logits_out), np.stack(free_out)
    clamped = (n_gate / max(n_all, 1), n_up / max(n_all, 1))
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out, logits_out, free_out, clamped
    tgt = ids[src + 1]
    h = rnd(rms(x[src], "model.norm.weight"))
    E = st["lm_head.weight"]
    chunk = max(64, (1 << 25) // h.shape[0])
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out, logits_out, free_out, clamped


def gptoss_state(fmt="float16", seed=0, **kw):
    """(model, cfg, state dict, dims, rope) of the tiny model with fmt-valued weights"""
    import llm_rescore as R
    model, cfg = tiny_gptoss(fmt=fmt, seed=seed, **kw)
    return model, cfg, state_of(model, False), R.gptoss_dims(cfg), R.gptoss_rope(cfg)


def gptoss_figures(st, rd, rope, seqs, fmt):
    """(e, e_router, share_ref, logits and free choice of the unrounded restatement) of one case, restatement against
    restatement: e what the contract's roundings alone do to the log-probs under the unrounded restatement's routes, e_router
    what they do to the router's logits, share_ref the share of (layer, row) pairs that the rounded restatement, left free,
    routes unlike the unrounded one (order included)."""
    exact, lg0, free0, _ = ref_logp_gptoss(st, rd, rope, seqs)
    rounded, lg1, _, _ = ref_logp_gptoss(st, rd, rope, seqs, fmt, routes=free0)
    _, _, free1, _ = ref_logp_gptoss(st, rd, rope, seqs, fmt)
    e = float(np.abs(np.concatenate(rounded) - np.concatenate(exact)).max())
    e_router = float(np.abs(lg1 - lg0).max())
    share_ref = float((free0 != free1).any(-1).mean())
    return e, e_router, share_ref, lg0, free0


# ---- the restatement ------------------------------------------------------------------------------------------------------
def hf_logp_float64(model, seqs):
    """hf_logp of HF's forward evaluated in float64 throughout, by the float-widening patch of tests/test_clm_mixtral_host.py
    (Tensor.float(), torch.float32 and torch.float give float64 while it runs); the final norm and the router (whose softmax
    over the top-k logits takes the logits' dtype) must both have seen float64."""
    import torch
    import transformers
    from unittest import mock
    wide = lambda t, *a, **k: t if t.dtype == torch.float64 else t.double()
    seen, routed = [], []
    hooks = [model.model.norm.register_forward_hook(lambda mod, args, out: seen.append((args[0].dtype, out.dtype))),
             model.model.layers[0].mlp.router.register_forward_hook(lambda mod, args, out: routed.append((out[0].dtype, out[1].dtype)))]
    model.config._experts_implementation = "eager"
    try:
        with mock.patch.object(torch.Tensor, "float", wide), mock.patch.object(torch, "float32", torch.float64), \
                mock.patch.object(torch, "float", torch.float64):
            out = hf_logp(model.double(), seqs)
    finally:
        for h in hooks:
            h.remove()
        model.float()
    ver = transformers.__version__
    assert seen and all(d == (torch.float64, torch.float64) for d in seen), f"transformers {ver}: the final norm saw {set(seen)}"
    assert routed and all(d == (torch.float64, torch.float64) for d in routed), f"transformers {ver}: the router gave {set(routed)}"
    return out


def test_unrounded_restatement_equals_hf_in_float64():
    """The unrounded restatement is HF's forward, HF's code evaluated in float64, to 10 x the measured difference (NOTES.md);
    were it not below 1e-10 it would be another function."""
    import torch
    model, cfg, st, rd, rope = gptoss_state()
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_gptoss(st, rd, rope, seqs)[0]
    hf = hf_logp_float64(model, seqs)
    err, mx = _maxdiff(exact, hf), max(np.abs(b).max() for b in hf)
    print(f"CLM gptoss restatement vs HF's forward in float64: {err:.3e} (max |logp| {mx:.2f})")
    assert torch.ones(1).float().dtype is torch.float32 and next(model.parameters()).dtype is torch.float32   # the patches are gone
    assert HF_BOUND < 1e-10 and mx > 5 and err <= HF_BOUND, err
    assert rd["windows"] == [16, 0] and max(map(len, seqs)) > 5 * 16


def _planted_clamp(st):
    """biases planted so that a share of the gates exceeds the limit and a share of the ups does on either side"""
    out = dict(st)
    for k, v in st.items():
        if k.endswith("gate_up_proj_bias"):
            b = v.clone()
            b[:, 0::8] += 9.0        # every fourth gate
            b[:, 1::16] += 9.0       # every eighth up above
            b[:, 9::16] -= 9.0       # every eighth up below
            out[k] = b
    return out


def test_restatement_is_sensitive_to_every_term():
    """One term at a time: sinks zeroed, the window ignored or off by one, the router bias dropped, each expert bias dropped, the
    + 1 dropped, the clamp dropped (biases planted: > 10 % of the gates and of the ups at the limit), 1.702 -> 1, the attention
    factor dropped.  Each moves the log-probs by more than 100 x HF_BOUND."""
    import torch
    model, cfg, st, rd, rope = gptoss_state()
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=(17, 33, 100))
    base = ref_logp_gptoss(st, rd, rope, seqs)[0]
    zero = lambda suffix: {k: (torch.zeros_like(v) if k.endswith(suffix) else v) for k, v in st.items()}
    assert rope[1] > 1.3       # yarn's factor, 0.1 ln 32 + 1
    moved = {
        "sinks zeroed": ref_logp_gptoss(zero("self_attn.sinks"), rd, rope, seqs)[0],
        "window ignored": ref_logp_gptoss(st, rd, rope, seqs, opts=("no_window",))[0],
        "window off by one": ref_logp_gptoss(st, rd, rope, seqs, opts=("window+1",))[0],
        "router bias": ref_logp_gptoss(zero("router.bias"), rd, rope, seqs)[0],
        "gate_up bias": ref_logp_gptoss(zero("gate_up_proj_bias"), rd, rope, seqs)[0],
        "down bias": ref_logp_gptoss(zero("down_proj_bias"), rd, rope, seqs)[0],
        "+ 1": ref_logp_gptoss(st, rd, rope, seqs, opts=("no_plus1",))[0],
        "1.702": ref_logp_gptoss(st, rd, rope, seqs, opts=("alpha1",))[0],
        "attention factor": ref_logp_gptoss(st, rd, (rope[0], 1.0), seqs)[0],
    }
    for what, got in moved.items():
        diff = _maxdiff(got, base)
        print(f"CLM gptoss sensitivity: {what} moves the log-probs by {diff:.3e}")
        assert diff > 100 * HF_BOUND, (what, diff)
    planted = _planted_clamp(st)
    with_clamp, _, _, (sg, su) = ref_logp_gptoss(planted, rd, rope, seqs)
    diff = _maxdiff(ref_logp_gptoss(planted, rd, rope, seqs, opts=("no_clamp",))[0], with_clamp)
    print(f"CLM gptoss sensitivity: clamp moves the log-probs by {diff:.3e} (gates above the limit {sg:.3f}, ups beyond it {su:.3f})")
    assert sg > 0.1 and su > 0.1 and diff > 100 * HF_BOUND
    # a sink of -1e4 is no sink
    no_sink = ref_logp_gptoss(st, rd, rope, seqs, opts=("no_sink",))[0]
    far = {k: (torch.full_like(v, -1e4) if k.endswith("sinks") else v) for k, v in st.items()}
    assert _maxdiff(ref_logp_gptoss(far, rd, rope, seqs)[0], no_sink) < 1e-12


def test_rope_equals_hf():
    """gptoss_rope's inv_freq and attention factor are the rotary module's, and the table cos * f, sin * f is its output evaluated
    in float64, for yarn (truncate false: the correction range is not rounded) and for the default type."""
    import torch
    import llm_rescore as R
    from unittest import mock
    for over in ({}, {"rope_parameters": {"rope_type": "default", "rope_theta": 10000.0}},
                 {"rope_parameters": {"rope_type": "yarn", "factor": 8.0, "beta_fast": 32.0, "beta_slow": 1.0, "truncate": True,
                                      "original_max_position_embeddings": 128, "rope_theta": 150000.0}}):
        model, cfg = tiny_gptoss(n_layers=1, **over)
        inv, att = R.gptoss_rope(cfg)
        remb = model.model.rotary_emb
        assert inv.dtype == np.float32 and np.array_equal(inv, remb.inv_freq.numpy()) and att == float(remb.attention_scaling)
        pos = torch.arange(400)[None]
        wide = lambda t, *a, **k: t if t.dtype == torch.float64 else t.double()
        with mock.patch.object(torch.Tensor, "float", wide):
            cos, sin = remb(torch.zeros(1, dtype=torch.float64), pos)
        assert cos.dtype == torch.float64 and cos.shape == (1, 400, 32)
        tc, ts = R.rope_tables(inv, 400)
        assert np.abs(tc.astype(np.float64) * att - cos[0].numpy()).max() < 2e-7     # the table is fp32
        ang = np.arange(400, dtype=np.float64)[:, None] * inv.astype(np.float64)[None]
        assert np.abs(np.cos(ang) * att - cos[0].numpy()).max() < 1e-12 and np.abs(np.sin(ang) * att - sin[0].numpy()).max() < 1e-12
    assert R.gptoss_rope(tiny_gptoss(n_layers=1)[1])[1] == pytest.approx(0.1 * np.log(32.0) + 1.0)


# ---- the loader --------------------------------------------------------------------------------------------------------
def mxfp4_pack(w):
    """(blocks uint8 [..., rows, K / 32, 16], scales uint8 [..., rows, K / 32]) of an fp32 tensor [..., rows, K] whose groups of 32
    are MXFP4-representable (mxfp4_representable makes them): the test-local inverse of llm_rescore.mxfp4_dequant."""
    import torch
    import llm_rescore as R
    g = w.reshape(*w.shape[:-1], w.shape[-1] // 32, 32).double()
    amax = g.abs().amax(-1, keepdim=True)
    ex = torch.where(amax > 0, torch.ceil(torch.log2(amax / 6.0)), torch.zeros_like(amax))     # amax <= 6 * 2^ex
    q = g / torch.exp2(ex)
    lut = torch.tensor(R._FP4_VALUES[:8], dtype=torch.float64)
    idx = (q.abs()[..., None] - lut).abs().argmin(-1)
    assert torch.equal(lut[idx], q.abs()), "not MXFP4-representable"
    code = idx + 8 * ((q < 0) | ((q == 0) & (torch.signbit(q)))).long()
    blocks = (code[..., 0::2] | (code[..., 1::2] << 4)).to(torch.uint8)
    return blocks, (ex[..., 0] + 127).to(torch.uint8)


def mxfp4_representable(w, seed=0):
    """an fp32 tensor of w's shape whose groups of 32 along the last dim are e2m1 values times a power of two near w's scale"""
    import torch
    import llm_rescore as R
    g = torch.Generator().manual_seed(seed)
    lut = torch.tensor(R._FP4_VALUES, dtype=torch.float32)
    vals = lut[torch.randint(0, 16, w.shape, generator=g)]
    ex = torch.randint(-8, -4, (*w.shape[:-1], w.shape[-1] // 32, 1), generator=g).float()
    return (vals.reshape(*w.shape[:-1], -1, 32) * torch.exp2(ex)).reshape(w.shape)


def mxfp4_state(st):
    """(the state dict with MXFP4-representable expert matrices in the plain spelling, the same in the published MXFP4 spelling:
    gate_up_proj_blocks / _scales [E][2F][d / 32]([16]) and down_proj_blocks / _scales [E][d][F / 32]([16]) -- the transposed
    matrix, rows along K)"""
    plain, packed = {}, {}
    for k, v in st.items():
        if k.endswith("experts.gate_up_proj") or k.endswith("experts.down_proj"):
            wt = mxfp4_representable(v.transpose(1, 2).contiguous(), seed=len(plain))      # [E][rows][K]
            plain[k] = wt.transpose(1, 2).contiguous()
            packed[k + "_blocks"], packed[k + "_scales"] = mxfp4_pack(wt)
        else:
            plain[k] = packed[k] = v
    return plain, packed


def test_mxfp4_dequant_equals_hf_and_the_packer_round_trips():
    import torch
    import llm_rescore as R
    from transformers.integrations.mxfp4 import convert_moe_packed_tensors
    g = torch.Generator().manual_seed(5)
    blocks = torch.randint(0, 256, (3, 40, 6, 16), dtype=torch.uint8, generator=g)
    scales = torch.randint(110, 136, (3, 40, 6), dtype=torch.uint8, generator=g)
    ours = R.mxfp4_dequant(blocks, scales)
    assert ours.dtype == torch.float32 and ours.shape == (3, 40, 192)
    hf = convert_moe_packed_tensors(blocks, scales, dtype=torch.bfloat16)          # [E][32 G][rows]
    assert hf.shape == (3, 192, 40) and torch.equal(ours.to(torch.bfloat16).transpose(1, 2).view(torch.int16), hf.contiguous().view(torch.int16))
    assert ours[0, 0, 0] == R._FP4_VALUES[int(blocks[0, 0, 0, 0]) & 15] * 2.0 ** (int(scales[0, 0, 0]) - 127)    # low nibble first
    assert ours[0, 0, 1] == R._FP4_VALUES[int(blocks[0, 0, 0, 0]) >> 4] * 2.0 ** (int(scales[0, 0, 0]) - 127)
    w = mxfp4_representable(torch.zeros(2, 24, 64), seed=3)
    b, s = mxfp4_pack(w)
    assert b.shape == (2, 24, 2, 16) and s.shape == (2, 24, 2) and torch.equal(R.mxfp4_dequant(b, s), w) and w.abs().max() > 0
    with pytest.raises(ValueError, match="uint8"):
        R.mxfp4_dequant(blocks.int(), scales)
    with pytest.raises(ValueError, match="do not go with"):
        R.mxfp4_dequant(blocks, scales[:, :, :5])


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_loader_layout_from_both_spellings(fmt, tmp_path):
    """Every array against the state dict under the inverse transposes / interleaves; the MXFP4 spelling of the same
    (MXFP4-representable) model gives the same arrays bit for bit, from a state dict and from a directory."""
    import torch
    from safetensors.torch import save_file
    import llm_rescore as R
    model, cfg = tiny_gptoss(fmt=fmt)
    sd, packed = mxfp4_state(state_of(model, False))
    assert "model.layers.1.mlp.experts.down_proj_blocks" in packed and "model.layers.1.mlp.experts.down_proj" not in packed
    dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
    wdt = getattr(torch, fmt)
    a, b = R.gptoss_device_layout(sd, dims, rope, fmt), R.gptoss_device_layout(packed, dims, rope, fmt)
    for sub, state in (("plain", sd), ("mxfp4", packed)):
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "config.json", "w") as f:
            json.dump(cfg, f)
        save_file({k: v.contiguous() for k, v in state.items()}, str(tmp_path / sub / "model.safetensors"))
    loaded = [R.load_gptoss_arrays(str(tmp_path / sub), dtype=fmt) for sub in ("plain", "mxfp4")]
    for dm, arr in [(dims, b)] + loaded:
        assert dm == dims and sorted(arr) == sorted(a)
        for k in a:
            assert arr[k].dtype == a[k].dtype and arr[k].shape == a[k].shape and torch.equal(arr[k], a[k]), k
    d, Fd, ne, V, Hq, Hkv, hd = 192, 64, 8, 300, 4, 2, 64
    assert dims["windows"] == [16, 0] and dims["max_pos"] == 512 and dims["head_dim"] == 64 and R.mixtral_strides(dims) == (256, 256)
    eq = lambda x, y: x.dtype == wdt and torch.equal(x, y.to(wdt)) and torch.equal(x.float(), y)   # bit for bit, and exact
    assert a["embed_tokens"].shape == (512, d) and eq(a["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert eq(a["lm_head"][:V], sd["lm_head.weight"]) and not a["lm_head"][V:].any() and a["lm_head"] is not a["embed_tokens"]
    tc, ts = R.rope_tables(rope[0], 512)
    assert a["rope_cos"].dtype == torch.float32 and a["rope_cos"].shape == (512, 32)
    assert np.array_equal(a["rope_cos"].numpy(), tc * np.float32(rope[1])) and np.array_equal(a["rope_sin"].numpy(), ts * np.float32(rope[1]))
    for l in range(2):
        p, g = f"model.layers.{l}.", lambda f: a[f"layers.{l}.{f}"]
        assert eq(g("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(g("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        assert g("qkv_w").shape == (512, d) and eq(g("qkv_w")[:512], qkv)               # (4 + 2 * 2) * 64 = 512 rows, checkpoint order
        assert eq(g("qkv_b"), torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"]))
        assert g("o_w").shape == (256, Hq * hd) and eq(g("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and not g("o_w")[d:].any()
        assert eq(g("o_b"), sd[p + "self_attn.o_proj.bias"])
        assert g("sinks").dtype == torch.float32 and torch.equal(g("sinks"), sd[p + "self_attn.sinks"])
        assert eq(g("router_w"), sd[p + "mlp.router.weight"]) and eq(g("router_b"), sd[p + "mlp.router.bias"])
        gu, gub, dn, dnb = g("gate_up_w"), g("gate_up_b"), g("down_w"), g("down_b")
        assert gu.shape == (ne, 256, d) and gub.shape == (ne, 256) and dn.shape == (ne, 256, Fd) and dnb.shape == (ne, 256)
        assert not gu[:, 2 * Fd:].any() and not gub[:, 2 * Fd:].any() and not dn[:, d:].any() and not dnb[:, d:].any()
        W, Bi = sd[p + "mlp.experts.gate_up_proj"], sd[p + "mlp.experts.gate_up_proj_bias"]      # [E][d][2F], [E][2F]
        for e in range(ne):
            blocks = gu[e, :2 * Fd].view(Fd // 32, 2, 32, d)
            assert eq(blocks[:, 0].reshape(Fd, d), W[e][:, 0::2].T) and eq(blocks[:, 1].reshape(Fd, d), W[e][:, 1::2].T)
            bb = gub[e, :2 * Fd].view(Fd // 32, 2, 32)
            assert eq(bb[:, 0].reshape(Fd), Bi[e][0::2]) and eq(bb[:, 1].reshape(Fd), Bi[e][1::2])
            assert eq(dn[e, :d], sd[p + "mlp.experts.down_proj"][e].T) and eq(dnb[e, :d], sd[p + "mlp.experts.down_proj_bias"][e])
        assert not torch.equal(gu[0], gu[1])


def test_loader_refusals(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_gptoss(n_layers=2)
    assert cfg["model_type"] == "gpt_oss"
    n = [0]

    def both(match, c):
        with pytest.raises(ValueError, match=match):
            R.gptoss_dims(c)
        n[0] += 1
        sub = tmp_path / f"c{n[0]}"
        os.makedirs(sub)
        with open(sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(sub), device="cpu")
    both("hidden_act", cfg | {"hidden_act": "gelu"})
    both("head_dim", cfg | {"head_dim": 128})
    both("num_local_experts", cfg | {"num_local_experts": 129})
    both("num_local_experts", cfg | {"num_local_experts": 0})
    both("num_experts_per_tok", cfg | {"num_experts_per_tok": 9, "num_local_experts": 16})
    both("num_experts_per_tok", cfg | {"num_experts_per_tok": 0})
    both("num_experts_per_tok", cfg | {"num_experts_per_tok": 5, "num_local_experts": 4})
    both("hidden_size 200", cfg | {"hidden_size": 200})
    both("intermediate_size 72", cfg | {"intermediate_size": 72})
    both("attention_bias", cfg | {"attention_bias": False})
    both("layer_types", cfg | {"layer_types": ["sliding_attention", "chunked_attention"]})
    both("layer_types", cfg | {"layer_types": ["sliding_attention"]})
    both("sliding_window", cfg | {"sliding_window": 0})
    both("sliding_window", cfg | {"sliding_window": None})
    both("rope_type", cfg | {"rope_parameters": {"rope_type": "llama3", "factor": 8.0, "rope_theta": 1e4}})
    both("rope_type", cfg | {"rope_parameters": {"rope_type": "linear", "factor": 2.0, "rope_theta": 1e4}})
    both("tie_word_embeddings", cfg | {"tie_word_embeddings": True})
    both("num_key_value_heads", cfg | {"num_key_value_heads": 3})
    # limits: 128 experts and top-8 are accepted; Mixtral's stay 64
    big = R.gptoss_dims(cfg | {"num_local_experts": 128, "num_experts_per_tok": 8})
    assert (big["n_experts"], big["top_k"]) == (128, 8) and R.MIXTRAL_MAX_EXPERTS == 64 and R.GPTOSS_MAX_EXPERTS == 128
    # the window does not lower max_pos; max_positions caps it; full layers need no window
    assert R.gptoss_dims(cfg)["max_pos"] == 512 and R.gptoss_dims(cfg, max_positions=64)["max_pos"] == 64
    assert R.gptoss_dims(cfg | {"sliding_window": None, "layer_types": ["full_attention"] * 2})["windows"] == [0, 0]
    assert R.gptoss_dims(cfg | {"layer_types": None})["windows"] == [16, 0]
    # the context cache is refused, and says so, before any weight is read
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="context cache .* not supported for this family"):
        R.build_scorer(str(bare), device="cuda", context_cache_tokens=64)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    # the unsupported-type message names this family in its middle
    os.makedirs(tmp_path / "other")
    with open(tmp_path / "other" / "config.json", "w") as f:
        json.dump(cfg | {"model_type": "gpt_oss_2"}, f)
    with pytest.raises(ValueError, match=r"is not supported \(opt, gpt2, gpt_neox, llama.*, gemma2, phi3, gpt_oss, olmo2, mixtral\)$"):
        R.build_scorer(str(tmp_path / "other"), device="cpu")
    # the layout: every tensor is required; a non-finite sink and a value that does not survive the cast are refused by name
    st = state_of(model, False)
    dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
    for lack in ("self_attn.sinks", "mlp.router.bias", "experts.down_proj_bias", "o_proj.bias", "lm_head.weight"):
        with pytest.raises(KeyError, match=lack):
            R.gptoss_device_layout({k: v for k, v in st.items() if not k.endswith(lack)}, dims, rope)
    bad = st["model.layers.1.self_attn.sinks"].clone()
    bad[2] = float("inf")
    with pytest.raises(ValueError, match=r"model.layers.1.self_attn.sinks"):
        R.gptoss_device_layout(dict(st, **{"model.layers.1.self_attn.sinks": bad}), dims, rope)
    with pytest.raises(ValueError, match="gate_up_proj: shape"):
        R.gptoss_device_layout(dict(st, **{"model.layers.0.mlp.experts.gate_up_proj": st["model.layers.0.mlp.experts.gate_up_proj"][:3]}),
                               dims, rope)
    _, packed = mxfp4_state(st)
    k = "model.layers.0.mlp.experts.down_proj_scales"
    huge = packed[k].clone()
    huge[0, 0, 0] = 127 + 16          # 6 * 2^16 is not an fp16 number
    assert R.gptoss_device_layout(dict(packed, **{k: huge}), dims, rope, "bfloat16")["layers.0.down_w"].isfinite().all()
    with pytest.raises(ValueError, match="down_proj_blocks / _scales: a value is not finite"):
        R.gptoss_device_layout(dict(packed, **{k: huge}), dims, rope, "float16")
    with pytest.raises(ValueError, match="down_proj_blocks / _scales: shapes"):
        R.gptoss_device_layout(dict(packed, **{k: huge[:, :, :1]}), dims, rope)


def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    import b2t_native as N
    model, cfg = tiny_gptoss(fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.GptOssScorer) and isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu"
        assert sc._family == "gptoss" and sc._SIZES == "b2t_clm_gptoss_" and sc._qk == (sc._oss,) and sc._size_args == (sc._oss,)
        assert sc.desc.n_heads == 4 and sc.desc.n_kv_heads == 2 and sc.desc.d_model == 192 and sc.desc.ffn_dim == 64
        oss = sc._oss
        assert isinstance(oss, N.ClmGptOss) and (oss.head_dim, oss.n_experts, oss.top_k, oss.gate_up_stride, oss.down_stride) == (64, 8, 4, 256, 256)
        assert oss.swiglu_limit == 7.0 and not oss.route_out
        for l in range(2):
            assert sc.desc.layers_host[l].qkv_b == sc.w[f"layers.{l}.qkv_b"].data_ptr()
            assert oss.layers_host[l].window == (16, 0)[l] and oss.layers_host[l].sinks == sc.w[f"layers.{l}.sinks"].data_ptr()
            assert oss.layers_host[l].down_b == sc.w[f"layers.{l}.down_b"].data_ptr() and sc.w[f"layers.{l}.sinks"].dtype is torch.float32
            assert sc.w[f"layers.{l}.router_b"].dtype is want
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    with pytest.raises(ValueError, match="context cache"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    with pytest.raises(ValueError, match="context cache"):
        R.GptOssScorer(sc.dims, {}, "cpu", context_cache_tokens=1)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_bf16", "score_tree_bf16")
SIZES = ("ws_bytes", "tree_ws_bytes")


def _oss(n_layers=1, ne=8, k=2, gus=1024, dns=256, hd=64, limit=7.0, layers=True, window=0, **null):
    import b2t_native as N
    arr = (N.ClmGptOssLayer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmGptOssLayer._fields_[:-1]:
            setattr(arr[i], f, None if null.get(f) else FAKE)
        arr[i].window = window
    o = N.ClmGptOss(hd, limit, ne, k, gus, dns, None, arr if layers else None)
    o._keep = arr
    return o


def _wide(**kw):
    """a Llama descriptor whose head count goes with head dim 64 the gpt-oss way: d 256, 8 heads of 64"""
    return _model(**dict(dict(d=256, heads=8, kv=2, ffn=512), **kw))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_entry_points_are_declared_and_bound(tmp_path):
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY + SIZES:     # the Llama twin's list with the descriptor after the model
        new, twin = "b2t_clm_gptoss_" + t, "b2t_clm_llama_" + t
        want = decl(twin)
        assert decl(new) == want[:1] + ["const b2t_clm_gptoss_t* oss"] + want[1:], new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == [g.argtypes[0], C.POINTER(N.ClmGptOss)] + list(g.argtypes[1:])
    names = sorted("b2t_clm_gptoss_" + t for t in ENTRY + SIZES)
    assert sorted(set(re.findall(r"\b(b2t_clm_gptoss_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))) == names
    assert set(names) <= set(N.header_symbols())
    # the structs' layout against the C compiler
    body = ""
    for tag, c, py in (("L", "b2t_clm_gptoss_layer_t", N.ClmGptOssLayer), ("D", "b2t_clm_gptoss_t", N.ClmGptOss)):
        body += f'printf("{tag} %zu\\n", sizeof({c}));' + "".join(f'printf("{tag}.{f} %zu\\n", offsetof({c}, {f}));' for f, _ in py._fields_)
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){' + body + "return 0;}")
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "lay")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "lay")], text=True).splitlines())
    for tag, py in (("L", N.ClmGptOssLayer), ("D", N.ClmGptOss)):
        assert int(got[tag]) == C.sizeof(py)
        for f, _ in py._fields_:
            assert int(got[f"{tag}.{f}"]) == getattr(py, f).offset, f
    assert len(N.ClmGptOssLayer._fields_) == 7 and len(N.ClmGptOss._fields_) == 8


def test_sizes():
    """ws = the Llama layout with the QKV width (Hq + 2 Hkv) 64 and no dense hidden rows, + the attention output
    [round_up(rows, 256)][Hq 64] + the region of S = round_up(rows * top_k, 256) + 256 * n_experts sorted rows, on both paths;
    non-decreasing in the rows; 0 on invalid input."""
    import b2t_native as N
    lib = N.load()
    al = lambda x: -(-x // 256) * 256
    for kw, ne, k in ((dict(d=192, heads=4, kv=2, ffn=64), 8, 4), (dict(d=256, heads=8, kv=2, ffn=512), 128, 4),
                      (dict(d=256, heads=4, kv=4, ffn=128), 8, 8)):
        desc, oss = _model(bias=True, **kw), _oss(ne=ne, k=k)
        d, F, Hq, Hkv = kw["d"], kw["ffn"], kw["heads"], kw["kv"]
        p, q = C.byref(desc), C.byref(oss)

        def region(rows):
            n = rows * k
            S = al(n) + 256 * ne
            return 3 * al(4 * n) + al(4 * S) + al(4 * (S // 128)) + al(2 * S * d) + al(2 * S * F) + al(4 * S * d)
        last = 0
        for M in (1, 2, 127, 128, 129, 256, 257, 692):
            for n_seq in sorted({1, max(1, M // 3), M}):
                Mp = al(M)
                llama = lib.b2t_clm_llama_ws_bytes(p, M, n_seq)
                # the Llama layout's qkv is [M][(Hq + 2 Hkv) d / Hq] and it has hidden rows [Mp][F]
                want = llama - al(2 * M * (Hq + 2 * Hkv) * (d // Hq)) + al(2 * M * (Hq + 2 * Hkv) * 64) - al(2 * Mp * F) \
                    + al(2 * Mp * Hq * 64) + region(M)
                assert lib.b2t_clm_gptoss_ws_bytes(p, q, M, n_seq) == want, (kw, M, n_seq)
                for rows in sorted({1, M // 2 + 1, M}):
                    Rp = al(rows)
                    want = lib.b2t_clm_llama_tree_ws_bytes(p, rows, M, n_seq) - al(2 * rows * (Hq + 2 * Hkv) * (d // Hq)) \
                        + al(2 * rows * (Hq + 2 * Hkv) * 64) - al(2 * Rp * F) + al(2 * Rp * Hq * 64) + region(rows)
                    assert lib.b2t_clm_gptoss_tree_ws_bytes(p, q, rows, M, n_seq) == want
            now = lib.b2t_clm_gptoss_ws_bytes(p, q, M, 1)
            assert now >= last > -1
            last = now
    desc, oss = _wide(), _oss()
    p, q = C.byref(desc), C.byref(oss)
    assert lib.b2t_clm_gptoss_ws_bytes(p, q, 10, 1) > 0
    assert lib.b2t_clm_gptoss_ws_bytes(None, q, 10, 1) == 0 and lib.b2t_clm_gptoss_ws_bytes(p, None, 10, 1) == 0
    assert lib.b2t_clm_gptoss_tree_ws_bytes(None, q, 5, 10, 1) == 0 and lib.b2t_clm_gptoss_tree_ws_bytes(p, None, 5, 10, 1) == 0
    for ne, k, hd in ((0, 1, 64), (129, 2, 64), (8, 0, 64), (8, 9, 64), (4, 5, 64), (8, 2, 128)):
        bad = C.byref(_oss(ne=ne, k=k, hd=hd))
        assert lib.b2t_clm_gptoss_ws_bytes(p, bad, 10, 1) == 0 and lib.b2t_clm_gptoss_tree_ws_bytes(p, bad, 5, 10, 1) == 0, (ne, k, hd)
    assert lib.b2t_clm_gptoss_ws_bytes(p, C.byref(_oss(ne=128, k=8)), 10, 1) > 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert lib.b2t_clm_gptoss_ws_bytes(p, q, n_tok, n_seq) == 0
    for nn, nt, ns in ((0, 5, 1), (6, 5, 1), (5, 0, 1), (3, 5, 0), (3, 5, 6)):
        assert lib.b2t_clm_gptoss_tree_ws_bytes(p, q, nn, nt, ns) == 0


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """Everything the descriptors can have wrong and everything the Llama twin refuses of a list, with fake pointers and no GPU;
    the list's and the workspace's messages carry the call's own name."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_gptoss_" + entry
    fn = getattr(lib, who)
    tree = "tree" in entry
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]
    NOM = object()

    def refused(match, desc, oss=NOM, ids=ok_ids, off=ok_off, own=True, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        n = len(off) - 1 if n_seq is None else n_seq
        dp = C.byref(desc) if desc is not None else None
        q = _oss(desc.n_layers if desc is not None else 1) if oss is NOM else oss
        if tree:
            rc = fn(dp, q, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
        else:
            rc = fn(dp, q, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        assert N.last_error().startswith((who + ":") if own else "b2t_clm_gptoss:"), N.last_error()

    refused("null model", None, own=False)
    refused("null gptoss descriptor", _wide(), oss=None, own=False)
    refused("bad dimensions", _wide(kv=0), own=False)
    refused("head dim 128", _wide(), oss=_oss(hd=128), own=False)
    refused("multiple of n_kv_heads", _wide(kv=3), own=False)
    refused("multiples of 64", _wide(ffn=500), own=False)
    refused("rms_eps", _wide(eps=-1.0), own=False)
    for ne in (0, -3, 129):
        refused(f"n_experts {ne} outside", _wide(), oss=_oss(ne=ne), own=False)
    for ne, k in ((8, 0), (8, 9), (4, 5), (128, -1)):
        refused(f"top_k {k} outside", _wide(), oss=_oss(ne=ne, k=k), own=False)
    refused("expert strides 0 / 256", _wide(), oss=_oss(gus=0), own=False)
    refused("expert strides 1024 / 0", _wide(), oss=_oss(dns=0), own=False)
    refused("expert strides 768 / 256", _wide(), oss=_oss(gus=768), own=False)
    refused("swiglu_limit", _wide(), oss=_oss(limit=0.0), own=False)
    refused("null weight pointer", _wide(), oss=_oss(layers=False), own=False)
    for f in ("sinks", "o_b", "router_w", "router_b", "gate_up_b", "down_b"):
        refused("null weight pointer in layer 0", _wide(), oss=_oss(**{f: True}), own=False)
    bad = _wide()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad, own=False)
    refused("layer 0 has no q / k / v biases", _wide(bias=False), own=False)
    refused("window -1", _wide(), oss=_oss(window=-1), own=False)
    # the list's
    refused("null argument", _wide(), scores=None)
    refused("null argument", _wide(), ws=None)
    refused("n_seq 0", _wide(), n_seq=0)
    refused("empty", _wide(), off=[0, 1, 1, 4])
    refused("outside", _wide(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", _wide(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    # the workspace: this family's size functions
    desc, oss = _wide(), _oss()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes
    p, q = C.byref(desc), C.byref(oss)
    need = lib.b2t_clm_gptoss_tree_ws_bytes(p, q, 4, 9, 3) if tree else lib.b2t_clm_gptoss_ws_bytes(p, q, 9, 3)
    assert need > 0
    refused("workspace", desc, oss, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_gptoss_unit_kernels_without_scratch():
    """The unit instantiates the grouped GEMM with EP_OSS_GLU (14) and EP_F32_BIAS (15) on two tiles and in two element types, the
    router, the gather, the flat and the tree attention with sink and window in two element types, the plan and combine kernels
    once, and nothing else: 18 kernels, ScratchSize 0."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_gptoss.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_gptoss.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_grouped_kernel" in k]
    assert len(res) == 18 and len(gemm) == 8 and not [k for k in res if "clm_gemm_kernel" in k], sorted(res)
    assert sum("ELi14E" in k for k in gemm) == 4 and sum("ELi15E" in k for k in gemm) == 4
    assert sum("ILi256ELi256E" in k for k in gemm) == 4 and sum("ILi128ELi128E" in k for k in gemm) == 4
    for kern, n in (("clm_gptoss_route_kernel", 2), ("clm_moe_gather_kernel", 2), ("clm_moe_plan_kernel", 1), ("clm_moe_combine_kernel", 1),
                    ("clm_attn_sink_kernelILi64E", 2), ("clm_attn_tree_sink_kernelILi64E", 2)):
        assert sum(kern in k for k in res) == n, (kern, sorted(res))
    assert not [k for k in res if "clm_moe_route_kernel" in k]
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_gptoss_unit_uses_the_one_tile_rule():
    """Both grouped GEMMs go through causal_lm.hip's launch_gemm, and the host never reads the routing back: no copy, no
    synchronisation, no allocation and no atomics in the unit or in clm_gptoss.h."""
    csrc = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")
    src = open(os.path.join(csrc, "causal_lm_gptoss.hip")).read()
    hdr = open(os.path.join(csrc, "clm_gptoss.h")).read()
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src + hdr
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_OSS_GLU, El, true>)") == 1
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_F32_BIAS, El, true>)") == 1
    for word in ("hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc", "hipEventSynchronize", "atomicAdd",
                 "atomic_", "__atomic", "__hip_atomic"):
        assert word not in src and word not in hdr, word


# ---- the precondition of the GPU test's routed-differently share ---------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_route_share_precondition(fmt):
    """share_ref, the share of (layer, row) pairs that the rounded restatement routes unlike the unrounded one (order of choice
    included), is at most 2 % in both formats on the contract's inputs (the GPU contract model: layer 0 sliding at W = 40).  The
    router's bias, N(0, 0.5), is exact in either restatement, so the spread of the logits that the roundings do not move grows
    with it while e_router grows with the weights' scale alone: ROUTER_SCALE = 0.125 is what keeps the share here.  Also the caps
    on e that the GPU bounds rely on."""
    model, cfg, st, rd, rope = gptoss_state(fmt, sliding_window=40)
    seqs = contract_seqs(cfg["vocab_size"])
    e, e_router, share_ref, lg0, _ = gptoss_figures(st, rd, rope, seqs, fmt)
    gap = float((gap_behind_choice(lg0, rd["top_k"]) > 3 * e_router).mean())
    print(f"CLM gptoss preconditions {fmt}: e {e:.3e}  e_router {e_router:.3e}  share_ref {share_ref:.4f}  "
          f"share of gaps above 3 e_router behind the choice {gap:.4f}")
    assert sum(map(len, seqs)) == 418 and rd["windows"] == [40, 0]
    assert share_ref <= SHARE_REF_MAX, share_ref
    assert e_router > 0
    if fmt == "float16":
        assert E16_CAP[0] < e < E16_CAP[1], e
    else:
        assert 0 < e <= E_BF16_MAX, e
