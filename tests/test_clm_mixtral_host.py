"""Host-side checks of the Mixtral rescorer (csrc/causal_lm_mixtral.hip, csrc/clm_moe.h, "mixtral" in llm_rescore; no GPU): the
float64 restatement of the contract (ref_logp_mixtral_fmt, the reference of tests/test_gpu_clm_mixtral.py) against HF's
MixtralForCausalLM (its forward evaluated in float64, and in fp32), the preconditions of the GPU bounds (e16, e_bf16, and the
router's: how far the roundings move a logit, how many rows the rounded restatement then routes unlike the unrounded one, and
how wide the gap behind the last chosen expert is beside that), the loader on both spellings of a checkpoint, the refusals, the eight entry points' declarations, bindings, sizes and
refusals before any device work, the kernels of the translation unit and a scorer on the CPU.

The tiny model (tiny_mixtral) is a random HF MixtralForCausalLM built in memory with tiny_model's recipe
(tests/test_clm_llama_host.py): d 128, 2 heads, 1 kv head, F 192, 4 experts, top-2, 2 layers, vocab 300.  The expert strides
round_up(2F, 256) = 512 and round_up(d, 256) = 256 differ from 2F = 384 and d = 128."""
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

TINY = dict(hidden_size=128, num_attention_heads=2, num_key_value_heads=1, intermediate_size=192, num_local_experts=4,
            num_experts_per_tok=2, vocab_size=300, max_position_embeddings=256, sliding_window=None, tie_word_embeddings=False,
            rms_norm_eps=1e-5)
HOST_LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # 692 rows
SEED = {"float16": 1, "bfloat16": 9}   # the committed seeds (test_router_preconditions / test_bf16_preconditions: what they give)
HF_BOUND = 1e-9      # the unrounded restatement is HF's forward of the fp32 model (evaluated in float64: hf_logp_float64)
E16_CAP = (1e-5, 1e-2)   # tests/test_clm_llama_host.py: 1e-5 < e16 < 1e-2
E_BF16_MAX = 0.1         # tests/test_clm_llama_bf16_host.py
GAP_SHARE = 0.99         # of the (layer, row) pairs have a gap above 3 e_router behind the last chosen expert


def tiny_mixtral(n_layers=2, fmt="float16", seed=0, **over):
    """tiny_model's recipe (tests/test_clm_llama_host.py) for TINY: (HF fp32 CPU MixtralForCausalLM in eval mode with random
    weights representable in fmt, its config as the dict of config.json).  A weight is N(0, 1) / sqrt(fan-in); the fan-in of the
    3-D expert tensors ([E][2F][d], [E][d][F]) is their LAST dimension, not shape[1]."""
    import torch
    import transformers
    kw = dict(TINY, **over)
    cfg = transformers.MixtralConfig(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(seed)
    model = transformers.MixtralForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(500 + seed)
    rdt = getattr(torch, fmt)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("norm.weight") or "layernorm" in k:
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif "embed_tokens" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[-1] ** 0.5
            p.copy_(v.to(rdt).float())
    return model, json.loads(cfg.to_json_string())


def fused_state(st, cfg):
    """The state dict in the fused spelling (mlp.gate.weight, mlp.experts.gate_up_proj, mlp.experts.down_proj) whichever
    spelling `st` has."""
    import torch
    ne = cfg["num_local_experts"]
    out = {}
    for k, v in st.items():
        m = re.match(r"(model\.layers\.\d+\.)block_sparse_moe\.(.*)", k)
        if not m:
            out[k] = v
        elif m.group(2) == "gate.weight":
            out[m.group(1) + "mlp.gate.weight"] = v
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{l}."
        if p + "mlp.experts.gate_up_proj" in out:
            continue
        e = lambda i, w: st[p + f"block_sparse_moe.experts.{i}.{w}.weight"]
        out[p + "mlp.experts.gate_up_proj"] = torch.stack([torch.cat([e(i, "w1"), e(i, "w3")], 0) for i in range(ne)])
        out[p + "mlp.experts.down_proj"] = torch.stack([e(i, "w2") for i in range(ne)])
    return out


def published_state(st, cfg):
    """The state dict in the published spelling (block_sparse_moe.gate.weight, block_sparse_moe.experts.<e>.w1 / w3 / w2.weight)."""
    F = cfg["intermediate_size"]
    out = {}
    for k, v in fused_state(st, cfg).items():
        m = re.match(r"(model\.layers\.\d+\.)mlp\.(.*)", k)
        if not m:
            out[k] = v
        elif m.group(2) == "gate.weight":
            out[m.group(1) + "block_sparse_moe.gate.weight"] = v
        elif m.group(2) == "experts.gate_up_proj":
            for e in range(v.shape[0]):
                out[m.group(1) + f"block_sparse_moe.experts.{e}.w1.weight"] = v[e, :F].contiguous()
                out[m.group(1) + f"block_sparse_moe.experts.{e}.w3.weight"] = v[e, F:].contiguous()
        else:
            for e in range(v.shape[0]):
                out[m.group(1) + f"block_sparse_moe.experts.{e}.w2.weight"] = v[e].contiguous()
    return out


def mixtral_ref_dims(cfg):
    return dict(ref_dims(cfg), n_experts=cfg["num_local_experts"], top_k=cfg["num_experts_per_tok"])


def ref_logp_mixtral_fmt(st, dims, inv_freq, seqs, fmt=None, routes=None):
    """The float64 restatement of include/b2t.h's Mixtral contract, in the style of ref_logp_llama_fmt
    (tests/test_clm_llama_bf16_host.py): fmt = None rounds nowhere; "float16" / "bfloat16" round where the kernels round -- the
    RMSNorm outputs (x, the operand of the router and of the experts alike), q, k, v, P per 32-key block, the attention output,
    silu(gate) * up -- and never the router's logits, the weights or an expert's output.  `st` is a state dict in the fused
    spelling (fused_state).  routes, when given, is an int array [n_layers][rows][top_k] that forces the expert ids of every
    (layer, row), in order of choice; the weights are still computed from the restatement's own logits of the forced experts.
    Returns (per-sequence log-probs, router logits [n_layers][rows][n_experts], free choice [n_layers][rows][top_k]) -- the
    free choice is what repeated argmax with a strict `>` takes from the restatement's own logits."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    rnd = (lambda t: t) if fmt is None else (lambda t: t.to(R.clm_dtype(fmt)).double())
    d, Hq, Hkv, nl, V, eps = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "n_layers", "vocab", "rms_eps"))
    ne, topk, Fd = dims["n_experts"], dims["top_k"], dims["ffn_dim"]
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
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    logits_out, free_out = [], []
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(rms(x, p + "input_layernorm.weight"))
        q = rnd(rot(lin(h, p + "self_attn.q_proj").view(M, Hq, hd)) * hd ** -0.5)
        k = rnd(rot(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd)))
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
        lg = h @ W(p + "mlp.gate.weight").T                             # [M, ne], never rounded
        work, free = lg.clone(), []
        for _ in range(topk):                                           # repeated argmax; torch's argmax takes the first maximum
            e = work.argmax(-1)
            free.append(e)
            work.scatter_(1, e[:, None], float("-inf"))
        free = torch.stack(free, 1)
        ch = free if routes is None else torch.as_tensor(np.ascontiguousarray(routes[l], dtype=np.int64), device=dev)
        sel = lg.gather(1, ch)
        wt = torch.exp(sel - sel[:, :1])
        wt = wt / wt.sum(-1, keepdim=True)
        gu, dn = W(p + "mlp.experts.gate_up_proj"), W(p + "mlp.experts.down_proj")
        y = torch.zeros(M, d, dtype=torch.float64, device=dev)
        for j in range(topk):                                           # in order of choice
            yj = torch.empty(M, d, dtype=torch.float64, device=dev)
            for e in range(ne):
                rows = (ch[:, j] == e).nonzero()[:, 0]
                if rows.numel():
                    g_u = h[rows] @ gu[e].T
                    gate, up = g_u[:, :Fd], g_u[:, Fd:]
                    yj[rows] = rnd(gate * torch.sigmoid(gate) * up) @ dn[e].T
            y = wt[:, j:j + 1] * yj if j == 0 else y + wt[:, j:j + 1] * yj
        x = x + y
        logits_out.append(lg.cpu().numpy())
        free_out.append(free.cpu().numpy())
    logits_out, free_out = np.stack(logits_out), np.stack(free_out)
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out, logits_out, free_out
    tgt = ids[src + 1]
    h = rnd(rms(x[src], "model.norm.weight"))
    E = st["lm_head.weight"] if "lm_head.weight" in st else st["model.embed_tokens.weight"]
    lp = ((h * E[tgt].double()).sum(-1) - torch.logsumexp(h @ E.double().T, -1)).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out, logits_out, free_out


def gap_behind_choice(logits, top_k):
    """[n_layers][rows]: the k-th largest logit minus the (k + 1)-th (inf where top_k experts are all there are)."""
    s = -np.sort(-logits, axis=-1)
    return s[..., top_k - 1] - s[..., top_k] if logits.shape[-1] > top_k else np.full(logits.shape[:-1], np.inf)


def mixtral_state(fmt="float16", seed=None, **kw):
    """(model, cfg, state dict in the fused spelling, reference dims, inv_freq) of the tiny model with fmt-valued weights"""
    model, cfg = tiny_mixtral(fmt=fmt, seed=SEED[fmt] if seed is None else seed, **kw)
    return model, cfg, fused_state(state_of(model, cfg["tie_word_embeddings"]), cfg), mixtral_ref_dims(cfg), hf_inv_freq(model)


def router_figures(st, rd, inv, seqs, fmt):
    """(rounded restatement, unrounded restatement, e, e_router, share of pairs with a gap above 3 e_router, same routing) of
    one case: everything the GPU bounds are made of, restatement against restatement."""
    exact, lg0, free0 = ref_logp_mixtral_fmt(st, rd, inv, seqs)
    rounded, lg1, free1 = ref_logp_mixtral_fmt(st, rd, inv, seqs, fmt, routes=free0)
    e = float(np.abs(np.concatenate(rounded) - np.concatenate(exact)).max())
    e_router = float(np.abs(lg1 - lg0).max())
    share = float((gap_behind_choice(lg0, rd["top_k"]) > 3 * e_router).mean())
    return rounded, exact, e, e_router, share, bool(np.array_equal(free0, free1)), lg1, free1


def _maxdiff(a, b):
    return float(max(np.abs(x - y).max() for x, y in zip(a, b)))


CONTRACT_LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65)   # 308 rows


def contract_seqs(V):
    """The sequences of the contract tests, here and on the GPU: 418 rows, shared prefixes and a duplicate."""
    seqs = tiny_seqs(V, seed=3, lens=CONTRACT_LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[7])]


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _hf_eager(model):
    model.config._experts_implementation = "eager"     # the loop over experts of modeling_mixtral.py, not a grouped_mm
    return model


def hf_logp_float64(model, seqs):
    """hf_logp of HF's forward evaluated in float64 throughout: the module's parameters and buffers widened (their values are
    the fp32 ones), and, while it runs, the three spellings by which modeling_mixtral.py asks for fp32 whatever the module's
    dtype -- Tensor.float() (rotary positions, the router's softmax), torch.float32 (RMSNorm, the attention softmax) and
    torch.float (inv_freq) -- give float64.  The code that runs is the library's; only its precision is lifted, so that a
    difference from the restatement is a difference of the function and not fp32 rounding (an fp32 log-prob of 13 is itself
    only good to 1e-6).  The module is returned to fp32 afterwards.
    Written against modeling_mixtral.py of transformers 5.15.0, where these three are every fp32 cast of the forward.  A
    release that spells one differently (say torch.to(dtype=...) from a module-level constant) leaves an fp32 island, which
    shows as a difference of 1e-7 .. 1e-5 in test_unrounded_restatement_equals_hf_to_1e_9: its message names the installed
    version and this function is the place to add the new spelling; a norm that does not see float64 is reported here."""
    import torch
    import transformers
    from unittest import mock
    wide = lambda t, *a, **k: t if t.dtype == torch.float64 else t.double()
    seen = []
    hook = model.model.norm.register_forward_hook(lambda mod, args, out: seen.append((args[0].dtype, out.dtype)))
    try:
        with mock.patch.object(torch.Tensor, "float", wide), mock.patch.object(torch, "float32", torch.float64), \
                mock.patch.object(torch, "float", torch.float64):
            out = hf_logp(_hf_eager(model).double(), seqs)
    finally:
        hook.remove()
        model.float()
    assert seen and all(d == (torch.float64, torch.float64) for d in seen), \
        f"transformers {transformers.__version__}: the final norm saw {set(seen)}, not float64: the patches no longer reach its fp32 casts"
    return out


def test_unrounded_restatement_equals_hf_to_1e_9():
    """The unrounded restatement is HF's forward of the fp32 model to 1e-9, HF's code evaluated in float64 (hf_logp_float64).
    Measured on the CPU (lengths 1..129, max |logp| 13.5): 1.1e-14.  The same module run in fp32 arithmetic is 7.0e-6 away
    (test_unrounded_restatement_equals_hf_fp32), and merely widened with .double() 3.8e-6, because the library keeps the rotary
    table, the norms and both softmaxes in fp32."""
    import torch
    model, cfg, st, rd, inv = mixtral_state()
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact = ref_logp_mixtral_fmt(st, rd, inv, seqs)[0]
    hf = hf_logp_float64(model, seqs)
    err, mx = _maxdiff(exact, hf), max(np.abs(b).max() for b in hf)
    print(f"CLM mixtral restatement vs HF's forward in float64: {err:.3e} (max |logp| {mx:.2f})")
    assert torch.ones(1).float().dtype is torch.float32 and next(model.parameters()).dtype is torch.float32   # the patches are gone
    import transformers
    assert mx > 5 and err <= HF_BOUND, \
        (f"{err:.3e} from HF's forward in float64 (transformers {transformers.__version__}; hf_logp_float64 was written against "
         "5.15.0): either the restatement is another function, or the library has a new fp32 cast that hf_logp_float64 misses")


HF_FP32_BOUND = 7.0e-5   # 10 x the measured 7.0e-6, never above 1e-4: the form of test_clm_llama_host.HF_BOUND


def test_unrounded_restatement_equals_hf_fp32():
    """Against HF's fp32 forward within 10 x the measured figure (7.0e-6), on both experts implementations of the library; a
    restatement with the two chosen experts exchanged in order is the same function, one with another expert is not."""
    model, cfg, st, rd, inv = mixtral_state()
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=HOST_LENS)
    exact, lg, free = ref_logp_mixtral_fmt(st, rd, inv, seqs)
    hf = hf_logp(model, seqs)
    err, mx = _maxdiff(exact, hf), max(np.abs(b).max() for b in hf)
    err_eager = _maxdiff(exact, hf_logp(_hf_eager(model), seqs))
    print(f"CLM mixtral restatement vs HF fp32: {err:.3e} (eager experts {err_eager:.3e}; max |logp| {mx:.2f})")
    assert mx > 5 and max(err, err_eager) <= HF_FP32_BOUND
    assert lg.shape == (2, 692, 4) and free.shape == (2, 692, 2)
    assert len({tuple(r) for r in free.reshape(-1, 2)}) == 12          # every ordered pair of the 4 experts is chosen
    forced = ref_logp_mixtral_fmt(st, rd, inv, seqs, routes=free)
    assert _maxdiff(forced[0], exact) == 0 and np.array_equal(forced[2], free)
    swapped = ref_logp_mixtral_fmt(st, rd, inv, seqs, routes=free[..., ::-1])[0]
    assert _maxdiff(swapped, exact) < 1e-12                             # the weights follow the experts
    other = ref_logp_mixtral_fmt(st, rd, inv, seqs, routes=(free + 1) % 4)[0]
    assert _maxdiff(other, exact) > 0.1


def test_router_preconditions():
    """What the GPU tests rely on, restatement against restatement on their sequences, for the committed seed of the float16
    model: e16 within the caps of tests/test_clm_llama_host.py (1e-5 < e16 < 1e-2); with e_router the largest difference between
    the rounded and the unrounded restatement's router logits under the same routes, the two choose the same experts in the
    same order for every (layer, row), and at least 99 % of the pairs have a gap above 3 e_router between the k-th and the
    (k + 1)-th logit.

    Measured on the CPU, 836 pairs, seed 1: e16 6.3e-3, e_router 2.6e-3, share 0.994, same routing (of seeds 0..11, eight keep
    the routing and seven reach 99 %)."""
    model, cfg, st, rd, inv = mixtral_state("float16")
    seqs = contract_seqs(cfg["vocab_size"])
    rounded, exact, e, e_router, share, same, _, _ = router_figures(st, rd, inv, seqs, "float16")
    print(f"CLM mixtral preconditions float16 seed {SEED['float16']}: e {e:.3e}  e_router {e_router:.3e}  share of gaps above "
          f"3 e_router {share:.4f}  same routing {same}")
    assert sum(map(len, seqs)) == 418
    assert E16_CAP[0] < e < E16_CAP[1], e
    assert e_router > 0
    assert same, "the rounded and the unrounded restatement route differently"
    assert share >= GAP_SHARE, share


BF16_E_ROUTER_MAX = E_BF16_MAX / 2   # a logit (spread 1) may move by half of what a log-prob may; seeds 0..11 give 0.020 .. 0.034
BF16_GAP_SHARE = 0.85                # the gaps of four N(0, 1) logits have a density of about 1.3, so 3 e_router = 0.06 .. 0.10 covers
                                     # 8 - 13 % of them: seeds 0..11 give shares of 0.879 .. 0.927
BF16_DIFFER_MAX = 0.01               # the GPU test's own cap on pairs routed unlike the restatement; seeds 0..11 give 0.0024 .. 0.0108


def test_bf16_preconditions():
    """The bfloat16 model's, on the GPU test's sequences and its committed seed: 0 < e_bf16 <= 0.1 (the cap of
    tests/test_clm_llama_bf16_host.py), and what holds of the router in this format, pinned:
      - 0 < e_router <= 0.05;
      - the rounded restatement routes at most 1 % of the (layer, row) pairs unlike the unrounded one (order included);
      - every such pair lies across a gap of at most 2 e_router in the UNROUNDED logits -- no rounding moves a logit by more than
        e_router, so two experts can change places only if they were that close: a larger gap is a fault of the restatement;
      - at least 85 % of the pairs have a gap above 3 e_router behind the last chosen expert.
    The float16 conditions of test_router_preconditions (no pair routed differently, 99 %) cannot be met by any model of this
    recipe in bfloat16: rounding x alone to 8 bits of mantissa (relative 2^-9 per element) moves a logit of spread 1 by about
    1e-3 rms, 4e-3 at the largest of 3344, before any other rounding of two layers, and scaling the router scales e_router with
    the gaps.  The bfloat16 GPU test forces the kernel's own routes into the ROUNDED restatement and compares the kernel's choice
    with that restatement's free choice (both see the same rounded x), under the same 1 % and 3 e_router.

    Measured on the CPU, 836 pairs, seed 9: e_bf16 5.6e-2, e_router 2.0e-2, 2 pairs (0.24 %) routed differently across gaps of
    at most 0.42 e_router, share 0.927.  Seeds 0..11: e_router 2.0e-2 .. 3.4e-2, 0.24 .. 1.08 % of the pairs across at most
    0.84 e_router, share 0.879 .. 0.927."""
    model, cfg, st, rd, inv = mixtral_state("bfloat16")
    seqs = contract_seqs(cfg["vocab_size"])
    exact, lg0, free0 = ref_logp_mixtral_fmt(st, rd, inv, seqs)
    rounded, lg1, free1 = ref_logp_mixtral_fmt(st, rd, inv, seqs, "bfloat16", routes=free0)
    e = float(np.abs(np.concatenate(rounded) - np.concatenate(exact)).max())
    e_router = float(np.abs(lg1 - lg0).max())
    share = float((gap_behind_choice(lg0, rd["top_k"]) > 3 * e_router).mean())
    differ = free0 != free1                                             # [layers][rows][k]
    pick = lambda ids: np.take_along_axis(lg0, ids, -1)
    gaps = np.abs(pick(free0) - pick(free1))[differ]
    pairs = float(differ.any(-1).mean())
    print(f"CLM mixtral preconditions bfloat16 seed {SEED['bfloat16']}: e {e:.3e}  e_router {e_router:.3e}  share of gaps above "
          f"3 e_router {share:.4f}  pairs routed differently {int(differ.any(-1).sum())} of {differ.any(-1).size} ({pairs:.4f}), "
          f"largest gap among them {(gaps.max() if gaps.size else 0.0) / e_router:.3f} e_router")
    assert differ.any(-1).size == 836 and np.isfinite(np.concatenate(rounded)).all()
    assert 0 < e <= E_BF16_MAX, e
    assert 0 < e_router <= BF16_E_ROUTER_MAX, e_router
    assert pairs <= BF16_DIFFER_MAX, pairs
    assert not gaps.size or gaps.max() <= 2 * e_router, (gaps.max(), e_router)
    assert share >= BF16_GAP_SHARE, share


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_loader_layout_from_both_spellings(fmt, tmp_path):
    """Both spellings of a checkpoint give the same arrays bit for bit, from a state dict and from a directory; every array
    equals its state-dict tensor: the experts stacked with strides round_up(2F, 256) = 512 and round_up(d, 256) = 256, gate /
    up interleaved in blocks of 32 per expert, zero padding, q / k rows under qkv_row_perm."""
    import torch
    from safetensors.torch import save_file
    import llm_rescore as R
    model, cfg = tiny_mixtral(fmt=fmt)
    sd = state_of(model, False)
    fused, pub = fused_state(sd, cfg), published_state(sd, cfg)
    assert "model.layers.1.mlp.experts.gate_up_proj" in fused and "model.layers.1.block_sparse_moe.experts.3.w2.weight" in pub
    assert not any("block_sparse_moe" in k for k in fused) and not any(".mlp." in k for k in pub)
    dims, inv = R.mixtral_dims(cfg), R.rope_inv_freq(cfg)
    wdt = getattr(torch, fmt)
    a, b = R.mixtral_device_layout(fused, dims, inv, fmt), R.mixtral_device_layout(pub, dims, inv, fmt)
    for sub, state in (("fused", fused), ("published", pub)):
        os.makedirs(tmp_path / sub)
        with open(tmp_path / sub / "config.json", "w") as f:
            json.dump(cfg, f)
        save_file({k: v.contiguous() for k, v in state.items()}, str(tmp_path / sub / "model.safetensors"))
    model.save_pretrained(str(tmp_path / "hf"))       # whichever spelling the installed library writes
    loaded = [R.load_mixtral_arrays(str(tmp_path / sub), dtype=fmt) for sub in ("fused", "published", "hf")]
    for dm, arr in [(dims, b)] + loaded:
        assert dm == dims and sorted(arr) == sorted(a)
        for k in a:
            assert arr[k].dtype == a[k].dtype and arr[k].shape == a[k].shape and torch.equal(arr[k], a[k]), k
    assert dims["n_experts"] == 4 and dims["top_k"] == 2 and dims["max_pos"] == 256 and R.mixtral_strides(dims) == (512, 256)
    d, Fd, ne, V = 128, 192, 4, 300
    eq = lambda x, y: x.dtype == wdt and torch.equal(x, y.to(wdt)) and torch.equal(x.float(), y)   # bit for bit, and exact
    assert a["embed_tokens"].shape == (512, d) and eq(a["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert eq(a["lm_head"][:V], sd["lm_head.weight"]) and not a["lm_head"][V:].any()
    qperm = torch.from_numpy(R.qkv_row_perm(2, 1, 64))
    for l in range(2):
        p, g = f"model.layers.{l}.", lambda f: a[f"layers.{l}.{f}"]
        assert eq(g("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(g("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
        assert g("qkv_w").shape == (256, d) and eq(g("qkv_w"), qkv[qperm]) and f"layers.{l}.qkv_b" not in a
        assert g("o_w").shape == (256, d) and eq(g("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and not g("o_w")[d:].any()
        assert g("router_w").shape == (ne, d) and eq(g("router_w"), fused[p + "mlp.gate.weight"])
        gu, dn = g("gate_up_w"), g("down_w")
        assert gu.shape == (ne, 512, d) and dn.shape == (ne, 256, Fd) and gu.is_contiguous() and dn.is_contiguous()
        assert not gu[:, 2 * Fd:].any() and not dn[:, d:].any()
        for e in range(ne):
            blocks = gu[e, :2 * Fd].view(Fd // 32, 2, 32, d)
            assert eq(blocks[:, 0].reshape(Fd, d), pub[p + f"block_sparse_moe.experts.{e}.w1.weight"])      # gate
            assert eq(blocks[:, 1].reshape(Fd, d), pub[p + f"block_sparse_moe.experts.{e}.w3.weight"])      # up
            assert eq(dn[e, :d], pub[p + f"block_sparse_moe.experts.{e}.w2.weight"])                         # down
        assert not torch.equal(gu[0], gu[1])


def test_loader_refusals(tmp_path):
    import llm_rescore as R
    model, cfg = tiny_mixtral(n_layers=1)
    assert cfg["model_type"] == "mixtral" and "mixtral" not in R.LLAMA_MODEL_TYPES
    with pytest.raises(ValueError, match="model_type 'mixtral'"):       # llama_dims stays as it is
        R.llama_dims(cfg)
    n = [0]

    def both(match, c):
        with pytest.raises(ValueError, match=match):
            R.mixtral_dims(c)
        n[0] += 1
        sub = tmp_path / f"c{n[0]}"
        os.makedirs(sub)
        with open(sub / "config.json", "w") as f:
            json.dump(c, f)
        with pytest.raises(ValueError, match=match):
            R.build_scorer(str(sub), device="cpu")
    plain = {k: v for k, v in cfg.items() if k not in ("rope_parameters", "rope_scaling")} | {"rope_theta": 10000.0}
    both("hidden_act", cfg | {"hidden_act": "gelu"})
    both("head_dim", cfg | {"head_dim": 32})
    both("head_dim", cfg | {"hidden_size": 320, "num_attention_heads": 4, "num_key_value_heads": 4})     # 80
    both("num_local_experts", cfg | {"num_local_experts": 65})
    both("num_local_experts", cfg | {"num_local_experts": 0})
    both("num_experts_per_tok", cfg | {"num_experts_per_tok": 5})
    both("num_experts_per_tok", cfg | {"num_experts_per_tok": 0})
    both("num_experts_per_tok", cfg | {"num_local_experts": 16, "num_experts_per_tok": 9})
    both("attention_bias", cfg | {"attention_bias": True})
    both("mlp_bias", cfg | {"mlp_bias": True})
    both("rope_type", plain | {"rope_scaling": {"rope_type": "yarn", "factor": 2.0}})
    both("rope_type", plain | {"rope_scaling": {"type": "linear", "factor": 2.0}})
    both("num_key_value_heads", cfg | {"num_attention_heads": 2, "num_key_value_heads": 3})
    both("intermediate_size 200", cfg | {"intermediate_size": 200})
    R.mixtral_dims(plain | {"rope_scaling": {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0,
                                             "high_freq_factor": 4.0, "original_max_position_embeddings": 64}})
    assert R.mixtral_dims(cfg | {"num_local_experts": 64, "num_experts_per_tok": 8})["top_k"] == 8
    # sliding_window lowers max_pos as for Mistral; max_positions caps it
    assert R.mixtral_dims(cfg | {"sliding_window": 100})["max_pos"] == 100 and R.mixtral_dims(cfg)["max_pos"] == 256
    assert R.mixtral_dims(cfg, max_positions=64)["max_pos"] == 64
    # the neighbours stay unsupported model types, and the message names this one at its end
    for mt in ("qwen3_moe", "olmoe"):
        os.makedirs(tmp_path / mt)
        with open(tmp_path / mt / "config.json", "w") as f:
            json.dump(cfg | {"model_type": mt}, f)
        with pytest.raises(ValueError, match=f"model_type '{mt}' is not supported .*olmo2, mixtral\\)$"):
            R.build_scorer(str(tmp_path / mt), device="cpu")
    bare = tmp_path / "bare"
    os.makedirs(bare)
    with open(bare / "config.json", "w") as f:
        json.dump(cfg, f)
    for dt in (None, "bfloat16", "auto"):
        with pytest.raises(FileNotFoundError):
            R.build_scorer(str(bare), device="cpu", dtype=dt)
    with pytest.raises(ValueError, match="follow-up"):     # bf16 with a cache stays refused
        R.build_scorer(str(bare), device="cuda", dtype="bfloat16", context_cache_tokens=64)
    # the layout: every tensor is required, any bias refused, by name
    st = fused_state(state_of(model, False), cfg)
    dims, inv = R.mixtral_dims(cfg), R.rope_inv_freq(cfg)
    for lack in ("mlp.gate.weight", "experts.down_proj", "post_attention_layernorm"):
        with pytest.raises(KeyError, match=lack):
            R.mixtral_device_layout({k: v for k, v in st.items() if lack not in k}, dims, inv)
    pub = published_state(st, cfg)
    with pytest.raises(KeyError, match="experts.2.w3.weight"):
        R.mixtral_device_layout({k: v for k, v in pub.items() if "experts.2.w3" not in k}, dims, inv)
    for bias in ("self_attn.q_proj.bias", "self_attn.o_proj.bias", "mlp.gate.bias", "block_sparse_moe.experts.0.w1.bias"):
        with pytest.raises(ValueError, match=bias):
            R.mixtral_device_layout(dict(st, **{"model.layers.0." + bias: st["model.norm.weight"]}), dims, inv)
    with pytest.raises(ValueError, match="gate_up_proj: shape"):
        R.mixtral_device_layout(dict(st, **{"model.layers.0.mlp.experts.gate_up_proj": st["model.layers.0.mlp.experts.gate_up_proj"][:3]}),
                                dims, inv)


def test_scorers_on_the_cpu(tmp_path):
    import torch
    import llm_rescore as R
    import b2t_native as N
    model, cfg = tiny_mixtral(fmt="bfloat16")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
        assert isinstance(sc, R.MixtralScorer) and isinstance(sc, R.LlamaScorer) and sc.dtype is want and str(sc.device) == "cpu"
        assert sc._family == "mixtral" and sc._SIZES == "b2t_clm_mixtral_" and R.LlamaScorer._SIZES == "b2t_clm_llama_"
        assert sc.desc.n_heads == 2 and sc.desc.n_kv_heads == 1 and sc.desc.d_model == 128 and sc.desc.ffn_dim == 192
        assert not sc.desc.layers_host[0].qkv_b
        moe = sc._moe
        assert isinstance(moe, N.ClmMoe) and (moe.n_experts, moe.top_k, moe.gate_up_stride, moe.down_stride) == (4, 2, 512, 256)
        assert not moe.route_out and sc._qk == (moe,) and sc._size_args == (moe,) and R.LlamaScorer._size_args == ()
        for l in range(2):
            assert moe.router_w_host[l] == sc.w[f"layers.{l}.router_w"].data_ptr()
            assert sc.desc.layers_host[l].gate_up_w == sc.w[f"layers.{l}.gate_up_w"].data_ptr()
            assert sc.w[f"layers.{l}.gate_up_w"].shape == (4, 512, 128) and sc.w[f"layers.{l}.router_w"].dtype is want
        assert sc.last_stats is None and sc.score([]).shape == (0,) and sc.eval() is sc
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    # Llama arrays are not Mixtral arrays
    from test_clm_llama_host import tiny_model
    m2, c2 = tiny_model("llama", n_layers=1)
    d2 = R.llama_dims(c2)
    with pytest.raises(KeyError, match="router_w"):
        R.MixtralScorer(d2, R.llama_device_layout(state_of(m2, False), d2, R.rope_inv_freq(c2)), "cpu")


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")
SIZES = ("ws_bytes", "tree_ws_bytes", "tree_cached_ws_bytes")


def _moe(n_layers=1, ne=8, k=2, gus=1024, dns=256, routers=True, router=FAKE):
    import b2t_native as N
    arr = (C.c_void_p * max(1, n_layers))()
    for i in range(n_layers):
        arr[i] = router
    m = N.ClmMoe(ne, k, arr if routers else None, gus, dns, None)
    m._keep = arr
    return m


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_entry_points_are_declared_and_bound(tmp_path):
    import subprocess
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY + SIZES:     # the Llama twin's list with the descriptor after the model
        new, twin = "b2t_clm_mixtral_" + t, "b2t_clm_llama_" + t
        want = decl(twin)
        assert decl(new) == want[:1] + ["const b2t_clm_moe_t* moe"] + want[1:], new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == [g.argtypes[0], C.POINTER(N.ClmMoe)] + list(g.argtypes[1:])
    names = sorted("b2t_clm_mixtral_" + t for t in ENTRY + SIZES)
    assert sorted(set(re.findall(r"\b(b2t_clm_mixtral_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))) == names
    assert set(names) <= set(N.header_symbols()) and "b2t_clm_mixtral_cache_kv_bytes" not in N.header_symbols()
    # the struct's layout
    fields = [n for n, _ in N.ClmMoe._fields_]
    body = "".join(f'printf("{f} %zu\\n", offsetof(b2t_clm_moe_t, {f}));' for f in fields)
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){'
                   'printf("size %zu\\n", sizeof(b2t_clm_moe_t));' + body + "return 0;}")
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "lay")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "lay")], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(N.ClmMoe) and len(fields) == 6
    for f in fields:
        assert int(got[f]) == getattr(N.ClmMoe, f).offset, f


def test_sizes():
    """ws = the Llama twin's, without the dense MLP's hidden rows [round_up(rows, 256)][F] that this forward never uses, + the
    region of S = round_up(rows * top_k, 256) + 256 * n_experts sorted rows, on all three paths; non-decreasing in the rows; 0 on
    invalid input."""
    import b2t_native as N
    lib = N.load()
    al = lambda x: -(-x // 256) * 256
    for kw, ne, k in ((dict(d=256, heads=4, kv=2, ffn=512), 8, 2), (dict(d=128, heads=2, kv=1, ffn=192), 4, 1),
                      (dict(d=512, heads=4, kv=4, ffn=448), 64, 8)):
        desc, moe = _model(bias=False, **kw), _moe(ne=ne, k=k)
        p, q = C.byref(desc), C.byref(moe)
        d, F = kw["d"], kw["ffn"]

        def extra(rows):
            n = rows * k
            S = al(n) + 256 * ne
            region = 3 * al(4 * n) + al(4 * S) + al(4 * (S // 128)) + al(2 * S * d) + al(2 * S * F) + al(4 * S * d)
            return region - al(2 * al(rows) * F)
        last = 0
        for M in (1, 2, 127, 128, 129, 255, 256, 257, 692, 4097):
            for n_seq in sorted({1, max(1, M // 3), M}):
                assert lib.b2t_clm_mixtral_ws_bytes(p, q, M, n_seq) == lib.b2t_clm_llama_ws_bytes(p, M, n_seq) + extra(M)
                for rows in sorted({1, M // 2 + 1, M}):
                    assert lib.b2t_clm_mixtral_tree_ws_bytes(p, q, rows, M, n_seq) == \
                        lib.b2t_clm_llama_tree_ws_bytes(p, rows, M, n_seq) + extra(rows)
                    assert lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, q, rows, M, n_seq) == \
                        lib.b2t_clm_llama_tree_cached_ws_bytes(p, rows, M, n_seq) + extra(rows)
            now = lib.b2t_clm_mixtral_ws_bytes(p, q, M, 1)
            assert now >= last > -1
            last = now
        sizes = [lib.b2t_clm_mixtral_tree_ws_bytes(p, q, r, 5000, 7) for r in range(1, 1200, 13)]
        assert sizes == sorted(sizes) and sizes[0] > 0
        sizes = [lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, q, r, 5000, 7) for r in range(1, 1200, 13)]
        assert sizes == sorted(sizes) and sizes[0] > 0
    desc, moe = _model(bias=False), _moe()
    p, q = C.byref(desc), C.byref(moe)
    assert lib.b2t_clm_mixtral_ws_bytes(p, q, 10, 1) > 0
    assert lib.b2t_clm_mixtral_ws_bytes(None, q, 10, 1) == 0 and lib.b2t_clm_mixtral_ws_bytes(p, None, 10, 1) == 0
    assert lib.b2t_clm_mixtral_tree_ws_bytes(None, q, 5, 10, 1) == 0 and lib.b2t_clm_mixtral_tree_ws_bytes(p, None, 5, 10, 1) == 0
    assert lib.b2t_clm_mixtral_tree_cached_ws_bytes(None, q, 5, 10, 1) == 0
    assert lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, None, 5, 10, 1) == 0
    for ne, k in ((0, 1), (65, 2), (8, 0), (8, 9), (4, 5), (-1, 1)):
        bad = C.byref(_moe(ne=ne, k=k))
        assert lib.b2t_clm_mixtral_ws_bytes(p, bad, 10, 1) == 0, (ne, k)
        assert lib.b2t_clm_mixtral_tree_ws_bytes(p, bad, 5, 10, 1) == 0 and lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, bad, 5, 10, 1) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert lib.b2t_clm_mixtral_ws_bytes(p, q, n_tok, n_seq) == 0, (n_tok, n_seq)
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert lib.b2t_clm_mixtral_tree_ws_bytes(p, q, nn, nt, ns) == 0, (nn, nt, ns)
        assert lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, q, nn, nt, ns) == 0, (nn, nt, ns)
    assert lib.b2t_clm_mixtral_ws_bytes(C.byref(_model(heads=0)), q, 10, 1) == 0


@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry):
    """Everything the Llama twin refuses, plus a null descriptor, router array or entry, expert counts outside the limits, a
    zero (or too small) stride and q / k / v biases, with fake pointers and no GPU; the call's own messages carry its name;
    the workspace wanted is this family's; on the cached call the cache is left as it was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_mixtral_" + entry
    fn = getattr(lib, who)
    tree, cached = "tree" in entry, "cached" in entry
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]
    nb = lambda **kw: _model(bias=False, **kw)     # d 256, ffn 512: strides 1024 and 256
    NOM = object()

    def refused(match, desc, moe=NOM, ids=ok_ids, off=ok_off, own=True, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None,
                cache=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        n = len(off) - 1 if n_seq is None else n_seq
        dp = C.byref(desc) if desc is not None else None
        q = _moe(desc.n_layers if desc is not None else 1) if moe is NOM else moe
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
    refused("multiple of n_kv_heads", nb(d=512, heads=8, kv=3), own=False)
    refused("multiples of 64", nb(d=256, heads=4, ffn=500), own=False)
    refused("bad dimensions", nb(kv=0), own=False)
    refused("rms_eps", nb(eps=-1.0), own=False)
    bad = nb()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad, own=False)
    # the descriptor's
    refused("null moe descriptor", nb(), moe=None)
    refused("null router_w_host", nb(), moe=_moe(routers=False))
    refused("null router weight in layer 0", nb(), moe=_moe(router=None))
    two = _moe(2)
    two.router_w_host[1] = None
    refused("null router weight in layer 1", nb(n_layers=2), moe=two)
    for ne in (0, -3, 65):
        refused(f"n_experts {ne} outside", nb(), moe=_moe(ne=ne))
    for ne, k in ((8, 0), (8, 9), (4, 5), (64, -1)):
        refused(f"top_k {k} outside", nb(), moe=_moe(ne=ne, k=k))
    refused("expert strides 0 / 256", nb(), moe=_moe(gus=0))
    refused("expert strides 1024 / 0", nb(), moe=_moe(dns=0))
    refused("expert strides 768 / 256", nb(), moe=_moe(gus=768))     # below round_up(2 * 512, 256)
    refused("layer 0 has q / k / v biases", _model(bias=True))
    # the list's
    refused("null argument", nb(), scores=None)
    refused("null argument", nb(), ws=None)
    refused("n_seq 0", nb(), n_seq=0)
    refused("empty", nb(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", nb(), off=[1, 2, 4])
    refused("outside", nb(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", nb(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4], cache=_cache(cap=3) if cached else None)
    # the workspace: this family's size functions; the Llama twin's size is too small
    desc, moe = nb(), _moe()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes, trunk 2
    p, q = C.byref(desc), C.byref(moe)
    if cached:
        need = lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, q, 4, 9, 3)
        assert need > lib.b2t_clm_llama_tree_cached_ws_bytes(p, 4, 9, 3)
        refused("workspace", desc, moe, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_mixtral_tree_cached_ws_bytes(p, q, 3, 9, 3)
        refused("workspace", desc, moe, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("null cache member", desc, moe, cache=_cache(kv=None))
        refused("above max_pos", nb(max_pos=64), cache=_cache(cap=65))
        rc = fn(p, q, None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1, FAKE, None, None, None, FAKE,
                1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_mixtral_score_tree_f16", N.last_error())
    elif tree:
        need = lib.b2t_clm_mixtral_tree_ws_bytes(p, q, 4, 9, 3)
        assert need > lib.b2t_clm_llama_tree_ws_bytes(p, 4, 9, 3)
        refused("workspace", desc, moe, ids=ids, off=off, ws_bytes=need - 1)
    else:
        need = lib.b2t_clm_mixtral_ws_bytes(p, q, 9, 3)
        assert need > lib.b2t_clm_llama_ws_bytes(p, 9, 3)
        refused("workspace", desc, moe, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_mixtral_unit_kernels_without_scratch():
    """The unit instantiates the grouped GEMM with EP_SWIGLU (5) and EP_F32 (10) on two tiles and in two element types, the
    route and gather kernels in two element types, the plan and combine kernels once, and nothing else -- no plain
    clm_gemm_kernel --: 14 kernels, ScratchSize 0, checked the way test_bf16_kernels_do_not_spill does."""
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_mixtral.hip" in G.HIP_SOURCES
    res = {k: v for k, v in W.resources(src="causal_lm_mixtral.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_grouped_kernel" in k]
    assert len(res) == 14 and len(gemm) == 8 and not [k for k in res if "clm_gemm_kernel" in k], sorted(res)
    assert sum("ELi5E" in k for k in gemm) == 4 and sum("ELi10E" in k for k in gemm) == 4
    assert sum("ILi256ELi256E" in k for k in gemm) == 4 and sum("ILi128ELi128E" in k for k in gemm) == 4
    assert sum(k.endswith("DF16_EEvNS_7ClmGemmE") for k in gemm) == 4 and sum(k.endswith("DF16bEEvNS_7ClmGemmE") for k in gemm) == 4
    for kern, n in (("clm_moe_route_kernel", 2), ("clm_moe_gather_kernel", 2), ("clm_moe_plan_kernel", 1), ("clm_moe_combine_kernel", 1)):
        assert sum(kern in k for k in res) == n, (kern, sorted(res))
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_mixtral_unit_uses_the_one_tile_rule():
    """Both grouped GEMMs go through causal_lm.hip's launch_gemm, and the host never reads the routing back: no copy, no
    synchronisation and no allocation in the unit or in clm_moe.h."""
    csrc = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")
    src = open(os.path.join(csrc, "causal_lm_mixtral.hip")).read()
    moe = open(os.path.join(csrc, "clm_moe.h")).read()
    code = src.split("#include")[1]
    assert "B2T_CLM_GEMM_256" not in code and "getenv" not in src + moe
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU, El, true>)") == 1
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_F32, El, true>)") == 1
    assert "clm_gemm_tiles" not in moe and "clm_gemm_kernel" not in src + moe
    for word in ("hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc", "hipEventSynchronize", "atomicAdd",
                 "atomic_", "__atomic", "__hip_atomic"):
        assert word not in src and word not in moe, word
