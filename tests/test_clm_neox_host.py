"""Host-side checks of the GPT-NeoX rescorer (csrc/causal_lm_neox.hip, llm_rescore.NeoxScorer; no GPU): the float64
restatement of the forward (ref_logp_neox, the reference of tests/test_gpu_clm_neox.py) against the HF fp32 models, the
separation of the erf GELU from the tanh form on a model built for it (`sep`), the loader's device layout against the state
dict under the inverse transform, its refusals, the refusals of the three entry points before any device work, the symbols,
sizes and struct layouts, the unit's kernel resources and the Python surface.

The tiny models (TINY) are random HF GPTNeoXForCausalLM instances built in memory, no download: two layers,
max_position_embeddings 128, F = 4 d, vocabularies that are no multiple of 64, with the weight recipe of
tests/test_clm_llama_host.py."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, hf_logp, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")

TINY = {
    "hd64_q": dict(hidden_size=128, num_attention_heads=2, rotary_pct=0.25, vocab_size=503, tie_word_embeddings=False),
    "hd64_h": dict(hidden_size=128, num_attention_heads=2, rotary_pct=0.5, vocab_size=611, tie_word_embeddings=False),
    "hd64_f": dict(hidden_size=128, num_attention_heads=2, rotary_pct=1.0, vocab_size=777, tie_word_embeddings=True,
                   hidden_act="gelu_fast"),
    "hd128_q": dict(hidden_size=256, num_attention_heads=2, rotary_pct=0.25, vocab_size=1003, tie_word_embeddings=False),
    # beyond the issue's four: head dim 128 with 64 rotary dims (the first 64-column slice rotates as a whole, the second passes
    # through) and with 128 (both slices rotate, the second with frequencies 32 .. 63, under the Llama permutation)
    "hd128_h": dict(hidden_size=256, num_attention_heads=2, rotary_pct=0.5, vocab_size=877, tie_word_embeddings=False),
    "hd128_f": dict(hidden_size=256, num_attention_heads=2, rotary_pct=1.0, vocab_size=901, tie_word_embeddings=False),
}
SEEDS = {"hd128_q": 0, "hd64_f": 1, "hd64_h": 2, "hd64_q": 3, "hd128_h": 4, "hd128_f": 5}   # of the weights, per model
ENTRY = ("b2t_clm_neox_score_f16", "b2t_clm_neox_score_tree_f16", "b2t_clm_neox_score_tree_cached_f16")
SIZES = ("b2t_clm_neox_ws_bytes", "b2t_clm_neox_tree_ws_bytes", "b2t_clm_neox_cache_kv_bytes", "b2t_clm_neox_tree_cached_ws_bytes")
# max |dlogp| of the unrounded float64 restatement against the HF fp32 CPU model over tiny_seqs (lengths 1 .. 100), measured
# here on the CPU; the test asserts at 10 x
HF_MEASURED = {"hd64_q": 1.4e-6, "hd64_h": 1.6e-6, "hd64_f": 4.0e-6, "hd128_q": 2.0e-6, "hd128_h": 1.6e-6, "hd128_f": 2.2e-6}
# the `sep` model (tiny_sep): fc1 scale, the weight of fc2's common column component, the weights' seed.  The scale was picked
# from the restatement alone: the mean of erf - tanh over Gaussian pre-activations of spread s is +5.7e-5 at s = 0.8 .. 1,
# crosses zero at s = 1.6 and is -2.6e-5 at s = 2, where the rounding of larger activations also costs more: planted tanh
# moves a log-prob by 0.9 e16 at scale 2, 0.5 e16 at 1.5, 3.9 e16 at 0.75 (a spread of 0.8)
SEP = dict(fc1_scale=0.75, common=3.0, seed=0)
CONTRACT_SEED = 3   # tests/test_gpu_clm_neox.py's sequences: the first seed from 3 upwards at which every model's e16 <= 1e-2 / 3
BOUND_CAP = 1e-2


def tiny_neox(name, n_layers=2, **over):
    """(HF fp32 CPU GPTNeoXForCausalLM in eval mode with fp16-representable random weights, its config as config.json's dict)."""
    import torch
    import transformers
    kw = dict(TINY[name], **over)
    cfg = transformers.GPTNeoXConfig(num_hidden_layers=n_layers, max_position_embeddings=128, intermediate_size=4 * kw["hidden_size"],
                                     attn_implementation="eager", bos_token_id=2, eos_token_id=2, **kw)
    torch.manual_seed(SEEDS[name])
    model = transformers.GPTNeoXForCausalLM(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(500 + SEEDS[name])
    with torch.no_grad():
        for k, p in model.named_parameters():
            if "layernorm" in k.replace("layer_norm", "layernorm") and k.endswith(".weight"):
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif k.endswith(".bias"):
                v = 0.3 * torch.randn(p.shape, generator=g)
            elif "embed_in" in k or "embed_out" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5      # logits with a spread of about 2
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            p.copy_(v.half().float())
    assert (model.get_output_embeddings().weight is model.gpt_neox.embed_in.weight) == kw["tie_word_embeddings"]
    return model, json.loads(cfg.to_json_string())


def neox_state(model):
    """The model's state dict under the names of the checkpoint files: the head is embed_out.weight (recent transformers
    call it lm_head in memory and rename it on saving)."""
    return {"embed_out.weight" if k == "lm_head.weight" else k: v.detach() for k, v in model.state_dict().items()}


def tiny_sep(fc1_scale=SEP["fc1_scale"], common=SEP["common"], seed=SEP["seed"]):
    """(state dict, config dict) of `sep`: one layer of hd64_q's shape in which the erf GELU and the tanh form can be told
    apart.  dense_h_to_4h (weight and bias) is scaled so that the pre-activations have a spread of about 0.8, where the mean of
    erf - tanh is largest (the comment at SEP); every column of dense_4h_to_h gets the same positive vector u added
    (|N(0, 1)| / sqrt(F) per entry, times `common`), so the even function erf - tanh adds up coherently across F along u while roundings do not; dense_4h_to_h's bias
    takes off what u contributes at the mean activation, so that this component does not drown the residual."""
    import torch
    model, cfg = tiny_neox("hd64_q", n_layers=1)
    st = neox_state(model)
    g = torch.Generator().manual_seed(900 + seed)
    p = "gpt_neox.layers.0.mlp."
    F, d = st[p + "dense_h_to_4h.weight"].shape
    for k in ("weight", "bias"):
        st[p + "dense_h_to_4h." + k] = (st[p + "dense_h_to_4h." + k] * fc1_scale).half().float()
    u = common * torch.randn(d, generator=g).abs() / F ** 0.5
    st[p + "dense_4h_to_h.weight"] = (st[p + "dense_4h_to_h.weight"] + u[:, None]).half().float()
    # E gelu(v) for v ~ N(0, s^2) is s^2 / sqrt(2 pi (1 + s^2)); s the spread of the pre-activations
    s = fc1_scale * (1 + 0.3 ** 2) ** 0.5
    mean_act = s * s / (2 * np.pi * (1 + s * s)) ** 0.5
    st[p + "dense_4h_to_h.bias"] = (st[p + "dense_4h_to_h.bias"] - F * mean_act * u).half().float()
    return st, cfg


def gelu_erf(v):
    import torch
    return 0.5 * v * (1 + torch.erf(v / 2 ** 0.5))


def gelu_tanh(v):
    import torch
    return 0.5 * v * (1 + torch.tanh((2 / np.pi) ** 0.5 * (v + 0.044715 * v ** 3)))


def ref_logp_neox(st, dims, seqs, rounded=True, act=None, theta=10000.0):
    """The forward restated in float64 from a state dict under HF's names (query_key_value interleaved per head as the
    checkpoint has it, nothing permuted); per sequence the log-probs (0 at the first token).  rounded=True rounds to fp16
    exactly where the contract of csrc/causal_lm_neox.hip says the kernels round, and nowhere else: both LayerNorm outputs; q
    after bias, the rotation of its first rotary_ndims dims and the factor head_dim^-0.5 (once); k after bias and rotation; v;
    the attention's probabilities per 32-key block relative to the running maximum (the kernel's P.V operand; the normaliser
    sums them unrounded) and its output; gelu(fc1).  cos / sin are then the fp32 table's entries (the angle p * inv_freq in
    double, inv_freq in fp32 as HF computes it).  Both LayerNorms read the layer's input; the residual receives the attention
    branch first, then the MLP branch.  rounded=False rounds nowhere.  `act` replaces the activation (default: dims["act"]: 0
    the erf GELU, 1 the tanh form)."""
    import torch
    F = torch.nn.functional
    W = lambda k: st[k if k.startswith("embed_out") else "gpt_neox." + k].double()
    r16 = (lambda t: t.half().double()) if rounded else (lambda t: t)
    if act is None:
        act = gelu_tanh if dims["act"] == 1 else gelu_erf
    d, H, nl, V, rn = dims["d_model"], dims["n_heads"], dims["n_layers"], dims["vocab"], dims["rotary_ndims"]
    hd = d // H
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["gpt_neox.embed_in.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    inv = 1.0 / (theta ** (torch.arange(0, rn, 2, dtype=torch.float) / rn))
    ang = pos.double()[:, None] * inv.to(dev).double()[None, :]
    cos, sin = torch.cos(ang), torch.sin(ang)
    if rounded:
        cos, sin = cos.float().double(), sin.float().double()
    cos, sin = torch.cat([cos, cos], -1)[:, None, :], torch.cat([sin, sin], -1)[:, None, :]   # [M, 1, rn]

    def rot(t):   # [M, H, hd]: HF's rotate_half on the first rn dims, the others pass through
        a, b = t[..., :rn], t[..., rn:]
        return torch.cat([a * cos + torch.cat([-a[..., rn // 2:], a[..., :rn // 2]], -1) * sin, b], -1)
    ln = lambda t, p: F.layer_norm(t, (d,), W(p + ".weight"), W(p + ".bias"), 1e-5)
    lin = lambda t, p: t @ W(p + ".weight").T + W(p + ".bias")
    x = W("embed_in.weight")[ids]
    M = x.shape[0]
    for l in range(nl):
        p = f"layers.{l}."
        h = r16(ln(x, p + "input_layernorm"))
        q, k, v = lin(h, p + "attention.query_key_value").view(M, H, 3, hd).unbind(2)      # rows [h][q | k | v][hd]
        q, k, v = r16(rot(q) * hd ** -0.5), r16(rot(k)), r16(v)
        o = torch.empty(M, d, dtype=torch.float64, device=dev)
        for j in range(B):
            a, b, n = off[j], off[j + 1], lens[j]
            qs, ks, vs = (t[a:b].transpose(0, 1) for t in (q, k, v))         # [H, n, hd]
            s = qs @ ks.transpose(1, 2)
            kk = torch.arange(n, device=dev)
            s = s.masked_fill((kk[None, :] > kk[:, None])[None], float("-inf"))
            nb = -(-n // 32)
            sb = F.pad(s, (0, nb * 32 - n), value=float("-inf")).view(H, n, nb, 32)
            mb = sb.amax(-1).cummax(-1).values
            pb = torch.exp(sb - mb[..., None])
            resc = torch.exp(mb - mb[..., -1:])[..., None]
            lsum = (pb * resc).sum((-1, -2))
            p16 = (r16(pb) * resc).view(H, n, nb * 32)[..., :n]
            o[a:b] = ((p16 @ vs) / lsum[..., None]).transpose(0, 1).reshape(n, d)
        h2 = r16(ln(x, p + "post_attention_layernorm"))                      # the layer's input again: the parallel residual
        mlp = lin(r16(act(lin(h2, p + "mlp.dense_h_to_4h"))), p + "mlp.dense_4h_to_h")
        x = (x + lin(r16(o), p + "attention.dense")) + mlp
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = r16(ln(x[src], "final_layer_norm"))
    E = st["embed_out.weight"] if "embed_out.weight" in st else st["gpt_neox.embed_in.weight"]
    chunk = max(64, (1 << 27) // h.shape[0])
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


# ---- the restatement against HF ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_fp64_restatement_matches_hf_fp32(name):
    """The unrounded float64 restatement against the HF fp32 CPU model (eager attention) at lengths 1 .. 100: what separates
    them is HF's fp32 arithmetic.  Asserted at 10 x the measured HF_MEASURED.  The restatement is the right function: the
    rotation of the first rotary_ndims dims only, the per-head interleaved query_key_value, the activation the config names,
    both LayerNorms on the layer's input."""
    import llm_rescore as R
    model, cfg = tiny_neox(name)
    dims = R.neox_dims(cfg)
    hd = cfg["hidden_size"] // cfg["num_attention_heads"]
    assert dims["rotary_ndims"] == int(hd * TINY[name]["rotary_pct"]) and dims["ffn_dim"] == 4 * dims["d_model"]
    assert dims["act"] == (1 if name == "hd64_f" else 0) and dims["vocab"] % 2 == 1
    seqs = tiny_seqs(cfg["vocab_size"], seed=4)
    assert [len(s) for s in seqs] == [1, 2, 17, 31, 32, 33, 64, 65, 100]
    ref = np.concatenate(ref_logp_neox(neox_state(model), dims, seqs, rounded=False))
    hf = np.concatenate(hf_logp(model, seqs))
    err = float(np.abs(ref - hf).max())
    print(f"CLM neox fp64 restatement vs HF fp32 {name}: max |dlogp| {err:.3e} (min logp {hf.min():.2f})")
    assert hf.min() < -8
    assert err <= 10 * HF_MEASURED[name], (name, err)
    # the other activation is a different function at this resolution
    other = gelu_erf if dims["act"] == 1 else gelu_tanh
    wrong = np.concatenate(ref_logp_neox(neox_state(model), dims, seqs, rounded=False, act=other))
    assert np.abs(wrong - hf).max() > 10 * HF_MEASURED[name]


def sep_figures():
    """(e16, the largest move of a log-prob when the tanh form is planted into the rounded restatement) of `sep` on the GPU
    file's sequences."""
    import llm_rescore as R
    st, cfg = tiny_sep()
    dims = R.neox_dims(cfg)
    seqs = contract_seqs(dims["vocab"], CONTRACT_SEED)
    ref = np.concatenate(ref_logp_neox(st, dims, seqs, True))
    exact = np.concatenate(ref_logp_neox(st, dims, seqs, False))
    planted = np.concatenate(ref_logp_neox(st, dims, seqs, True, act=gelu_tanh))
    return float(np.abs(ref - exact).max()), float(np.abs(planted - ref).max())


LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128)


def contract_seqs(V, seed):
    """The GPU contract test's list: LENS plus two candidates that share 20 tokens and a duplicate."""
    seqs = tiny_seqs(V, seed=seed, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]


def tiny_state(name):
    """(state dict under the checkpoint's names, config dict) of a tiny model or `sep`."""
    if name == "sep":
        return tiny_sep()
    model, cfg = tiny_neox(name)
    return neox_state(model), cfg


@pytest.mark.parametrize("name", list(TINY) + ["sep"])
def test_contract_seed_meets_the_precondition(name):
    """The GPU file's bound min(3 e16, 1e-2) presupposes 0 < e16 <= 1e-2 / 3 on its sequences; CONTRACT_SEED = 3, the first
    candidate, meets it for every model, by the restatement alone."""
    import llm_rescore as R
    st, cfg = tiny_state(name)
    dims = R.neox_dims(cfg)
    seqs = contract_seqs(dims["vocab"], CONTRACT_SEED)
    assert [len(s) for s in seqs] == list(LENS) + [23, 23, 127] and max(map(len, seqs)) == dims["max_pos"]
    ref = np.concatenate(ref_logp_neox(st, dims, seqs, True))
    exact = np.concatenate(ref_logp_neox(st, dims, seqs, False))
    e16 = float(np.abs(ref - exact).max())
    print(f"CLM neox e16 {name}: {e16:.3e}")
    assert CONTRACT_SEED == 3 and 0 < e16 <= BOUND_CAP / 3, (name, e16)


def test_the_bound_separates_erf_from_tanh_on_sep():
    """On ordinary tiny models min(3 e16, 1e-2) does not tell the erf GELU from the tanh form (the header of
    tests/test_gpu_clm_gpt2.py has the figures).  On `sep` it does: restatement against restatement, the tanh form planted
    into the rounded restatement moves a log-prob by more than the bound, while the bound's precondition holds."""
    e16, moved = sep_figures()
    print(f"CLM neox sep: e16 {e16:.3e}  bound {min(3 * e16, BOUND_CAP):.3e}  tanh planted moves a log-prob by {moved:.3e}")
    assert 0 < e16 <= BOUND_CAP / 3, e16
    assert moved > min(3 * e16, BOUND_CAP), (moved, e16)


# ---- the loader --------------------------------------------------------------------------------------------------------
def test_head_perm():
    import llm_rescore as R
    r = lambda a, b: list(range(a, b))
    assert R.neox_head_perm(64, 16).tolist() == r(0, 8) + r(16, 40) + r(8, 16) + r(40, 64)
    assert R.neox_head_perm(64, 32).tolist() == r(0, 16) + r(32, 48) + r(16, 32) + r(48, 64)
    assert R.neox_head_perm(64, 64).tolist() == r(0, 64)
    assert R.neox_head_perm(128, 32).tolist() == r(0, 16) + r(32, 48) + r(16, 32) + r(48, 64) + r(64, 128)
    assert R.neox_head_perm(128, 64).tolist() == r(0, 128)
    assert R.neox_head_perm(128, 128).tolist() == R.head_dim_perm(128).tolist()
    for hd in (64, 128):
        for rn in (hd // 4, hd // 2, hd):
            p = R.neox_head_perm(hd, rn)
            assert sorted(p.tolist()) == r(0, hd)
            inv = np.argsort(p)
            for f in range(rn // 2):   # pair f: 32 apart in slice f // 32, at lane f % 32 -- what EP_ROPE_PART relies on
                assert inv[f] == 64 * (f // 32) + f % 32 and inv[f + rn // 2] == inv[f] + 32
    for hd, rn in ((64, 8), (64, 48), (80, 20), (256, 64), (128, 16)):
        with pytest.raises(ValueError, match="not supported"):
            R.neox_head_perm(hd, rn)


@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict_under_the_inverse_transform(name, tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_neox(name)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_neox_arrays(str(tmp_path))
    d, H, V = cfg["hidden_size"], cfg["num_attention_heads"], cfg["vocab_size"]
    hd, tied = d // H, TINY[name]["tie_word_embeddings"]
    rn = int(hd * TINY[name]["rotary_pct"])
    assert dims == dict(n_layers=2, d_model=d, n_heads=H, ffn_dim=4 * d, vocab=V, max_pos=128, rotary_ndims=rn,
                        act=1 if name == "hd64_f" else 0, tied=tied)
    sd = neox_state(model)
    eq = lambda a, b: torch.equal(a, b.half())
    rup = lambda n: -(-n // 256) * 256
    hp =torch.from_numpy(R.neox_head_perm(hd, rn))

    def check(arr):
        assert arr["embed_in"].shape == (rup(V), d) and eq(arr["embed_in"][:V], sd["gpt_neox.embed_in.weight"])
        assert not arr["embed_in"][V:].any()
        if tied:
            assert arr["embed_out"] is arr["embed_in"]
        else:
            assert arr["embed_out"].shape == (rup(V), d) and eq(arr["embed_out"][:V], sd["embed_out.weight"])
            assert not arr["embed_out"][V:].any() and not torch.equal(arr["embed_out"], arr["embed_in"])
        assert eq(arr["final_ln_w"], sd["gpt_neox.final_layer_norm.weight"])
        assert eq(arr["final_ln_b"], sd["gpt_neox.final_layer_norm.bias"])
        # the table against HF's inv_freq: cos / sin of p * inv_freq evaluated in double, row stride rotary_ndims / 2
        inv = model.gpt_neox.rotary_emb.inv_freq.detach().float().numpy()
        assert inv.shape == (rn // 2,) and np.array_equal(R.neox_inv_freq(cfg), inv)
        ang = np.arange(128, dtype=np.float64)[:, None] * inv.astype(np.float64)[None, :]
        assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (128, rn // 2)
        assert np.array_equal(arr["rope_cos"].numpy(), np.cos(ang).astype(np.float32))
        assert np.array_equal(arr["rope_sin"].numpy(), np.sin(ang).astype(np.float32))
        for l in range(2):
            p, a = f"gpt_neox.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
            for ours, theirs in (("ln1", "input_layernorm"), ("ln2", "post_attention_layernorm")):
                assert eq(a(ours + "_w"), sd[p + theirs + ".weight"]) and eq(a(ours + "_b"), sd[p + theirs + ".bias"])
            for ours, theirs, n_in, n_out in (("out", "attention.dense", d, d), ("fc1", "mlp.dense_h_to_4h", d, 4 * d),
                                              ("fc2", "mlp.dense_4h_to_h", 4 * d, d)):
                w, b = a(ours + "_w"), a(ours + "_b")
                assert w.shape == (rup(n_out), n_in) and not w[n_out:].any(), ours
                assert eq(w[:n_out], sd[p + theirs + ".weight"]) and eq(b, sd[p + theirs + ".bias"]), ours
            # qkv: the permutation inverted inside every q and k head, then interleaved back per head
            w, b = a("qkv_w"), a("qkv_b")
            assert w.shape == (rup(3 * d), d) and not w[3 * d:].any() and b.shape == (3 * d,)
            for t, theirs in ((w[:3 * d], sd[p + "attention.query_key_value.weight"]), (b, sd[p + "attention.query_key_value.bias"])):
                t = t.view(3, H, hd, *t.shape[1:]).clone()
                back = torch.empty_like(t)
                back[:2, :, hp] = t[:2]            # stored row i = original row hp[i]
                back[2] = t[2]
                assert eq(back.transpose(0, 1).reshape(theirs.shape), theirs)
        assert all(t.is_contiguous() for t in arr.values())
        assert all(t.dtype == (torch.float32 if k.startswith("rope_") else torch.float16) for k, t in arr.items())
        assert len(arr) == 6 + 2 * 12

    check(arr)
    # keys without the 'gpt_neox.' prefix, and the buffers of old checkpoints
    bare = {k[len("gpt_neox."):] if k.startswith("gpt_neox.") else k: v for k, v in sd.items()}
    if tied:
        bare.pop("embed_out.weight", None)
    bare["layers.0.attention.bias"] = torch.ones(1, 1, 128, 128)
    bare["layers.1.attention.masked_bias"] = torch.tensor(-1e9)
    bare["layers.0.attention.rotary_emb.inv_freq"] = torch.ones(rn // 2)
    check(R.neox_device_layout(bare, dims, R.neox_inv_freq(cfg)))
    # either spelling of the config gives the same dims and table
    old = {k: v for k, v in cfg.items() if k != "rope_parameters"}
    old |= {"rotary_pct": TINY[name]["rotary_pct"], "rotary_emb_base": 10000, "rope_scaling": None}
    assert R.neox_dims(old) == dims and np.array_equal(R.neox_inv_freq(old), R.neox_inv_freq(cfg))
    assert cfg["rope_parameters"]["partial_rotary_factor"] == TINY[name]["rotary_pct"]


def test_loader_refusals():
    import llm_rescore as R
    model, cfg = tiny_neox("hd64_q", n_layers=1)
    dims = R.neox_dims(cfg)
    old = {k: v for k, v in cfg.items() if k != "rope_parameters"} | {"rotary_pct": 0.25, "rotary_emb_base": 10000}

    def refused(match, base=cfg, **kw):
        with pytest.raises(ValueError, match=match):
            R.neox_dims(base | kw)
    refused("use_parallel_residual=False", use_parallel_residual=False)
    refused("attention_bias=False", attention_bias=False)
    refused("layer_norm_eps", layer_norm_eps=1e-6)
    refused("rope_type 'linear'", rope_parameters=dict(cfg["rope_parameters"], rope_type="linear", factor=2.0))
    refused("rope_type 'dynamic'", base=old, rope_scaling={"type": "dynamic", "factor": 2.0})
    refused("hidden_act 'relu'", hidden_act="relu")
    refused("hidden_act 'silu'", hidden_act="silu")
    refused(r"head dim.*pythia-2.8b.*80.*pythia-1b.*256", hidden_size=2560, num_attention_heads=32, intermediate_size=10240)
    refused(r"head dim.*pythia-2.8b.*pythia-1b", hidden_size=2048, num_attention_heads=8, intermediate_size=8192)
    # GPT-NeoX-20B (hidden_size 6144, 64 heads: head dim 96, 24 rotary dims) is refused, and the message says so
    refused(r"head dim hidden_size 6144 / num_attention_heads 64.*gpt-neox-20b 96", hidden_size=6144, num_attention_heads=64,
            intermediate_size=24576, hidden_act="gelu_fast")
    refused("head dim", num_attention_heads=4)                       # head dim 32
    refused("head dim", num_attention_heads=3)                       # not a divisor
    refused("rotary dims", rope_parameters=dict(cfg["rope_parameters"], partial_rotary_factor=0.125))
    refused("rotary dims", base=old, rotary_pct=0.75)
    refused("multiples of 64", intermediate_size=500)
    # what is accepted: the four activation names, both spellings of the config
    for act, code in (("gelu", 0), ("gelu_new", 1), ("gelu_fast", 1), ("gelu_pytorch_tanh", 1)):
        assert R.neox_dims(cfg | {"hidden_act": act}) == dict(dims, act=code)
    assert R.neox_dims(old) == dims and R.neox_dims(old | {"rotary_pct": 1.0})["rotary_ndims"] == 64
    # the layout: a query_key_value of the wrong shape, a missing tensor
    st = neox_state(model)
    inv = R.neox_inv_freq(cfg)
    R.neox_device_layout(st, dims, inv)
    k = "gpt_neox.layers.0.attention.query_key_value.weight"
    with pytest.raises(ValueError, match=r"query_key_value.weight: shape \(128, 384\), expected \(384, 128\)"):
        R.neox_device_layout(dict(st, **{k: st[k].t()}), dims, inv)
    with pytest.raises(KeyError, match="final_layer_norm.bias"):
        R.neox_device_layout({k: v for k, v in st.items() if k != "gpt_neox.final_layer_norm.bias"}, dims, inv)
    with pytest.raises(KeyError, match="attention.dense.bias"):
        R.neox_device_layout({k: v for k, v in st.items() if k != "gpt_neox.layers.0.attention.dense.bias"}, dims, inv)
    # llama_dims and rope_inv_freq are what they were: the Llama family still refuses partial rotary and this model_type
    with pytest.raises(ValueError, match="model_type 'gpt_neox'"):
        R.llama_dims(cfg)
    with pytest.raises(ValueError, match="partial rotary"):
        R.rope_inv_freq(cfg)


# ---- the entry points --------------------------------------------------------------------------------------------------------
def _model(n_layers=1, d=256, heads=4, ffn=512, vocab=1000, max_pos=64, rot=None, act=0, table=FAKE):
    import b2t_native as N
    layers = (N.ClmLayer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmLayer._fields_:
            setattr(layers[i], f, FAKE)
    m = N.ClmNeoxDesc(n_layers, d, heads, ffn, vocab, max_pos, d // heads // 4 if rot is None else rot, act, FAKE, FAKE, FAKE, FAKE,
                      table, table, layers)
    m._keep = layers
    return m


def _flat(lib, desc, ids, off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None, tree=False):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    d = C.byref(desc) if desc is not None else None
    n = len(off) - 1 if n_seq is None else n_seq
    if tree:
        return lib.b2t_clm_neox_score_tree_f16(d, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
    return lib.b2t_clm_neox_score_f16(d, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)


def _model_refusals(refused):
    """The refusals of a descriptor, each under the entry point's own name."""
    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8))
    refused("head dim 80", _model(d=320, heads=4, rot=20))
    refused("head dim 256", _model(d=512, heads=2))
    refused("head dim 96", _model(d=384, heads=4, rot=24))      # GPT-NeoX-20B's
    refused("multiples of 64", _model(d=256, heads=4, ffn=500))
    refused("rotary_ndims 8 for head dim 64", _model(rot=8))
    refused("rotary_ndims 48 for head dim 64", _model(rot=48))
    refused("rotary_ndims 0", _model(rot=0))
    refused("rotary_ndims 16 for head dim 128", _model(d=256, heads=2, rot=16))
    refused("unknown act 2", _model(act=2))
    refused("unknown act -1", _model(act=-1))
    refused("null rotary table", _model(table=None))
    import b2t_native as N
    refused("null weight", N.ClmNeoxDesc(0, 256, 4, 512, 1000, 64, 16, 0, FAKE, None, FAKE, FAKE, FAKE, FAKE, None))
    bad = _model()
    bad._keep[0].fc2_b = None
    refused("null weight pointer in layer 0", bad)


@pytest.mark.parametrize("tree", [False, True])
def test_score_refusals_before_device_work(tree):
    import b2t_native as N
    lib = N.load()
    who = ENTRY[1] if tree else ENTRY[0]
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, **kw):
        rc = _flat(lib, desc, ids, off, tree=tree, **kw)
        err = N.last_error()
        assert rc != 0 and re.search(match, err), (match, rc, err)
        assert err.startswith(who + ":"), err      # the entry point's own name

    _model_refusals(refused)
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    for desc in (_model(), _model(rot=32, act=1), _model(d=256, heads=2, rot=128)):
        need = lib.b2t_clm_neox_tree_ws_bytes(C.byref(desc), 4, 4, 2) if tree else lib.b2t_clm_neox_ws_bytes(C.byref(desc), 4, 2)
        assert need > 0
        refused("workspace", desc, ws_bytes=need - 1)


def test_cached_score_refusals_before_device_work():
    """Every refusal of the tree call, plus the cache's own; a refused call leaves the cache untouched."""
    import b2t_native as N
    lib = N.load()
    who = ENTRY[2]
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def call(desc, cache, ids=ok_ids, off=ok_off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        return lib.b2t_clm_neox_score_tree_cached_f16(C.byref(desc) if desc is not None else None,
                                                      C.byref(cache) if cache is not None else None, update, ids.ctypes.data,
                                                      off.ctypes.data, len(off) - 1 if n_seq is None else n_seq, scores, None,
                                                      None, None, ws, ws_bytes, None)

    def refused(match, desc, cache=None, **kw):
        cache = _cache() if cache is None else cache
        n0, ids0 = cache.n, cache._keep.copy()
        rc = call(desc, cache, **kw)
        err = N.last_error()
        assert rc != 0 and re.search(match, err), (match, rc, err)
        assert err.startswith(who + ":"), err
        assert cache.n == n0 and (cache._keep == ids0).all()      # a refusal leaves the cache alone

    _model_refusals(refused)
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", _model(max_pos=3), cache=_cache(cap=3), ids=[2, 5, 7, 9], off=[0, 4])
    rc = call(_model(), None)
    assert rc != 0 and re.search(r"null cache \(callers without one use b2t_clm_neox_score_tree_f16\)", N.last_error())
    refused("null cache member", _model(), cache=_cache(kv=None))
    refused("null cache member", _model(), cache=_cache(logp=None))
    refused("cap 0", _model(), cache=_cache(ids=(), cap=0))
    refused("above max_pos", _model(max_pos=64), cache=_cache(cap=65))
    refused(r"n 9 outside", _model(), cache=_cache(cap=8, n=9))
    refused(r"n -1 outside", _model(), cache=_cache(cap=8, n=-1))
    refused("cached token 1 has id 1000", _model(vocab=1000), cache=_cache(ids=(2, 1000)))
    desc = _model()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]              # 9 tokens, 4 nodes, trunk 2
    need = lib.b2t_clm_neox_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
    refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
    need3 = lib.b2t_clm_neox_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)  # the cache (2, 5) spares one row
    assert 0 < need3 <= need
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)


def test_symbols_sizes_and_struct_layouts(tmp_path):
    """The header declares the seven functions and the library exports them with the OPT twins' signatures on the family's own
    model struct; the sizes are the OPT layout's (the same buffers); b2t_clm_neox_t is what the C compiler lays out, and
    b2t_clm_layer_t and b2t_clm_cache_t are what they were."""
    import b2t_native as N
    lib = N.load()
    declared = [s for s in N.header_symbols() if "neox" in s]
    assert sorted(declared) == sorted(ENTRY + SIZES)
    for name in ENTRY + SIZES:
        res, args = N._SIGNATURES[name]
        tres, targs = N._SIGNATURES[name.replace("neox_", "")]
        assert hasattr(lib, name) and res == tres and args[1:] == targs[1:] and args[0] == C.POINTER(N.ClmNeoxDesc), name
    with open(os.path.join(ROOT, "include", "b2t.h")) as f:
        hdr = f.read()
    sec = hdr[hdr.index("the same scoring for GPT-NeoX"):hdr.index("} b2t_clm_neox_t;")]
    for word in ("b2t_clm_tree_plan_host", "b2t_clm_cache_plan_host", "b2t_clm_cache_t", "attention branch first", "rotary_ndims"):
        assert word in sec, word
    assert not re.search(r"b2t_clm_neox_\w*plan", hdr)
    # the sizes: those of an OPT model of the same dimensions (same layout, same cache), 0 where the twins give 0
    neox, opt = _model(n_layers=3, max_pos=64), N.ClmDesc(3, 256, 4, 512, 1000, 64, FAKE, FAKE, FAKE, FAKE, None)
    a, b = C.byref(neox), C.byref(opt)
    assert lib.b2t_clm_neox_ws_bytes(a, 50, 3) == lib.b2t_clm_ws_bytes(b, 50, 3) > 0
    assert lib.b2t_clm_neox_tree_ws_bytes(a, 40, 50, 3) == lib.b2t_clm_tree_ws_bytes(b, 40, 50, 3) > 0
    assert lib.b2t_clm_neox_tree_cached_ws_bytes(a, 40, 50, 3) == lib.b2t_clm_tree_cached_ws_bytes(b, 40, 50, 3) > 0
    assert lib.b2t_clm_neox_cache_kv_bytes(a, 10) == lib.b2t_clm_cache_kv_bytes(b, 10) == 3 * 10 * 2 * 256 * 2
    assert lib.b2t_clm_neox_cache_kv_bytes(a, 65) == 0 and lib.b2t_clm_neox_cache_kv_bytes(a, 0) == 0
    assert lib.b2t_clm_neox_cache_kv_bytes(None, 10) == 0 and lib.b2t_clm_neox_ws_bytes(None, 5, 1) == 0
    assert lib.b2t_clm_neox_ws_bytes(a, 0, 1) == 0 and lib.b2t_clm_neox_ws_bytes(a, 3, 4) == 0
    assert lib.b2t_clm_neox_tree_ws_bytes(a, 51, 50, 3) == 0 and lib.b2t_clm_neox_tree_cached_ws_bytes(a, 0, 50, 3) == 0
    gcc = shutil.which("gcc")
    assert gcc is not None, "no C compiler"
    structs = {"b2t_clm_layer_t": (N.ClmLayer, 96), "b2t_clm_neox_t": (N.ClmNeoxDesc, 88), "b2t_clm_cache_t": (N.ClmCache, 32)}
    body = 'printf("act %d %d\\n", B2T_CLM_NEOX_ACT_GELU_ERF, B2T_CLM_NEOX_ACT_GELU_TANH);\n'
    for cname, (cls, _) in structs.items():
        body += f'printf("{cname} %zu\\n", sizeof({cname}));\n'
        body += "".join(f'printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));\n' for f in cls._fields_)
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){\n' + body + "return 0; }\n")
    exe = tmp_path / "lay"
    subprocess.run([gcc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if not line.strip():
            continue
        if line.startswith("act "):
            assert line.split()[1:] == [str(N.CLM_NEOX_ACT_GELU_ERF), str(N.CLM_NEOX_ACT_GELU_TANH)] == ["0", "1"]
            continue
        name, val = line.split()
        if "." in name:
            cname, field = name.split(".")
            assert getattr(structs[cname][0], field).offset == int(val), name
        else:
            assert C.sizeof(structs[name][0]) == int(val) == structs[name][1], name
        seen += 1
    assert seen == 3 + 12 + 15 + 5


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_neox_unit_has_four_gemm_kernels_without_scratch():
    """causal_lm_neox.hip instantiates its two epilogues (EP_ROPE_PART = 8, EP_GELU_ERF = 9) on both tiles and nothing else;
    none spills.  The tile rule is not restated there, and the tanh GELU is causal_lm_gpt2.hip's instantiation."""
    import wave_kernel_resources as W
    res = W.resources(src="causal_lm_neox.hip")
    assert len(res) == 4 and all("clm_gemm_kernel" in k for k in res), sorted(res)
    shapes = sorted(re.search(r"clm_gemm_kernelILi(\d+)ELi\d+ELi\d+ELi\d+ELi(\d+)E", k).groups() for k in res)
    assert shapes == [("128", "8"), ("128", "9"), ("256", "8"), ("256", "9")], sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize", -1) == 0 and 0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256, (k, v)
    src = open(os.path.join(CSRC, "causal_lm_neox.hip")).read()
    assert "getenv" not in src and "B2T_CLM_GEMM_256" not in src
    assert "launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE_PART>)" in src and "launch_gemm(g, s, &clm_gemm_tiles<EP_GELU_ERF>)" in src
    assert "clm_gemm_tiles<EP_GELU>" not in src and "__global__" not in src
    with open(os.path.join(CSRC, "clm_internal.h")) as f:
        assert "EP_ROPE_PART = 8, EP_GELU_ERF = 9" in f.read()
    import __graft_entry__ as G
    assert "causal_lm_neox.hip" in G.HIP_SOURCES


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(tmp_path):
    import inspect
    import torch
    import llm_rescore as R
    model, cfg = tiny_neox("hd64_q")
    model.save_pretrained(str(tmp_path))
    sc = R.build_scorer(str(tmp_path), device="cpu")
    assert type(sc) is R.NeoxScorer and isinstance(sc, R._Scorer) and sc.dtype is torch.float16
    assert inspect.signature(R.NeoxScorer.__init__) == inspect.signature(R.OptScorer.__init__)
    assert sc._ENTRY == "b2t_clm_neox_" and sc.dims == R.neox_dims(cfg)
    assert (sc.desc.max_pos, sc.desc.ffn_dim, sc.desc.rotary_ndims, sc.desc.act, sc.desc.n_heads) == (128, 512, 16, 0, 2)
    assert sc.desc.embed_out != sc.desc.embed_in and sc.w["rope_cos"].dtype is torch.float32
    assert sc.share_prefixes is False and sc.cache_len == 0 and sc.eval() is sc
    for dtype in ("auto", "float16", torch.float16, None):
        assert R.build_scorer(str(tmp_path), device="cpu", dtype=dtype).dtype is torch.float16
    # a tied model: the head is embed_in
    tied_dir = tmp_path / "tied"
    tmodel, tcfg = tiny_neox("hd64_f")
    tmodel.save_pretrained(str(tied_dir))
    tsc = R.build_scorer(str(tied_dir), device="cpu")
    assert tsc.desc.embed_out == tsc.desc.embed_in and (tsc.desc.act, tsc.desc.rotary_ndims) == (1, 64)
    # a config that says bfloat16: "auto" is still fp16
    with open(tmp_path / "config.json") as f:
        saved = json.load(f)
    with open(tmp_path / "config.json", "w") as f:
        json.dump(saved | {"torch_dtype": "bfloat16", "dtype": "bfloat16"}, f)
    assert R.build_scorer(str(tmp_path), device="cpu", dtype="auto").dtype is torch.float16
    # bfloat16 is refused with the family's own message, before any weight is read
    os.rename(tmp_path / "model.safetensors", tmp_path / "model.safetensors.away")
    with pytest.raises(ValueError, match="NeoxScorer: dtype 'bfloat16' is not supported for GPT-NeoX"):
        R.build_scorer(str(tmp_path), device="cpu", dtype="bfloat16")
    with pytest.raises(ValueError, match="is not supported"):
        R.build_scorer(str(tmp_path), device="cpu", dtype="float32")
    with pytest.raises(FileNotFoundError):
        R.build_scorer(str(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="NeoxScorer: dtype 'bfloat16'"):
        R.NeoxScorer(R.neox_dims(cfg), {}, "cpu", dtype=torch.bfloat16)
    # a refused config is refused by build_scorer, naming the cause; an unknown model_type names this family among the known
    with open(tmp_path / "config.json", "w") as f:
        json.dump(saved | {"use_parallel_residual": False}, f)
    with pytest.raises(ValueError, match="use_parallel_residual=False"):
        R.build_scorer(str(tmp_path), device="cpu")
    with open(tmp_path / "config.json", "w") as f:
        json.dump(saved | {"model_type": "bloom"}, f)
    with pytest.raises(ValueError, match=r"model_type 'bloom' is not supported \(opt, gpt2, gpt_neox, llama"):
        R.build_scorer(str(tmp_path), device="cpu")
