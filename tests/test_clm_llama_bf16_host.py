"""Host-side checks of the bfloat16 mode of the Llama-family rescorer (csrc/causal_lm_llama_bf16.hip, the `dtype` parameter of
llm_rescore; no GPU): the float64 restatement of the contract with the rounding format as a parameter (ref_logp_llama_fmt, the
reference of tests/test_gpu_clm_llama_bf16.py), what bf16 rounding does to the tiny models' log-probs, the range argument for
bf16 (a rescaling that fp16 cannot hold and bf16 does not notice), the loader in bf16, the dtype resolution and refusals, the
two new entry points' refusals before any device work, and the kernels' resources.

The tiny models are tests/test_clm_llama_host.py's, with every parameter rounded to bf16 first (bf16_model), so the weights are
exactly what the device holds."""
import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

from test_clm_llama_host import FAKE, TINY, _model, _ref_logp_llama, hf_inv_freq, ref_dims, state_of, tiny_model, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LENS = (1, 2, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)   # 692 tokens, 12 of them first tokens
E_BF16_MAX = 0.1   # the condition on the inputs: the GPU tests' bound 3 x e_bf16 is then never looser than 0.3


def bf16_model(name, n_layers=2, **over):
    """tiny_model with every parameter rounded to bf16 (to nearest even)."""
    import torch
    model, cfg = tiny_model(name, n_layers, **over)
    with torch.no_grad():
        for p in model.parameters():
            p.copy_(p.bfloat16().float())
    return model, cfg


def ref_logp_llama_fmt(st, dims, inv_freq, seqs, fmt=None):
    """_ref_logp_llama (tests/test_clm_llama_host.py) restated with the rounding format as a parameter: fmt = None rounds
    nowhere, "float16" and "bfloat16" round to that format (to nearest even) exactly where the contract of include/b2t.h says
    the kernels round, and nowhere else: the RMSNorm outputs; q after bias, rotation and the factor head_dim^-0.5; k after
    bias and rotation; v; the attention's probabilities per 32-key block relative to the running maximum (the normaliser sums
    them unrounded) and its output; silu(gate) * up.  With a format, cos / sin are the kernel's fp32 table entries.  float64
    tensors on the device the state dict is on; per sequence the log-probs (0 at the first token)."""
    import torch
    import llm_rescore as R
    F = torch.nn.functional
    W = lambda k: st[k].double()
    if fmt is None:
        rnd = lambda t: t
    else:
        rdt = R.clm_dtype(fmt)
        rnd = lambda t: t.to(rdt).double()
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
    lin = lambda t, p: t @ W(p + ".weight").T + (W(p + ".bias") if p + ".bias" in st else 0.0)
    groups, cur = [], []   # padded attention batches of whole sequences, each score tensor <= 2^27 fp64 elements
    for i in range(B):
        if cur and (len(cur) + 1) * Hq * max(lens[j] for j in cur + [i]) ** 2 > 1 << 27:
            groups.append(cur); cur = []
        cur.append(i)
    groups.append(cur)
    x = W("model.embed_tokens.weight")[ids]
    M = x.shape[0]
    for l in range(nl):
        p = f"model.layers.{l}."
        h = rnd(rms(x, p + "input_layernorm.weight"))
        q = rnd(rot(lin(h, p + "self_attn.q_proj").view(M, Hq, hd)) * hd ** -0.5)
        k = rnd(rot(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd)))
        v = rnd(lin(h, p + "self_attn.v_proj")).view(M, Hkv, hd)
        k, v = k.repeat_interleave(G, 1), v.repeat_interleave(G, 1)     # query head h reads kv head h // G
        o = torch.empty(M, d, dtype=torch.float64, device=dev)
        for g in groups:
            Lg = max(lens[j] for j in g)
            idx = torch.as_tensor(np.stack([off[j] + np.minimum(np.arange(Lg), lens[j] - 1) for j in g]), device=dev)
            L = torch.as_tensor([lens[j] for j in g], device=dev)
            sh = lambda t: t[idx].transpose(1, 2)                        # [b, Hq, Lg, hd]
            s = sh(q) @ sh(k).transpose(2, 3)
            kk = torch.arange(Lg, device=dev)
            mask = (kk[None, :] > kk[:, None])[None] | (kk[None, None, :] >= L[:, None, None])
            s = s.masked_fill(mask[:, None], float("-inf"))
            nb = -(-Lg // 32)
            sb = F.pad(s, (0, nb * 32 - Lg), value=float("-inf")).view(len(g), Hq, Lg, nb, 32)
            mb = sb.amax(-1).cummax(-1).values
            pb = torch.exp(sb - mb[..., None])
            resc = torch.exp(mb - mb[..., -1:])[..., None]
            lsum = (pb * resc).sum((-1, -2))
            pr = (rnd(pb) * resc).view(len(g), Hq, Lg, nb * 32)[..., :Lg]
            og = ((pr @ sh(v)) / lsum[..., None]).transpose(1, 2).reshape(len(g), Lg, d)
            for a, j in enumerate(g):
                o[off[j]:off[j + 1]] = og[a, :lens[j]]
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
    chunk = max(64, (1 << 27) // h.shape[0])
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def scaled_state(st, n_layers, k=14):
    """The same function in other units: up_proj * 2^k, down_proj * 2^-k (exact in bf16 and, at these weights, finite in fp16)."""
    out = dict(st)
    for l in range(n_layers):
        out[f"model.layers.{l}.mlp.up_proj.weight"] = st[f"model.layers.{l}.mlp.up_proj.weight"] * 2.0 ** k
        out[f"model.layers.{l}.mlp.down_proj.weight"] = st[f"model.layers.{l}.mlp.down_proj.weight"] * 2.0 ** -k
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_restatement_with_the_rounding_format_as_a_parameter(name):
    """Unrounded it is _ref_logp_llama(rounded=False) exactly and with fp16 rounding _ref_logp_llama(rounded=True) exactly;
    with bf16 rounding it is a different function, 0 < e_bf16 <= 0.1 away.  Measured on the CPU (max |logp| about 15):
    e_bf16 llama 5.8e-2, qwen2 3.8e-2, mistral 6.0e-2, llama3 7.1e-2 -- ten times the fp16 figures 6.0e-3, 4.2e-3, 5.9e-3,
    7.0e-3, as 3 bits of mantissa fewer make it."""
    model, cfg = bf16_model(name)
    st, rd, inv = state_of(model, TINY[name]["tie_word_embeddings"]), ref_dims(cfg), hf_inv_freq(model)
    seqs = tiny_seqs(rd["vocab"], seed=3, lens=LENS)
    cat = np.concatenate
    exact = cat(ref_logp_llama_fmt(st, rd, inv, seqs, None))
    assert np.array_equal(exact, cat(_ref_logp_llama(st, rd, inv, seqs, rounded=False)))
    r16 = cat(ref_logp_llama_fmt(st, rd, inv, seqs, "float16"))
    assert np.array_equal(r16, cat(_ref_logp_llama(st, rd, inv, seqs, rounded=True)))
    rb = cat(ref_logp_llama_fmt(st, rd, inv, seqs, "bfloat16"))
    e_bf16, e16 = float(np.abs(rb - exact).max()), float(np.abs(r16 - exact).max())
    print(f"CLM llama bf16 restatement {name}: e_bf16 {e_bf16:.3e}  e16 {e16:.3e}  (max |logp| {np.abs(exact).max():.2f})")
    assert len(exact) == 692 and np.isfinite(rb).all()
    assert 0 < e_bf16 <= E_BF16_MAX, (name, e_bf16)
    assert e16 < e_bf16


def test_range_invariance_of_the_bf16_contract():
    """up_proj * 2^14 and down_proj * 2^-14 is the same model.  The bf16 contract returns the unscaled model's log-probs
    exactly (8 exponent bits: silu(gate) * up * 2^14 rounds as silu(gate) * up does); the fp16 contract overflows at
    silu(gate) * up and returns non-finite log-probs for every token that has one (all but the 12 first tokens of 692)."""
    import torch
    model, cfg = bf16_model("llama")
    st, rd, inv = state_of(model, False), ref_dims(cfg), hf_inv_freq(model)
    sc = scaled_state(st, rd["n_layers"])
    for k in sc:   # every scaled weight is finite in both formats, and exact in bf16
        assert torch.isfinite(sc[k].half()).all() and torch.equal(sc[k].bfloat16().float(), sc[k])
    seqs = tiny_seqs(rd["vocab"], seed=3, lens=LENS)
    cat = np.concatenate
    plain = cat(ref_logp_llama_fmt(st, rd, inv, seqs, "bfloat16"))
    scaled = cat(ref_logp_llama_fmt(sc, rd, inv, seqs, "bfloat16"))
    print(f"CLM llama bf16 range: max |scaled - unscaled| {np.abs(scaled - plain).max():.3e}")
    assert np.isfinite(plain).all() and (scaled == plain).all()
    bad = cat(ref_logp_llama_fmt(sc, rd, inv, seqs, "float16"))
    finite = int(np.isfinite(bad).sum())
    print(f"CLM llama fp16 on the scaled model: {finite} of {len(bad)} entries finite")
    assert len(bad) == 692 and finite == 12 and not np.isfinite(bad).all()


# ---- the loader -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_loader_in_bf16_is_the_state_dict_permuted_bit_for_bit(name):
    import torch
    import llm_rescore as R
    model, cfg = bf16_model(name)
    small, large = float(torch.tensor(1e-6).bfloat16()), float(torch.tensor(1e5).bfloat16())
    # neither survives fp16: the one becomes a subnormal with another value, the other inf
    assert float(torch.tensor(small).half()) != small and torch.isinf(torch.tensor(large).half())
    with torch.no_grad():
        for l in range(cfg["num_hidden_layers"]):
            for n in ("self_attn.q_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj"):
                w = model.model.layers[l].get_submodule(n).weight
                w[1, 3], w[2, 5] = small, large
        model.model.embed_tokens.weight[5, 7], model.model.embed_tokens.weight[6, 8] = small, large
    tied = TINY[name]["tie_word_embeddings"]
    sd = {k: v.bfloat16() for k, v in state_of(model, tied).items()}     # a bf16 checkpoint
    for k, v in state_of(model, tied).items():
        assert torch.equal(sd[k].float(), v), k                          # holding exactly the model's values
    dims = R.llama_dims(cfg)
    inv = R.rope_inv_freq(cfg)
    arr = R.llama_device_layout(sd, dims, inv, dtype=torch.bfloat16)
    rd = ref_dims(cfg)
    d, Hq, Hkv, Fd, V = rd["d_model"], rd["n_heads"], rd["n_kv_heads"], rd["ffn_dim"], rd["vocab"]
    hd = d // Hq

    def eq(a, b):   # bit for bit
        return a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.shape == b.shape and \
            torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
    for k, t in arr.items():
        assert t.is_contiguous() and t.dtype == (torch.float32 if k.startswith("rope_") else torch.bfloat16), k
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert not arr["embed_tokens"][V:].any()
    assert float(arr["embed_tokens"][5, 7]) == small and float(arr["embed_tokens"][6, 8]) == large
    if tied:
        assert arr["lm_head"] is arr["embed_tokens"]
    else:
        assert eq(arr["lm_head"][:V], sd["lm_head.weight"]) and not arr["lm_head"][V:].any()
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    f16 = R.llama_device_layout(sd, dims, inv)
    assert torch.equal(arr["rope_cos"], f16["rope_cos"]) and torch.equal(arr["rope_sin"], f16["rope_sin"])   # the same table
    unperm = lambda h: torch.cat([h[:, 0:32], h[:, 64:96], h[:, 32:64], h[:, 96:128]], 1) if hd == 128 else h
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        assert eq(a("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(a("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any()
        un = unperm(w[:(Hq + Hkv) * hd].view(Hq + Hkv, hd, d)).reshape(-1, d)
        assert eq(un[:Hq * hd], sd[p + "self_attn.q_proj.weight"]) and eq(un[Hq * hd:], sd[p + "self_attn.k_proj.weight"])
        assert eq(w[(Hq + Hkv) * hd:qw], sd[p + "self_attn.v_proj.weight"])
        if name == "qwen2":
            b = a("qkv_b")
            hb = unperm(b[:(Hq + Hkv) * hd].view(Hq + Hkv, hd)).reshape(-1)
            assert b.shape == (qw,) and eq(hb[:Hq * hd], sd[p + "self_attn.q_proj.bias"])
            assert eq(hb[Hq * hd:], sd[p + "self_attn.k_proj.bias"]) and eq(b[(Hq + Hkv) * hd:], sd[p + "self_attn.v_proj.bias"])
        else:
            assert f"layers.{l}.qkv_b" not in arr
        assert eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and a("o_w").shape[0] % 256 == 0 and not a("o_w")[d:].any()
        gu = a("gate_up_w")
        assert gu.shape == (-(-2 * Fd // 256) * 256, d) and not gu[2 * Fd:].any()
        blocks = gu[:2 * Fd].view(Fd // 32, 2, 32, d)
        assert eq(blocks[:, 0].reshape(Fd, d), sd[p + "mlp.gate_proj.weight"])
        assert eq(blocks[:, 1].reshape(Fd, d), sd[p + "mlp.up_proj.weight"])
        assert eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"]) and a("down_w").shape == (-(-d // 256) * 256, Fd)
        planted = [float(x) for f in ("qkv_w", "o_w", "gate_up_w", "down_w") for x in a(f).float().flatten()
                   if float(x) in (small, large)]
        assert planted.count(small) >= 6 and planted.count(large) >= 6    # both survive in every matrix they were planted in
    # an fp32 checkpoint is rounded to nearest even, and the string spelling is the same call
    fp32 = {k: v.float() * (1 + 2.0 ** -10) for k, v in sd.items()}
    arr32 = R.llama_device_layout(fp32, dims, inv, dtype="bfloat16")
    assert torch.equal(arr32["final_norm_w"], fp32["model.norm.weight"].bfloat16())
    assert eq(arr32["embed_tokens"][:V], fp32["model.embed_tokens.weight"].bfloat16())


def test_default_loader_still_returns_fp16():
    import torch
    import llm_rescore as R
    model, cfg = tiny_model("qwen2")
    st = state_of(model, True)
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    base = R.llama_device_layout(st, dims, inv)
    assert torch.equal(base["embed_tokens"][:dims["vocab"]], st["model.embed_tokens.weight"].half())
    assert torch.equal(base["layers.0.down_w"][:dims["d_model"]], st["model.layers.0.mlp.down_proj.weight"].half())
    for spelling in (None, "float16", torch.float16):
        arr = R.llama_device_layout(st, dims, inv, dtype=spelling)
        assert sorted(arr) == sorted(base)
        for k in base:
            assert arr[k].dtype == (torch.float32 if k.startswith("rope_") else torch.float16), k
            assert torch.equal(arr[k], base[k]), k
    assert list(inspect.signature(R.llama_device_layout).parameters)[:3] == ["state", "dims", "inv_freq"]


# ---- dtype resolution and refusals --------------------------------------------------------------------------------------------
def test_dtype_resolution():
    import torch
    import llm_rescore as R
    f16, bf = torch.float16, torch.bfloat16
    assert R.clm_dtype(None) is f16 and R.clm_dtype("float16") is f16 and R.clm_dtype(f16) is f16
    assert R.clm_dtype("bfloat16") is bf and R.clm_dtype(bf) is bf
    for key in ("torch_dtype", "dtype"):     # the older and the newer spelling of config.json
        assert R.clm_dtype("auto", {key: "bfloat16"}) is bf
        for other in ("float16", "float32", None):
            assert R.clm_dtype("auto", {key: other}) is f16
        assert R.clm_dtype(None, {key: "bfloat16"}) is f16 and R.clm_dtype("float16", {key: "bfloat16"}) is f16
        assert R.clm_dtype("bfloat16", {key: "float16"}) is bf
    assert R.clm_dtype("auto", {}) is f16
    for bad in ("float32", "bf16", "half", "", 16, torch.float32):
        with pytest.raises(ValueError, match="dtype"):
            R.clm_dtype(bad)
    for fn in (R.OptScorer.__init__, R.LlamaScorer.__init__, R.build_scorer, R.build_opt):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "dtype" and params["dtype"].default is None, fn
    assert list(inspect.signature(R.LlamaScorer.__init__).parameters) == list(inspect.signature(R.OptScorer.__init__).parameters)


def test_dtype_refusals_come_before_the_weights_are_read(tmp_path):
    """Directories with a config.json and no weight files: a refused dtype is a ValueError, an accepted one gets as far as the
    missing weights."""
    import llm_rescore as R
    _, cfg = tiny_model("llama", n_layers=1)
    llama, opt = tmp_path / "llama", tmp_path / "opt"
    for d, c in ((llama, dict(cfg, torch_dtype="bfloat16")),
                 (opt, dict(model_type="opt", vocab_size=100, hidden_size=64, num_hidden_layers=2, ffn_dim=128,
                            num_attention_heads=1, max_position_embeddings=32, word_embed_proj_dim=64, do_layer_norm_before=True,
                            activation_function="relu", torch_dtype="bfloat16"))):
        os.makedirs(d)
        with open(d / "config.json", "w") as f:
            json.dump(c, f)
    for build in (R.build_scorer, R.build_opt):
        with pytest.raises(ValueError, match="dtype 'float32'"):
            build(str(llama), device="cpu", dtype="float32")
        with pytest.raises(ValueError, match="dtype 'float32'"):
            build(str(opt), device="cpu", dtype="float32")
        with pytest.raises(ValueError, match="bfloat16.*OPT"):
            build(str(opt), device="cpu", dtype="bfloat16")
        for dt in ("bfloat16", "auto"):
            with pytest.raises(ValueError, match="context cache behind bfloat16 is the follow-up"):
                build(str(llama), device="cuda", context_cache_tokens=64, dtype=dt)
        # accepted: these read on, to the weights that are not there
        for d, dt in ((llama, None), (llama, "float16"), (llama, "bfloat16"), (llama, "auto"), (opt, None), (opt, "float16"),
                      (opt, "auto")):
            with pytest.raises(FileNotFoundError):
                build(str(d), device="cpu", dtype=dt)


def test_scorers_on_the_cpu(tmp_path):
    """A bf16 scorer builds on device "cpu" as the fp16 one does (the descriptor only needs addressable weights); "auto"
    follows config.json in either spelling; the scorer exposes its dtype and checks its tensors against it."""
    import torch
    import llm_rescore as R
    model, cfg = bf16_model("qwen2")
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    with open(tmp_path / "config.json") as f:
        saved = json.load(f)
    assert "bfloat16" in (saved.get("torch_dtype"), saved.get("dtype"))
    sd = {k: v.float() for k, v in model.state_dict().items()}
    for key in ("torch_dtype", "dtype"):
        c = {k: v for k, v in saved.items() if k not in ("torch_dtype", "dtype")} | {key: "bfloat16"}
        with open(tmp_path / "config.json", "w") as f:
            json.dump(c, f)
        sc = R.build_scorer(str(tmp_path), device="cpu", dtype="auto")
        assert isinstance(sc, R.LlamaScorer) and sc.dtype is torch.bfloat16 and str(sc.device) == "cpu"
        assert sc.w["embed_tokens"].dtype == torch.bfloat16 and sc.w["rope_cos"].dtype == torch.float32
        assert torch.equal(sc.w["embed_tokens"][:777].float(), sd["model.embed_tokens.weight"])   # kept exactly
        assert sc.desc.lm_head == sc.desc.embed_tokens and sc.desc.layers_host[0].qkv_b
        assert sc.score([]).shape == (0,) and sc.eval() is sc
        for dt in (None, "float16"):
            s16 = R.build_scorer(str(tmp_path), device="cpu", dtype=dt)
            assert s16.dtype is torch.float16 and s16.w["embed_tokens"].dtype == torch.float16
        assert R.build_scorer(str(tmp_path), device="cpu", dtype="bfloat16", share_prefixes=True).share_prefixes is True
    with open(tmp_path / "config.json", "w") as f:
        json.dump({k: v for k, v in saved.items() if k not in ("torch_dtype", "dtype")} | {"torch_dtype": "float32"}, f)
    assert R.build_scorer(str(tmp_path), device="cpu", dtype="auto").dtype is torch.float16
    # the scorer checks its tensors against its own dtype, and refuses the cache in bf16 before anything else
    arr16, arrb = dict(s16.w), dict(sc.w)
    with pytest.raises(ValueError, match="expected torch.bfloat16"):
        R.LlamaScorer(sc.dims, arr16, "cpu", dtype="bfloat16")
    with pytest.raises(ValueError, match="expected torch.float16"):
        R.LlamaScorer(sc.dims, arrb, "cpu")
    with pytest.raises(ValueError, match="follow-up"):
        R.LlamaScorer(sc.dims, arrb, "cuda", False, 64, "bfloat16")
    with pytest.raises(ValueError, match="OPT"):
        R.OptScorer({}, {}, "cpu", dtype="bfloat16")
    with pytest.raises(ValueError, match="dtype 'int8'"):
        R.LlamaScorer(sc.dims, arrb, "cpu", dtype="int8")


# ---- the two entry points -------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1))
    for new, twin in (("b2t_clm_llama_score_bf16", "b2t_clm_llama_score_f16"),
                      ("b2t_clm_llama_score_tree_bf16", "b2t_clm_llama_score_tree_f16")):
        assert decl(new) == decl(twin)                       # the twin's argument list
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == list(g.argtypes)
    assert "b2t_clm_llama_ws_bytes_bf16" not in hdr and "bf16_ws_bytes" not in hdr    # no new size function
    assert not hasattr(N, "ClmLlamaDescBf16")                # the same descriptor


def _call(lib, tree, desc, ids, off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    n = len(off) - 1 if n_seq is None else n_seq
    dp = C.byref(desc) if desc is not None else None
    if tree:
        return lib.b2t_clm_llama_score_tree_bf16(dp, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
    return lib.b2t_clm_llama_score_bf16(dp, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)


@pytest.mark.parametrize("tree", [False, True])
def test_bf16_score_refusals_before_device_work(tree):
    """Everything the fp16 twin refuses (test_score_refusals_before_device_work of tests/test_clm_llama_host.py), with fake
    pointers and no GPU; the messages of the call's own checks carry the bf16 entry point's name."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_llama_score_tree_bf16" if tree else "b2t_clm_llama_score_bf16"
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, own=False, **kw):
        rc = _call(lib, tree, desc, ids, off, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        if own:
            assert N.last_error().startswith(who + ":"), N.last_error()

    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8, kv=8))
    refused("head dim 80", _model(d=320, heads=4, kv=4))
    refused("multiple of n_heads", _model(d=256, heads=3, kv=3))
    refused("multiple of n_kv_heads", _model(d=512, heads=8, kv=3))
    refused("multiples of 64", _model(d=256, heads=4, ffn=500))
    refused("bad dimensions", _model(kv=0))
    refused("bad dimensions", _model(max_pos=0))
    refused("rms_eps", _model(eps=-1.0))
    refused("rms_eps", _model(eps=float("nan")))
    d0 = N.ClmLlamaDesc(0, 256, 4, 2, 512, 1000, 64, 1e-5, FAKE, FAKE, FAKE, FAKE, 0, None)
    refused("null weight", d0)
    bad = _model()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad)
    refused("null argument", _model(), scores=None, own=True)
    refused("null argument", _model(), ws=None, own=True)
    refused("n_seq 0", _model(), n_seq=0, own=True)
    refused("empty", _model(), off=[0, 1, 1, 4], own=True)
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4], own=True)
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9], own=True)
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9], own=True)
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4], own=True)
    for desc in (_model(), _model(bias=False)):     # a null qkv_b is a model without q / k / v biases, not an error
        need = (lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 4, 2) if tree else lib.b2t_clm_llama_ws_bytes(C.byref(desc), 4, 2))
        assert need > 0
        refused("workspace", desc, ws_bytes=need - 1, own=True)
    if tree:
        desc = _model()
        ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes
        need = lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1, own=True)


# ---- the kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_bf16_kernels_do_not_spill():
    # at the time of writing: the 256-tile GEMMs 222 VGPRs, the 128-tile ones 85-88 (+ 64 AGPRs), flat attention 175 / 224
    # (head dim 64 / 128), tree attention 113 / 202, embed and RMSNorm 16; scratch 0 everywhere
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm_llama_bf16.hip").items() if "clm_" in k}
    count = lambda s: len([k for k in res if s in k])
    # EP_ROPE, EP_SWIGLU, EP_RESID and EP_HEAD on both tiles; flat and tree attention for head dims 64 and 128
    assert count("clm_gemm_kernel") == 8 and count("clm_attn_kernel") == 2 and count("clm_attn_tree_kernel") == 2, sorted(res)
    assert count("clm_llama_embed_kernel") == 1 and count("clm_llama_rmsnorm_kernel") == 1 and len(res) == 14, sorted(res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_bf16_unit_uses_the_one_tile_rule():
    """As test_one_tile_rule_for_both_families: every bf16 GEMM goes through causal_lm.hip's launch_gemm."""
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_llama_bf16.hip")).read()
    assert "getenv" not in src and "B2T_CLM_GEMM_256" not in src
    for ep in ("EP_ROPE", "EP_SWIGLU", "EP_RESID", "EP_HEAD"):
        assert src.count(f"launch_gemm(g, s, &clm_gemm_tiles<{ep}, __bf16>)") == 1, ep
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    assert "causal_lm_llama_bf16.hip" in G.HIP_SOURCES
