"""Host-side checks of the Llama-family rescorer (csrc/causal_lm_llama.hip, llm_rescore.LlamaScorer; no GPU): the loader's
device layout against the state dict, inv_freq against HF's, the refusals, the float64 restatement of the forward
(_ref_logp_llama, the reference of tests/test_gpu_clm_llama.py) against the HF fp32 models, the ABI structs against the C
compiler's layout, the workspace sizes, the refusals of the two score calls before any device work, the kernels' resources
and the Python surface.

The tiny models (TINY) are random HF models built in memory, no download: between them grouped-query ratios 1, 2, 4 and 8,
head dims 64 and 128, q / k / v biases, a tied and an untied head, "default" and "llama3" rotary scaling, a sliding window."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FAKE = 0x10000   # a non-null "device" pointer that is never dereferenced

# 2 layers, d <= 512, F a multiple of 64 that is no power of two, vocab no multiple of 64
TINY = {
    "llama": dict(cls="LlamaConfig", hidden_size=256, num_attention_heads=4, num_key_value_heads=2, intermediate_size=320,
                  vocab_size=1003, max_position_embeddings=256, tie_word_embeddings=False, rms_norm_eps=1e-5),
    "qwen2": dict(cls="Qwen2Config", hidden_size=512, num_attention_heads=4, num_key_value_heads=1, intermediate_size=448,
                  vocab_size=777, max_position_embeddings=256, tie_word_embeddings=True, rms_norm_eps=1e-6),
    "mistral": dict(cls="MistralConfig", hidden_size=512, num_attention_heads=4, num_key_value_heads=4, intermediate_size=576,
                    vocab_size=1003, max_position_embeddings=4096, sliding_window=192, tie_word_embeddings=False,
                    rms_norm_eps=1e-5),
    "llama3": dict(cls="LlamaConfig", hidden_size=512, num_attention_heads=8, num_key_value_heads=1, intermediate_size=192,
                   vocab_size=515, max_position_embeddings=512, tie_word_embeddings=True, rms_norm_eps=1e-5,
                   rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                     original_max_position_embeddings=64), rope_theta=500000.0),
}


def tiny_model(name, n_layers=2, **over):
    """(HF fp32 CPU model in eval mode with fp16-representable random weights, its config as the dict of config.json);
    `over` replaces entries of TINY[name]."""
    import torch
    import transformers
    kw = dict(TINY[name], **over)
    cls = getattr(transformers, kw.pop("cls"))
    if "rope_theta" in kw and "rope_scaling" in kw:   # one dict in either spelling of the library's versions
        kw["rope_scaling"] = dict(kw["rope_scaling"], rope_theta=kw.pop("rope_theta"))
    cfg = cls(num_hidden_layers=n_layers, attn_implementation="eager", **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = getattr(transformers, cls.__name__.replace("Config", "ForCausalLM"))(cfg).float().eval()
    d = cfg.hidden_size
    g = torch.Generator().manual_seed(100 + sorted(TINY).index(name))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.endswith("norm.weight") or "layernorm" in k:
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif k.endswith(".bias"):
                v = 0.3 * torch.randn(p.shape, generator=g)
            elif "embed_tokens" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5      # logits with a spread of about 2
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[1] ** 0.5
            p.copy_(v.half().float())
    return model, json.loads(cfg.to_json_string())


def hf_inv_freq(model):
    return model.model.rotary_emb.inv_freq.detach().float().numpy().copy()


def ref_dims(cfg):
    Hq = cfg["num_attention_heads"]
    return dict(n_layers=cfg["num_hidden_layers"], d_model=cfg["hidden_size"], n_heads=Hq,
                n_kv_heads=cfg.get("num_key_value_heads") or Hq, ffn_dim=cfg["intermediate_size"], vocab=cfg["vocab_size"],
                rms_eps=cfg["rms_norm_eps"])


def _ref_logp_llama(st, dims, inv_freq, seqs, rounded=True):
    """The forward restated in float64 from a state dict under HF's names (nothing permuted or interleaved); per sequence
    the log-probs (0 at the first token).  rounded=True rounds to fp16 exactly where the contract of include/b2t.h says the
    kernels round, and nowhere else: the RMSNorm outputs; q after bias, rotation and the factor head_dim^-0.5; k after bias and
    rotation; v; the attention's probabilities per 32-key block relative to the running maximum (the kernel's P.V operand; the
    normaliser sums them unrounded) and its output; silu(gate) * up.  cos / sin are the kernel's fp32 table entries (evaluated
    in double).  rounded=False rounds nowhere: the exact forward of the fp16-valued weights.  float64 tensors on the device the
    state dict is on (the CPU here, the GPU in tests/test_gpu_clm_llama.py, where the full widths would take minutes)."""
    import torch
    F = torch.nn.functional
    W = lambda k: st[k].double()
    r16 = (lambda t: t.half().double()) if rounded else (lambda t: t)
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
    if rounded:
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
        h = r16(rms(x, p + "input_layernorm.weight"))
        q = r16(rot(lin(h, p + "self_attn.q_proj").view(M, Hq, hd)) * hd ** -0.5)
        k = r16(rot(lin(h, p + "self_attn.k_proj").view(M, Hkv, hd)))
        v = r16(lin(h, p + "self_attn.v_proj")).view(M, Hkv, hd)
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
            p16 = (r16(pb) * resc).view(len(g), Hq, Lg, nb * 32)[..., :Lg]
            og = ((p16 @ sh(v)) / lsum[..., None]).transpose(1, 2).reshape(len(g), Lg, d)
            for a, j in enumerate(g):
                o[off[j]:off[j + 1]] = og[a, :lens[j]]
        x = x + lin(r16(o), p + "self_attn.o_proj")
        h = r16(rms(x, p + "post_attention_layernorm.weight"))
        gate = lin(h, p + "mlp.gate_proj")
        x = x + lin(r16(gate * torch.sigmoid(gate) * lin(h, p + "mlp.up_proj")), p + "mlp.down_proj")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = r16(rms(x[src], "model.norm.weight"))
    E = st["lm_head.weight"] if "lm_head.weight" in st else st["model.embed_tokens.weight"]
    chunk = max(64, (1 << 27) // h.shape[0])
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def hf_logp(model, seqs):
    """Per-token log-probs of the HF fp32 model, one sequence at a time (no padding)."""
    import torch
    out = []
    with torch.no_grad():
        for s in seqs:
            ids = torch.as_tensor(np.asarray(s, np.int64))[None]
            lp = torch.log_softmax(model(input_ids=ids).logits[0].double(), -1)
            o = np.zeros(len(s))
            o[1:] = lp[torch.arange(len(s) - 1), ids[0, 1:]].numpy()
            out.append(o)
    return out


def tiny_seqs(V, seed=0, lens=(1, 2, 17, 31, 32, 33, 64, 65, 100)):
    rng = np.random.default_rng(seed)
    return [[2] + list(rng.integers(0, V, n - 1)) for n in lens]


def state_of(model, tied):
    st = {k: v.detach() for k, v in model.state_dict().items()}
    if tied:
        st.pop("lm_head.weight", None)
    return st


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict_permuted(name, tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_model(name)
    model.save_pretrained(str(tmp_path))
    dims, arr = R.load_llama_arrays(str(tmp_path))
    sd = model.state_dict()
    rd = ref_dims(cfg)
    for k in ("n_layers", "d_model", "n_heads", "n_kv_heads", "ffn_dim", "vocab"):
        assert dims[k] == rd[k], k
    assert abs(dims["rms_eps"] - rd["rms_eps"]) < 1e-12
    d, Hq, Hkv, Fd, V = rd["d_model"], rd["n_heads"], rd["n_kv_heads"], rd["ffn_dim"], rd["vocab"]
    hd = d // Hq
    # max_pos: the model's, lowered to the sliding window in use
    assert dims["max_pos"] == {"llama": 256, "qwen2": 256, "mistral": 192, "llama3": 512}[name]
    eq = lambda a, b: torch.equal(a, b.half())
    Vp = -(-V // 256) * 256
    assert arr["embed_tokens"].shape == (Vp, d) and eq(arr["embed_tokens"][:V], sd["model.embed_tokens.weight"])
    assert not arr["embed_tokens"][V:].any()
    if TINY[name]["tie_word_embeddings"]:
        assert arr["lm_head"] is arr["embed_tokens"]
    else:
        assert arr["lm_head"].shape == (Vp, d) and eq(arr["lm_head"][:V], sd["lm_head.weight"]) and not arr["lm_head"][V:].any()
        assert not torch.equal(arr["lm_head"], arr["embed_tokens"])
    assert eq(arr["final_norm_w"], sd["model.norm.weight"])
    # the rotary table: cos / sin of p * inv_freq evaluated in double
    inv = hf_inv_freq(model)
    ang = np.arange(dims["max_pos"], dtype=np.float64)[:, None] * inv.astype(np.float64)[None]
    assert arr["rope_cos"].dtype == torch.float32 and arr["rope_cos"].shape == (dims["max_pos"], hd // 2)
    assert np.array_equal(arr["rope_cos"].numpy(), np.cos(ang).astype(np.float32))
    assert np.array_equal(arr["rope_sin"].numpy(), np.sin(ang).astype(np.float32))
    for l in range(dims["n_layers"]):
        p, a = f"model.layers.{l}.", lambda f: arr[f"layers.{l}.{f}"]
        assert eq(a("norm1_w"), sd[p + "input_layernorm.weight"]) and eq(a("norm2_w"), sd[p + "post_attention_layernorm.weight"])
        qw = (Hq + 2 * Hkv) * hd
        w = a("qkv_w")
        assert w.shape == (-(-qw // 256) * 256, d) and not w[qw:].any()
        # undo the stated permutation: inside every q and k head of 128 the stored order is [0..31, 64..95, 32..63, 96..127]
        heads = w[:(Hq + Hkv) * hd].view(Hq + Hkv, hd, d)
        if hd == 128:
            heads = torch.cat([heads[:, 0:32], heads[:, 64:96], heads[:, 32:64], heads[:, 96:128]], 1)   # the order is an involution
        un = heads.reshape(-1, d)
        assert eq(un[:Hq * hd], sd[p + "self_attn.q_proj.weight"]) and eq(un[Hq * hd:], sd[p + "self_attn.k_proj.weight"])
        assert eq(w[(Hq + Hkv) * hd:qw], sd[p + "self_attn.v_proj.weight"])
        if name == "qwen2":
            b = a("qkv_b")
            hb = b[:(Hq + Hkv) * hd].view(Hq + Hkv, hd)
            hb = torch.cat([hb[:, 0:32], hb[:, 64:96], hb[:, 32:64], hb[:, 96:128]], 1).reshape(-1)
            assert b.shape == (qw,) and eq(hb[:Hq * hd], sd[p + "self_attn.q_proj.bias"])
            assert eq(hb[Hq * hd:], sd[p + "self_attn.k_proj.bias"]) and eq(b[(Hq + Hkv) * hd:], sd[p + "self_attn.v_proj.bias"])
        else:
            assert f"layers.{l}.qkv_b" not in arr
        assert eq(a("o_w")[:d], sd[p + "self_attn.o_proj.weight"]) and a("o_w").shape[0] % 256 == 0 and not a("o_w")[d:].any()
        gu = a("gate_up_w")
        assert gu.shape == (-(-2 * Fd // 256) * 256, d) and not gu[2 * Fd:].any()
        blocks = gu[:2 * Fd].view(Fd // 32, 2, 32, d)   # row 64b + i = gate[32b + i], row 64b + 32 + i = up[32b + i]
        assert eq(blocks[:, 0].reshape(Fd, d), sd[p + "mlp.gate_proj.weight"])
        assert eq(blocks[:, 1].reshape(Fd, d), sd[p + "mlp.up_proj.weight"])
        assert eq(a("down_w")[:d], sd[p + "mlp.down_proj.weight"]) and a("down_w").shape == (-(-d // 256) * 256, Fd)
    for t in arr.values():
        assert t.is_contiguous()


def test_head_dim_permutation_puts_rotary_pairs_32_apart():
    import llm_rescore as R
    for hd in (64, 128):
        p = R.head_dim_perm(hd)
        assert sorted(p) == list(range(hd))
        for blk in range(hd // 64):
            for i in range(32):
                a, b = p[64 * blk + i], p[64 * blk + 32 + i]
                assert b - a == hd // 2 and a == 32 * blk + i     # the frequency index the EP_ROPE epilogue uses
    g = R.gate_up_row_perm(128)
    assert g[:32].tolist() == list(range(32)) and g[32:64].tolist() == list(range(128, 160)) and g[64] == 32 and g[96] == 160


@pytest.mark.parametrize("name", list(TINY))
def test_inv_freq_equals_hf(name):
    import llm_rescore as R
    model, cfg = tiny_model(name, n_layers=1)
    ours = R.rope_inv_freq(cfg)
    assert ours.dtype == np.float32 and np.array_equal(ours, hf_inv_freq(model)), name
    if name == "llama3":   # the scaling did something: high frequencies kept, the lowest divided by the factor
        plain = R.rope_inv_freq({k: v for k, v in cfg.items() if k not in ("rope_parameters", "rope_scaling")} |
                                {"rope_theta": 500000.0})
        assert np.array_equal(ours[:3], plain[:3]) and np.allclose(ours[-1], plain[-1] / 8.0) and not np.array_equal(ours, plain)
    # the older spelling of the same config
    rp = cfg.get("rope_parameters")
    if rp:
        old = {k: v for k, v in cfg.items() if k != "rope_parameters"}
        old["rope_theta"] = rp["rope_theta"]
        if rp["rope_type"] != "default":
            old["rope_scaling"] = {("type" if k == "rope_type" else k): v for k, v in rp.items() if k != "rope_theta"}
        assert np.array_equal(R.rope_inv_freq(old), ours)


def test_loader_refusals(tmp_path):
    import llm_rescore as R
    _, cfg = tiny_model("llama", n_layers=1)
    base = {k: v for k, v in cfg.items() if k != "rope_parameters"} | {"rope_theta": 10000.0}
    R.llama_dims(base)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            R.llama_dims(base | kw)
    for kind in ("linear", "dynamic", "yarn", "longrope"):
        refused("rope_type", rope_scaling={"rope_type": kind, "factor": 2.0})
        refused("rope_type", rope_scaling={"type": kind, "factor": 2.0})
    refused("head dim", num_attention_heads=8)                      # head dim 32
    refused("head dim", hidden_size=320, num_attention_heads=4)     # head dim 80
    refused("head dim", head_dim=128)                               # Hq * hd != d_model
    refused("multiple of num_key_value_heads", num_key_value_heads=3)
    refused("multiples of 64", intermediate_size=300)
    refused("multiples of 64", hidden_size=192, num_attention_heads=3, num_key_value_heads=3, intermediate_size=200)
    refused("activation", hidden_act="gelu")
    refused("mlp_bias", mlp_bias=True)
    refused("model_type", model_type="gemma")
    with pytest.raises(ValueError, match="max_positions"):
        R.llama_dims(base, max_positions=0)
    # the caps on max_pos
    assert R.llama_dims(base)["max_pos"] == 256 and R.llama_dims(base, max_positions=100)["max_pos"] == 100
    assert R.llama_dims(base | {"max_position_embeddings": 131072})["max_pos"] == R.LLAMA_MAX_POSITIONS
    assert R.llama_dims(base | {"model_type": "mistral", "sliding_window": 64})["max_pos"] == 64
    assert R.llama_dims(base | {"model_type": "mistral", "sliding_window": None})["max_pos"] == 256
    q = base | {"model_type": "qwen2", "sliding_window": 64}
    assert R.llama_dims(q | {"use_sliding_window": False})["max_pos"] == 256
    assert R.llama_dims(q | {"use_sliding_window": True, "layer_types": ["full_attention", "sliding_attention"]})["max_pos"] == 64
    assert R.llama_dims(q | {"use_sliding_window": True, "layer_types": ["full_attention"]})["max_pos"] == 256
    # build_scorer dispatches on model_type and refuses the rest as it refuses an unsupported OPT
    with open(tmp_path / "config.json", "w") as f:
        json.dump(base | {"model_type": "gemma"}, f)
    with pytest.raises(ValueError, match="model_type 'gemma'"):
        R.build_scorer(str(tmp_path), device="cpu")
    # an o_proj bias (attention_bias=True checkpoints) is refused by the layout
    model, cfg2 = tiny_model("llama", n_layers=1)
    st = state_of(model, False)
    st["model.layers.0.self_attn.o_proj.bias"] = st["model.norm.weight"]
    with pytest.raises(ValueError, match="biases other than"):
        R.llama_device_layout(st, R.llama_dims(cfg2), R.rope_inv_freq(cfg2))


# ---- the reference restatement against HF fp32 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_unrounded_restatement_equals_hf_fp32(name):
    # measured here (CPU, fp32 HF eager attention against float64; log-probs down to -13.6 .. -16.2): max |dlogp| llama
    # 7.33e-6, qwen2 5.87e-6, mistral 9.43e-6, llama3 6.70e-6; HF_BOUND is 10 x that
    model, cfg = tiny_model(name)
    seqs = tiny_seqs(cfg["vocab_size"], seed=1)
    ref = _ref_logp_llama(state_of(model, TINY[name]["tie_word_embeddings"]), ref_dims(cfg), hf_inv_freq(model), seqs,
                          rounded=False)
    hf = hf_logp(model, seqs)
    err = max(np.abs(a - b).max() for a, b in zip(ref, hf))
    mx = max(np.abs(b).max() for b in hf)
    print(f"CLM llama restatement vs HF fp32 {name}: max |dlogp| {err:.3e} (max |logp| {mx:.2f})")
    assert mx > 5 and err <= HF_BOUND[name], (name, err)


HF_BOUND = {"llama": 7.4e-5, "qwen2": 5.9e-5, "mistral": 9.5e-5, "llama3": 6.7e-5}   # 10 x the measured, never above 1e-4


def test_rounding_changes_the_restatement():
    """rounded=True is a different function (the GPU tests' bound is 3 x this difference), and still close to HF."""
    model, cfg = tiny_model("llama")
    seqs = tiny_seqs(cfg["vocab_size"], seed=2)
    st, rd, inv = state_of(model, False), ref_dims(cfg), hf_inv_freq(model)
    a = np.concatenate(_ref_logp_llama(st, rd, inv, seqs, rounded=True))
    b = np.concatenate(_ref_logp_llama(st, rd, inv, seqs, rounded=False))
    e16 = np.abs(a - b).max()
    print(f"CLM llama e16 (tiny llama): {e16:.3e}")
    assert 1e-5 < e16 < 1e-2


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs a C compiler")
def test_struct_layouts_match_the_header(tmp_path):
    import b2t_native as N
    src = tmp_path / "lay.c"
    fl = [n for n, _ in N.ClmLlamaLayer._fields_]
    fd = [n for n, _ in N.ClmLlamaDesc._fields_]
    body = "".join(f'printf("L.{f} %zu\\n", offsetof(b2t_clm_llama_layer_t, {f}));' for f in fl) + \
           "".join(f'printf("D.{f} %zu\\n", offsetof(b2t_clm_llama_t, {f}));' for f in fd)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){'
                   'printf("L %zu\\nD %zu\\n", sizeof(b2t_clm_llama_layer_t), sizeof(b2t_clm_llama_t));' + body + "return 0;}")
    exe = tmp_path / "lay"
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["L"]) == C.sizeof(N.ClmLlamaLayer) and int(got["D"]) == C.sizeof(N.ClmLlamaDesc)
    for f in fl:
        assert int(got["L." + f]) == getattr(N.ClmLlamaLayer, f).offset, f
    for f in fd:
        assert int(got["D." + f]) == getattr(N.ClmLlamaDesc, f).offset, f
    assert len(fl) == 7 and len(fd) == 14


def _model(n_layers=1, d=256, heads=4, kv=2, ffn=512, vocab=1000, max_pos=64, eps=1e-5, bias=True):
    import b2t_native as N
    layers = (N.ClmLlamaLayer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmLlamaLayer._fields_:
            setattr(layers[i], f, FAKE if (bias or f != "qkv_b") else None)
    desc = N.ClmLlamaDesc(n_layers, d, heads, kv, ffn, vocab, max_pos, eps, FAKE, FAKE, FAKE, FAKE, FAKE, layers)
    desc._keep = layers
    return desc


def test_ws_bytes():
    import b2t_native as N
    lib = N.load()
    desc = _model()
    ws = lambda M, n: lib.b2t_clm_llama_ws_bytes(C.byref(desc), M, n)
    assert lib.b2t_clm_llama_ws_bytes(None, 10, 1) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert ws(n_tok, n_seq) == 0, (n_tok, n_seq)
    d, Fd, V, qw = 256, 512, 1000, (4 + 2 * 2) * 64
    ncg = (V + 63) // 64
    prev = 0
    for M in list(range(1, 600, 7)) + [4095, 4096, 4097]:
        for n_seq in sorted({1, max(1, M // 3), M}):
            b = ws(M, n_seq)
            Mh, Mp = M - n_seq, -(-M // 256) * 256
            parts = [4 * (2 * M + 2 * Mh + 2 * (n_seq + 1)), 4 * M * d, 2 * Mp * d, 2 * M * qw, 2 * Mp * Fd,
                     4 * Mh * ncg, 4 * Mh * ncg, 4 * Mh, 4 * Mh]
            assert b >= sum(parts) and b % 256 == 0, (M, n_seq, b, sum(parts))
        b1 = ws(M, 1)
        assert b1 >= prev, M
        prev = b1
    sizes = [ws(M, 4) for M in range(4, 2000, 13)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    # the tree call
    tws = lambda nn, nt, ns: lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), nn, nt, ns)
    assert lib.b2t_clm_llama_tree_ws_bytes(None, 5, 10, 1) == 0
    for nn, nt, ns in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert tws(nn, nt, ns) == 0, (nn, nt, ns)
    for M in (1, 2, 255, 256, 257, 600, 4097):
        for Mn in sorted({1, M // 2 + 1, M}):
            for n_seq in sorted({1, max(1, M // 3), M}):
                b = tws(Mn, M, n_seq)
                Mp = -(-Mn // 256) * 256
                parts = [4 * (4 * Mn + 2 * M + 2 * n_seq + 1), 4 * Mn * d, 2 * Mp * d, 2 * Mn * qw, 2 * Mp * Fd,
                         4 * Mn * ncg, 4 * Mn * ncg, 4 * Mn, 4 * Mn]
                assert b >= sum(parts) and b % 256 == 0, (Mn, M, n_seq, b, sum(parts))
    for s in ([tws(Mn, 3000, 7) for Mn in range(1, 3001, 11)], [tws(40, M, 7) for M in range(40, 3000, 13)],
              [tws(40, 3000, n) for n in range(1, 3001, 17)]):
        assert all(a > 0 for a in s) and all(a <= b for a, b in zip(s, s[1:]))
    assert tws(500, 2500, 100) < tws(2500, 2500, 100)
    # a descriptor whose sizes mean nothing
    assert lib.b2t_clm_llama_ws_bytes(C.byref(_model(heads=0)), 10, 1) == 0
    assert lib.b2t_clm_llama_tree_ws_bytes(C.byref(_model(kv=0)), 5, 10, 1) == 0


def _call(lib, tree, desc, ids, off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    n = len(off) - 1 if n_seq is None else n_seq
    dp = C.byref(desc) if desc is not None else None
    if tree:
        return lib.b2t_clm_llama_score_tree_f16(dp, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
    return lib.b2t_clm_llama_score_f16(dp, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)


@pytest.mark.parametrize("tree", [False, True])
def test_score_refusals_before_device_work(tree):
    """Every refusal returns before any device work: the test needs no GPU and the pointers are fake."""
    import b2t_native as N
    lib = N.load()
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, **kw):
        rc = _call(lib, tree, desc, ids, off, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())

    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8, kv=8))
    refused("head dim 80", _model(d=320, heads=4, kv=4))            # OPT's 80 is not the Llama family's
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
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    for desc in (_model(), _model(bias=False)):     # a null qkv_b is a model without q / k / v biases, not an error
        need = (lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 4, 2) if tree else lib.b2t_clm_llama_ws_bytes(C.byref(desc), 4, 2))
        assert need > 0
        refused("workspace", desc, ws_bytes=need - 1)
    if tree:
        desc = _model()
        ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]    # 9 tokens, 4 nodes
        need = lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 4, 9, 3)
        assert 0 < need <= lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), 9, 9, 3)
        refused("workspace", desc, ids=ids, off=off, ws_bytes=need - 1)


# ---- the kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_llama_kernels_do_not_spill():
    # the bound of tests/test_clm_host.py; at the time of writing: the 256-tile GEMMs 222 VGPRs, the 128-tile ones 86, embed
    # and RMSNorm 16, scratch 0 everywhere.  The unit has no attention kernel of its own: it launches clm_attn_kernel
    # (causal_lm.hip) and clm_attn_tree_kernel (causal_lm_tree.hip), the kernels OPT runs, so their scratch-0 and register
    # assertions are the ones test_clm_kernels_do_not_spill and test_tree_kernels_do_not_spill make
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm_llama.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_kernel" in k]
    # the two new epilogues on both tiles; the other four epilogues are instantiated in causal_lm.hip alone
    assert len(gemm) == 4 and not [k for k in res if "attn" in k] and len(res) == 6, sorted(res)
    assert any("clm_llama_embed_kernel" in k for k in res) and any("clm_llama_rmsnorm_kernel" in k for k in res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_one_tile_rule_for_both_families():
    """The Llama unit launches its GEMMs through causal_lm.hip's launch_gemm (the rule tests/test_clm_host.py pins) and has
    no tile rule of its own."""
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm_llama.hip")).read()
    assert "B2T_CLM_GEMM_256" not in src and "getenv" not in src
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_ROPE>)") == 1
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_SWIGLU>)") == 1
    hdr = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "clm_gemm.h")).read()
    assert "getenv" not in hdr


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(tmp_path):
    import inspect
    import llm_rescore as R
    for fn in ("score", "token_logprobs", "eval"):
        assert callable(getattr(R.LlamaScorer, fn))
    for name in ("share_prefixes",):
        assert inspect.signature(R.LlamaScorer.__init__).parameters[name].default is False
    assert inspect.signature(R.LlamaScorer.__init__).parameters["context_cache_tokens"].default == 0
    assert list(inspect.signature(R.LlamaScorer.score).parameters) == list(inspect.signature(R.OptScorer.score).parameters)
    assert list(inspect.signature(R.LlamaScorer.token_logprobs).parameters) == \
        list(inspect.signature(R.OptScorer.token_logprobs).parameters)
    assert list(inspect.signature(R.LlamaScorer.__init__).parameters) == list(inspect.signature(R.OptScorer.__init__).parameters)
    assert inspect.signature(R.build_opt).parameters["max_positions"].default is None
    model, cfg = tiny_model("qwen2")
    model.save_pretrained(str(tmp_path))
    # the weights only have to be addressable for the descriptor: device "cpu" builds it without a GPU
    sc = R.build_scorer(str(tmp_path), device="cpu")
    assert isinstance(sc, R.LlamaScorer) and sc.share_prefixes is False and sc.context_cache_tokens == 0
    assert sc.eval() is sc and str(sc.device) == "cpu" and sc.last_stats is None
    assert sc.desc.n_kv_heads == 1 and sc.desc.n_heads == 4 and sc.desc.max_pos == 256 and sc.desc.vocab == 777
    assert sc.desc.lm_head == sc.desc.embed_tokens                 # tied
    assert sc.desc.layers_host[0].qkv_b                            # Qwen2's biases
    assert R.build_scorer(str(tmp_path), device="cpu", share_prefixes=True).share_prefixes is True
    assert R.build_scorer(str(tmp_path), device="cpu", max_positions=100).desc.max_pos == 100
    with pytest.raises(ValueError, match="context_cache_tokens"):
        R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=64)
    with pytest.raises(ValueError, match="context cache"):
        R.LlamaScorer(sc.dims, {k: v for k, v in sc.w.items()}, "cpu", False, 64)
    with pytest.raises(ValueError, match="context cache"):
        sc.score([[2, 3]], use_cache=True)
    assert sc.score([]).shape == (0,)
    # build_opt itself: the directory needs a tokenizer
    tok_ok = _save_word_tokenizer(str(tmp_path), 777)
    if tok_ok:
        s2, tok = R.build_opt(str(tmp_path), device="cpu")
        assert isinstance(s2, R.LlamaScorer) and tok.padding_side == "right" and tok.pad_token is not None
        with pytest.raises(ValueError, match="context_cache_tokens"):
            R.build_opt(str(tmp_path), device="cpu", context_cache_tokens=8)
    m2, _ = tiny_model("llama", n_layers=1)
    d2 = tmp_path / "untied"
    m2.save_pretrained(str(d2))
    s3 = R.build_scorer(str(d2), device="cpu")
    assert s3.desc.lm_head != s3.desc.embed_tokens and not s3.desc.layers_host[0].qkv_b


def _save_word_tokenizer(path, vocab):
    """A word-level tokenizer.json in `path` (the tokenizers library, offline); False where the library is missing."""
    try:
        from tokenizers import Tokenizer, models, pre_tokenizers
        from transformers import PreTrainedTokenizerFast
    except ImportError:
        return False
    words = {"<pad>": 1, "<s>": 2, "<unk>": 0, "</s>": 3}
    words.update({f"w{i}": i for i in range(4, vocab)})
    t = Tokenizer(models.WordLevel(words, unk_token="<unk>"))
    t.pre_tokenizer = pre_tokenizers.Whitespace()
    PreTrainedTokenizerFast(tokenizer_object=t, bos_token="<s>", eos_token="</s>", unk_token="<unk>").save_pretrained(path)
    return True
