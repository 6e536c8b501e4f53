"""Host-side checks of the fine-grained FP8 spelling of a Llama-family checkpoint (quantization_config quant_method "fp8",
float8_e4m3fn weights beside fp32 weight_scale_inv blocks; no GPU): the dense reading of such a directory against an expansion
written out here, the packed layout of linear_weights="fp8" against the dense one, the bytes the packed projections take, every
refusal by its message, and the refusals of csrc/causal_lm_llama_fp8.hip's entry points before any device work.

fp8_state (shared with tests/test_gpu_clm_fp8.py) is a random state dict in that spelling whose codes are uniform over the 254
codes that are no NaN -- subnormals, +-0 and +-448 included -- and whose scales are 2^U(-9, -5) with full 24-bit mantissas, a
different one in every block: a neighbour's scale, a scale row off by one, a truncated product or a swapped byte moves the result.

None of this exists without the feature: the dense reading casts the codes by value on a tree that lacks it (test_dense_read),
and the keyword, the layout and the symbols are not there."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, _model, tiny_model, tiny_seqs
from test_clm_qwen3_host import _qkn, ref_logp_qwen3, tiny_qwen3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("score_f16", "score_tree_f16", "score_tree_cached_f16", "score_bf16", "score_tree_bf16")
LINEARS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
           "mlp.down_proj")
# the three models of the GPU identity test: (config, block)
QWEN3_WIDE = dict(hidden_size=512, num_attention_heads=4, num_key_value_heads=2, intermediate_size=640)
_CFG = {}


def model_cfg(name):
    """config.json's dict of "llama" (d 256, 4 / 2 heads of 64, ffn 320), "qwen2" (d 512, head dim 128, ffn 448, q / k / v biases)
    or "qwen3" (d 512, 4 / 2 heads of 128, ffn 640), from tiny_model / tiny_qwen3, whose weights are not used"""
    if name not in _CFG:
        _CFG[name] = tiny_qwen3("hd128", **QWEN3_WIDE)[1] if name == "qwen3" else tiny_model(name)[1]
    return dict(_CFG[name])


MODELS = {"llama": (32, 64), "qwen2": (64, 64), "qwen3": (128, 128)}   # the block each is packed in


def linear_shapes(cfg):
    d, Hq, F = cfg["hidden_size"], cfg["num_attention_heads"], cfg["intermediate_size"]
    hd = d // Hq
    kv = (cfg.get("num_key_value_heads") or Hq) * hd
    return {"self_attn.q_proj": (d, d), "self_attn.k_proj": (kv, d), "self_attn.v_proj": (kv, d), "self_attn.o_proj": (d, d),
            "mlp.gate_proj": (F, d), "mlp.up_proj": (F, d), "mlp.down_proj": (d, F)}


def fp8_state(cfg, fmt="float16", seed=0, block=(128, 128), device="cpu"):
    """The packed state dict of a tiny model with config cfg: every linear of every layer as a float8_e4m3fn weight [N][K] of
    codes uniform over the 254 non-NaN codes and an fp32 weight_scale_inv [N / bn][K / bk] of 2^U(-9, -5); embedding, head (unless
    tied), norms, q / k norms (Qwen3) and q / k / v biases (Qwen2) random in fmt, in tiny_model's spreads."""
    import torch
    bn, bk = block
    g = torch.Generator().manual_seed(7000 + seed)
    wdt = getattr(torch, fmt)
    d, V, hd = cfg["hidden_size"], cfg["vocab_size"], cfg["hidden_size"] // cfg["num_attention_heads"]
    rn = lambda *shape: torch.randn(shape, generator=g)
    st = {"model.embed_tokens.weight": (rn(V, d) * 2.0 / d ** 0.5).to(wdt), "model.norm.weight": (1 + 0.2 * rn(d)).to(wdt)}
    if not cfg.get("tie_word_embeddings"):
        st["lm_head.weight"] = (rn(V, d) * 2.0 / d ** 0.5).to(wdt)
    ok = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
    assert len(ok) == 254
    for l in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{l}."
        st[p + "input_layernorm.weight"] = (1 + 0.2 * rn(d)).to(wdt)
        st[p + "post_attention_layernorm.weight"] = (1 + 0.2 * rn(d)).to(wdt)
        if cfg["model_type"] == "qwen3":
            st[p + "self_attn.q_norm.weight"] = (1 + 0.2 * rn(hd)).to(wdt)
            st[p + "self_attn.k_norm.weight"] = (1 + 0.2 * rn(hd)).to(wdt)
        for n, (N, K) in linear_shapes(cfg).items():
            st[p + n + ".weight"] = ok[torch.randint(0, 254, (N, K), generator=g)].view(torch.float8_e4m3fn)
            st[p + n + ".weight_scale_inv"] = torch.exp2(-9 + 4 * torch.rand((N // bn, K // bk), generator=g, dtype=torch.float64)).float()
            if cfg["model_type"] == "qwen2" and n in LINEARS[:3]:
                st[p + n + ".bias"] = (0.3 * rn(N)).to(wdt)
    return {k: v.to(device) for k, v in st.items()}


def quant_config(block, **over):
    return dict({"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": list(block), "activation_scheme": "dynamic",
                 "modules_to_not_convert": ["lm_head"]}, **over)


def save_fp8(path, cfg, st, block, dtype="bfloat16", **over):
    """the directory of a checkpoint in the FP8 spelling: config.json with the quantization_config, model.safetensors"""
    from safetensors.torch import save_file
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(dict(cfg, torch_dtype=dtype, quantization_config=quant_config(block, **over)), f)
    save_file({k: v.cpu().contiguous() for k, v in st.items()}, os.path.join(path, "model.safetensors"))
    return path


def expand(q, s, bn, bk):
    """the contract, written out independently of llm_rescore.fp8_dequant: fp32 (q.float() * s_expanded)"""
    N, K = q.shape
    se = s[np.arange(N) // bn][:, np.arange(K) // bk]
    return q.float() * se


def plain_of(st, block, fmt):
    """the plain spelling of a packed state dict in fmt: HF's Fp8Dequantize rule, (q.float() * s_expanded).to(dtype)"""
    import torch
    out = {k: v for k, v in st.items() if not k.endswith("weight_scale_inv")}
    for k in st:
        if k.endswith("weight_scale_inv"):
            n = k[:-len("_scale_inv")]
            out[n] = expand(st[n], st[k], *block).to(getattr(torch, fmt))
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t.contiguous()


def weight_bytes(dims, bk):
    """the derived number: per layer the sum over the four GEMMs of rows_padded K + 4 (rows_padded / 32) (K / bk)"""
    d, F, hd = dims["d_model"], dims["ffn_dim"], dims["d_model"] // dims["n_heads"]
    rup = lambda x: -(-x // 256) * 256
    groups = [(rup((dims["n_heads"] + 2 * dims["n_kv_heads"]) * hd), d), (rup(d), d), (rup(2 * F), d), (rup(d), F)]
    return dims["n_layers"] * sum(r * K + 4 * (r // 32) * (K // bk) for r, K in groups)


# ---- the state dict itself --------------------------------------------------------------------------------------------------
def test_fp8_state_covers_the_codes_and_varies_the_scales():
    import torch
    cfg = model_cfg("qwen3")
    st = fp8_state(cfg, block=(128, 128))
    q = st["model.layers.0.mlp.gate_proj.weight"].view(torch.uint8)
    assert sorted(set(q.flatten().tolist())) == [c for c in range(256) if c & 0x7F != 0x7F]
    s = st["model.layers.0.mlp.gate_proj.weight_scale_inv"]
    assert s.dtype == torch.float32 and tuple(s.shape) == (5, 4) and 2.0 ** -9 <= float(s.min()) and float(s.max()) <= 2.0 ** -5
    assert len(set(s.flatten().tolist())) == s.numel() and (s.view(torch.int32) & 0xFFF != 0).all()   # no short mantissas


# ---- the dense reading ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_dense_read(name, fmt, tmp_path):
    """build_scorer(dir, device="cpu") of an FP8 directory holds, tensor for tensor and byte for byte, llama_device_layout of the
    plain state dict whose weights are (q.float() * s_expanded).to(dtype), the expansion written out above; dtype "auto" reads
    torch_dtype as for any checkpoint; the fp64 restatement of the family's contract is finite on that state dict, so a NaN on the
    GPU is the kernels'.  Fails on a tree that casts the codes by value."""
    import torch
    import llm_rescore as R
    cfg, block = model_cfg(name), MODELS[name]
    st = fp8_state(cfg, fmt, seed=1, block=block)
    path = save_fp8(str(tmp_path / name), cfg, st, block, dtype=fmt)
    sc = R.build_scorer(path, device="cpu", dtype=fmt)
    assert type(sc) is R.LlamaScorer and sc.dtype is getattr(torch, fmt)
    assert R.build_scorer(path, device="cpu", dtype="auto").dtype is getattr(torch, fmt)
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    plain = plain_of(st, block, fmt)
    want = R.llama_device_layout(plain, dims, inv, dtype=fmt)
    assert sorted(sc.w) == sorted(want) and "layers.1.down_w" in want
    for k, v in want.items():
        assert sc.w[k].dtype == v.dtype and torch.equal(_bits(sc.w[k]), _bits(v)), k
    dims2, arr = R.load_llama_arrays(path, dtype=fmt)
    assert dims2 == dims and all(torch.equal(_bits(arr[k]), _bits(v)) for k, v in want.items())
    w = want["layers.0.qkv_w"].float()
    assert torch.isfinite(w).all() and float(w.abs().max()) > 1.0    # scaled values, not codes cast by value (those reach 448)
    assert float(w.abs().max()) <= 448 * 2.0 ** -5
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=(1, 17, 33, 100))
    logp = ref_logp_qwen3(plain, dict(dims, rms_eps=cfg["rms_norm_eps"]), inv, seqs, fmt, qk_norm=name == "qwen3")
    assert all(np.isfinite(t).all() for t in logp) and min(t.min() for t in logp) < -1.0


def test_fp8_dequant_is_the_written_out_expansion():
    import torch
    import llm_rescore as R
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 127, (64, 192), generator=g, dtype=torch.uint8)
    s = torch.exp2(-130 + 140 * torch.rand((2, 3), generator=g, dtype=torch.float64)).float()   # down to fp32-subnormal products
    got = R.fp8_dequant(q.view(torch.float8_e4m3fn), s, 32, 64)
    assert got.dtype == torch.float32 and torch.equal(got.view(torch.int32), expand(q.view(torch.float8_e4m3fn), s, 32, 64).view(torch.int32))
    assert torch.equal(R.fp8_dequant(q, s, 32, 64), got)          # the same bytes as uint8
    assert ((got != 0) & (got.abs() < 2.0 ** -126)).any()          # subnormal products are kept
    with pytest.raises(ValueError, match=r"x: shape 64 x 192 is not a multiple of the block \[48, 64\]"):
        R.fp8_dequant(q, s, 48, 64, "x")
    with pytest.raises(ValueError, match=r"scales \(2, 3\) do not go with codes 64 x 192 in blocks of \[64, 64\]"):
        R.fp8_dequant(q, s, 64, 64)


# ---- the packed layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_packed_layout(name, fmt, tmp_path):
    """linear_weights="fp8": <g>_q is the codes under the dense matrices' row permutation and zero padding, <g>_s the scale of
    every 32 stored rows; re-expanded on the host and cast they are the dense arrays to the byte; every other array is the dense
    layout's; weight_bytes() is the derived number; the descriptor points at the arrays and the model holds no dense projection."""
    import torch
    import b2t_native as N
    import llm_rescore as R
    cfg, (bn, bk) = model_cfg(name), MODELS[name]
    st = fp8_state(cfg, fmt, seed=2, block=(bn, bk))
    path = save_fp8(str(tmp_path / name), cfg, st, (bn, bk), dtype=fmt)
    dense = R.build_scorer(path, device="cpu", dtype=fmt)
    sc = R.build_scorer(path, device="cpu", dtype=fmt, linear_weights="fp8")
    assert type(sc) is R.Fp8LlamaScorer and isinstance(sc, R.LlamaScorer) and sc._family == "llama_fp8" and sc.block_k == bk
    assert sc._SIZES == "b2t_clm_llama_" and sc._size_args == () and sc.dtype is dense.dtype
    mats = ("qkv", "o", "gate_up", "down")
    packed = {k for k in sc.w if k.endswith(tuple(R._FP8_FIELDS))}
    assert len(packed) == 8 * cfg["num_hidden_layers"] and R._FP8_FIELDS == tuple(m + t for m in mats for t in ("_q", "_s"))
    assert sorted(set(sc.w) - packed) == sorted(k for k in dense.w if not k.endswith(tuple(m + "_w" for m in mats)))
    for k in set(sc.w) - packed:
        assert torch.equal(_bits(sc.w[k]), _bits(dense.w[k])), k
    dims = sc.dims
    Hq, Hkv, hd, d, F = dims["n_heads"], dims["n_kv_heads"], dims["d_model"] // dims["n_heads"], dims["d_model"], dims["ffn_dim"]
    qperm, gperm = R.qkv_row_perm(Hq, Hkv, hd), R.gate_up_row_perm(F)
    for l in range(dims["n_layers"]):
        p = f"model.layers.{l}."
        cat = lambda ns, suf, f: torch.cat([f(st[p + n + suf]) for n in ns], 0)
        codes = lambda ns: cat(ns, ".weight", lambda t: t.view(torch.uint8))
        rowsc = lambda ns: cat(ns, ".weight_scale_inv", lambda t: t.repeat_interleave(bn, 0))     # a scale row per row
        src = {"qkv": (LINEARS[:3], qperm), "o": (LINEARS[3:4], None), "gate_up": (LINEARS[4:6], gperm), "down": (LINEARS[6:], None)}
        for m, (ns, perm) in src.items():
            q, s, w = sc.w[f"layers.{l}.{m}_q"], sc.w[f"layers.{l}.{m}_s"], dense.w[f"layers.{l}.{m}_w"]
            cq, cs = codes(ns), rowsc(ns)
            if perm is not None:
                cq, cs = cq[perm], cs[perm]
            n, K = cq.shape
            assert q.dtype is torch.uint8 and s.dtype is torch.float32 and tuple(q.shape) == tuple(w.shape) and q.shape[0] % 256 == 0
            assert tuple(s.shape) == (q.shape[0] // 32, K // bk)
            assert torch.equal(q[:n], cq) and not q[n:].any() and not s[-(-n // 32):].any()
            assert torch.equal(s[:n // 32].repeat_interleave(32, 0), cs[:n // 32 * 32])
            back = R.fp8_dequant(q, s, 32, bk).to(dense.dtype)
            assert torch.equal(_bits(back), _bits(w)) and (w != 0).any(), (l, m)
            assert getattr(sc._fp8_layers[l], m + "_q") == q.data_ptr() and getattr(sc._fp8_layers[l], m + "_s") == s.data_ptr()
            assert not getattr(sc.desc.layers_host[l], m + "_w")
        assert sc.desc.layers_host[l].norm1_w == sc.w[f"layers.{l}.norm1_w"].data_ptr()
    assert sc.weight_bytes() == weight_bytes(dims, bk) == sum(sc.w[k].numel() * sc.w[k].element_size() for k in packed)
    assert sc._fp8.block_k == bk and isinstance(sc._fp8, N.ClmLlamaFp8)
    assert (sc._qk[0] is not None) == (name == "qwen3") and sc._qk[1] is sc._fp8
    assert sc.score([]).shape == (0,)
    dims2, arr = R._load_arrays(R._family_for(R.FAMILIES[cfg["model_type"]], "dense", "fp8", json.load(open(path + "/config.json"))),
                                path, dtype=fmt)
    assert "layers.1.down_q" in arr and "layers.1.down_w" not in arr
    with pytest.raises(KeyError, match="qkv_q"):
        R.Fp8LlamaScorer(dims, dense.w, "cpu", dtype=fmt)
    with pytest.raises(ValueError, match="layers.0.o_s is torch.float64, expected torch.float32"):
        R.Fp8LlamaScorer(dims, dict(arr, **{"layers.0.o_s": arr["layers.0.o_s"].double()}), "cpu", dtype=fmt)


def test_8b_arithmetic():
    """the memory claim of the documents, from the derived number: Llama-3-8B's four projections a layer in FP8 at [128, 128]"""
    dims = dict(n_layers=32, d_model=4096, n_heads=32, n_kv_heads=8, ffn_dim=14336)
    packed = weight_bytes(dims, 128)
    dense = 2 * 32 * (6144 * 4096 + 4096 * 4096 + 28672 * 4096 + 4096 * 14336)
    assert dense == 13958643712 and packed == dense // 2 + dense // 2 // 1024 == 6986137600    # a byte a weight, and 4 / (32 * 128)


# ---- the refusals ---------------------------------------------------------------------------------------------------------------
def test_keyword_and_config_refusals(tmp_path):
    """Everything that is refused before any weight is read: the directories hold a config.json and nothing else."""
    import inspect
    import llm_rescore as R
    cfg = model_cfg("llama")

    def bare(name, cfg, **q):
        os.makedirs(tmp_path / name)
        with open(tmp_path / name / "config.json", "w") as f:
            json.dump(dict(cfg, **({"quantization_config": q} if q else {})), f)
        return str(tmp_path / name)
    for fn in (R.build_scorer, R.build_opt):
        par = inspect.signature(fn).parameters
        assert par["linear_weights"].default == "dense" and par["linear_weights"].kind is inspect.Parameter.KEYWORD_ONLY
        assert list(par).index("linear_weights") + 1 == list(par).index("expert_weights")
    assert R.LINEAR_WEIGHTS == ("dense", "fp8")
    for qm in ("compressed-tensors", "gptq", "awq", "bitsandbytes", "mxfp4", "fbgemm_fp8", None):
        with pytest.raises(ValueError, match=f"quant_method {qm!r} is not supported"):
            R.build_scorer(bare(f"qm-{qm}", cfg, quant_method=qm), device="cpu")
    with pytest.raises(ValueError, match="fmt 'e5m2' is not supported"):
        R.build_scorer(bare("e5m2", cfg, **quant_config((128, 128), fmt="e5m2")), device="cpu")
    for block, said in (((48, 64), r"\[48, 64\]"), ((32, 96), r"\[32, 96\]"), ((0, 64), r"\[0, 64\]")):
        with pytest.raises(ValueError, match="weight_block_size " + said + " is not supported"):
            R.build_scorer(bare("b%d-%d" % block, cfg, **quant_config(block)), device="cpu")
    with pytest.raises(ValueError, match="weight_block_size None is not supported"):
        R.build_scorer(bare("pertensor", cfg, quant_method="fp8", activation_scheme="static"), device="cpu")
    assert R.fp8_block(dict(cfg, quantization_config={"quant_method": "fp8", "weight_block_size": [64, 192]})) == (64, 192)
    assert R.fp8_block(cfg) is None and R.fp8_block({"model_type": "gpt_oss", "quantization_config": {"quant_method": "mxfp4"}}) is None
    # linear_weights="fp8": a plain checkpoint, another family, a bad value, bfloat16 with a cache
    with pytest.raises(ValueError, match="quantising a plain checkpoint is not built"):
        R.build_scorer(bare("plain", cfg), device="cpu", linear_weights="fp8")
    for mt in ("gemma2", "gpt_oss", "olmo2", "opt"):
        with pytest.raises(ValueError, match=f"linear_weights='fp8' is for llama, mistral, qwen2, qwen3 checkpoints.*{mt!r}"):
            R.build_scorer(bare("fam-" + mt, {"model_type": mt}), device="cpu", linear_weights="fp8")
    with pytest.raises(ValueError, match="FP8 checkpoints are read for llama, mistral, qwen2, qwen3 only, not model_type 'olmo2'"):
        R.build_scorer(bare("olmo2-fp8", {"model_type": "olmo2"}, **quant_config((128, 128))), device="cpu")
    for bad in ("FP8", "e4m3", None, "", "mxfp4"):
        with pytest.raises(ValueError, match="linear_weights .* is not one of"):
            R.build_scorer(bare(f"kw-{bad}", cfg, **quant_config((128, 128))), device="cpu", linear_weights=bad)
    fp8_dir = bare("fp8", cfg, **quant_config((128, 128)))
    with pytest.raises(ValueError, match="dtype 'bfloat16' with context_cache_tokens > 0 is not supported"):
        R.build_scorer(fp8_dir, device="cuda", dtype="bfloat16", context_cache_tokens=64, linear_weights="fp8")
    with pytest.raises(ValueError, match="context cache .* lives in GPU memory"):
        R.build_scorer(fp8_dir, device="cpu", context_cache_tokens=64, linear_weights="fp8")
    with pytest.raises(FileNotFoundError):      # everything above passed: the next thing is the weights
        R.build_scorer(fp8_dir, device="cpu", linear_weights="fp8")


@pytest.mark.parametrize("how", ["dense", "fp8"])
def test_tensor_refusals(how):
    """What is refused by the tensor's name, alike by the dense reading and by the packed layout."""
    import torch
    import llm_rescore as R
    cfg, block = model_cfg("llama"), (32, 64)
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    base = fp8_state(cfg, "bfloat16", seed=3, block=block)

    def load(st, fmt="float16", blk=block):
        if how == "fp8":
            return R.llama_fp8_device_layout(st, dims, inv, fmt, blk)
        return R.llama_device_layout(R.fp8_dense_state(st, dims, blk, fmt), dims, inv, fmt)
    assert "layers.1." + ("down_q" if how == "fp8" else "down_w") in load(base)
    # k_proj has 128 rows, down_proj 320 columns: checkpoints whose other linears go with the block
    with pytest.raises(ValueError, match=r"layers\.0\.self_attn\.k_proj\.weight: shape 128 x 256 is not a multiple of the block \[256, 64\]"):
        load(fp8_state(cfg, "bfloat16", seed=3, block=(256, 64)), blk=(256, 64))
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj\.weight: shape 256 x 320 is not a multiple of the block \[32, 128\]"):
        load(fp8_state(cfg, "bfloat16", seed=3, block=(32, 128)), blk=(32, 128))
    with pytest.raises(ValueError, match=r"q_proj\.weight: scales \(8, 4\) do not go with codes 256 x 256 in blocks of \[64, 64\]"):
        load(base, blk=(64, 64))
    k = "model.layers.1.mlp.up_proj.weight"
    for code in (0x7F, 0xFF):
        q = base[k].view(torch.uint8).clone()
        q[100, 200] = code
        with pytest.raises(ValueError, match=r"layers\.1\.mlp\.up_proj\.weight: a NaN code"):
            load(dict(base, **{k: q.view(torch.float8_e4m3fn)}))
    for bad in (float("inf"), float("nan"), float("-inf")):
        s = base[k + "_scale_inv"].clone()
        s[3, 1] = bad
        with pytest.raises(ValueError, match=r"layers\.1\.mlp\.up_proj\.weight_scale_inv: a scale is not finite"):
            load(dict(base, **{k + "_scale_inv": s}))
    for gone in ("q_proj", "k_proj", "v_proj"):
        st = {n: v for n, v in base.items() if n != f"model.layers.1.self_attn.{gone}.weight_scale_inv"}
        with pytest.raises(ValueError, match=rf"lacks model\.layers\.1\.self_attn\.{gone}\.weight_scale_inv"):
            load(st)
    st = {n: v for n, v in base.items() if not n.startswith("model.layers.1.") or "o_proj.weight_scale_inv" not in n}
    st["model.layers.1.self_attn.o_proj.weight"] = torch.zeros(256, 256, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match=r"model\.layers\.1\.self_attn\.o_proj is plain and model\.layers\.0\.self_attn\.o_proj is not"):
        load(st)
    with pytest.raises(ValueError, match=r"lm_head\.weight_scale_inv: only the layers'"):
        load(dict(base, **{"lm_head.weight_scale_inv": torch.ones(1, 1)}))
    with pytest.raises(ValueError, match=r"o_proj\.weight is torch\.bfloat16 beside a weight_scale_inv"):
        load(dict(base, **{"model.layers.0.self_attn.o_proj.weight": torch.zeros(256, 256, dtype=torch.bfloat16)}))
    # 448 * 150 = 67200 > 65504: over range in fp16, a number in bf16; one below, 448 * 146 = 65408, passes in both
    q = base[k].view(torch.uint8).clone()
    q[64, 64] = 0xFE                                   # -448
    for scale, f16_ok in ((150.0, False), (146.0, True)):
        s = base[k + "_scale_inv"].clone()
        s[2, 1] = scale
        st = dict(base, **{k: q.view(torch.float8_e4m3fn), k + "_scale_inv": s})
        load(st, "bfloat16")
        if f16_ok:
            load(st, "float16")
        else:
            with pytest.raises(ValueError, match=r"up_proj\.weight / weight_scale_inv: a value is not finite in torch\.float16"):
                load(st, "float16")
    # a group that the checkpoint holds plain is read by the dense reading and refused by the packed layout
    st = {n: v for n, v in base.items() if "o_proj.weight_scale_inv" not in n}
    for l in range(2):
        st[f"model.layers.{l}.self_attn.o_proj.weight"] = torch.zeros(256, 256, dtype=torch.bfloat16)
    if how == "dense":
        assert not load(st)["layers.0.o_w"].any()
    else:
        with pytest.raises(ValueError, match=r"lacks model\.layers\.0\.self_attn\.o_proj\.weight_scale_inv"):
            load(st)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_bound():
    """The five score calls have the Qwen3 twins' lists with the fp8 descriptor behind the q / k norm array, in the header and in
    the bindings; the two unpack calls theirs; there is no new size function; the records have the C layout."""
    import b2t_native as N
    lib = N.load()
    hdr = open(os.path.join(ROOT, "include", "b2t.h")).read()
    decl = lambda n: [a.strip() for a in re.sub(r"\s+", " ", re.search(r"\n(?:int|size_t) " + n + r"\((.*?)\);", hdr, re.S).group(1)).split(",")]
    for t in ENTRY:
        new, twin = "b2t_clm_llama_fp8_" + t, "b2t_clm_qwen3_" + t
        dn, dt = decl(new), decl(twin)
        assert dn == dt[:2] + ["const b2t_clm_llama_fp8_t* fp8"] + dt[2:], new
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == list(g.argtypes[:2]) + [C.POINTER(N.ClmLlamaFp8)] + list(g.argtypes[2:])
    for t in ("f16", "bf16"):
        f = getattr(lib, "b2t_clm_fp8_unpack_" + t)
        assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        assert decl("b2t_clm_fp8_unpack_" + t) == ["const void* q", "const void* s", "long long rows", "int K", "int block_k", "void* out",
                                                   "void* stream"]
    names = re.findall(r"\b(b2t_clm_(?:llama_)?fp8_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert sorted(names) == sorted(["b2t_clm_llama_fp8_" + t for t in ENTRY] + ["b2t_clm_fp8_unpack_f16", "b2t_clm_fp8_unpack_bf16"])
    assert set(names) <= set(N.header_symbols())
    assert [f for f, _ in N.ClmLlamaFp8Layer._fields_] == ["qkv_q", "qkv_s", "o_q", "o_s", "gate_up_q", "gate_up_s", "down_q", "down_s"]
    assert C.sizeof(N.ClmLlamaFp8Layer) == 64 and C.sizeof(N.ClmLlamaFp8) == 16 and N.ClmLlamaFp8.layers_host.offset == 8
    for f, _ in N.ClmLlamaFp8Layer._fields_:
        assert re.search(r"const void \*" + f[:-2] + r"_q, \*" + f[:-2] + r"_s;", hdr), f
    assert re.search(r"int block_k;[^}]*const b2t_clm_llama_fp8_layer_t\* layers_host;[^}]*\} b2t_clm_llama_fp8_t;", hdr, re.S)


def _fp8(n_layers=1, block_k=128, layers=True, **null):
    import b2t_native as N
    arr = (N.ClmLlamaFp8Layer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmLlamaFp8Layer._fields_:
            setattr(arr[i], f, None if null.get(f) == i + 1 else FAKE)
    desc = N.ClmLlamaFp8(block_k, arr if layers else None)
    desc._keep = arr
    return desc


def _packed_model(bias=False, **kw):
    """_model's descriptor as a caller of the fp8 calls holds it: no dense projections"""
    desc = _model(bias=bias, **kw)
    for i in range(desc.n_layers):
        for f in ("qkv_w", "o_w", "gate_up_w", "down_w"):
            setattr(desc.layers_host[i], f, None)
    return desc


@pytest.mark.parametrize("qwen3", [False, True], ids=["llama", "qwen3"])
@pytest.mark.parametrize("entry", ENTRY)
def test_refusals_before_device_work(entry, qwen3):
    """With fake pointers and no GPU: a null descriptor, a null layers_host or pointer inside it, a model that holds dense
    projections as well and a block_k the tile cannot follow are refused under the call's own name; what the Llama and Qwen3 twins
    refuse of the model, the norm array and the lists is refused as they refuse it; the workspace is the Llama size functions';
    on the cached call the cache is left as it was."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_llama_fp8_" + entry
    fn = getattr(lib, who)
    tree, cached = "tree" in entry, "cached" in entry
    NOF = object()

    def refused(match, desc, fp8=NOF, qkn=NOF, ids=(2, 5, 7, 9), off=(0, 1, 4), own=True, ws_bytes=1 << 30, scores=FAKE, cache=None):
        ids, off = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(off, np.int32)
        nl = desc.n_layers if desc is not None else 1
        f8 = _fp8(nl) if fp8 is NOF else fp8
        q = (_qkn(nl) if qwen3 else None) if qkn is NOF else qkn
        dp = C.byref(desc) if desc is not None else None
        fp = C.byref(f8) if f8 is not None else None
        if cached:
            cache = _cache() if cache is None else cache
            n0, ids0 = cache.n, cache._keep.copy()
            rc = fn(dp, q, fp, C.byref(cache), 1, ids.ctypes.data, off.ctypes.data, len(off) - 1, scores, None, None, None, FAKE,
                    ws_bytes, None)
            assert cache.n == n0 and (cache._keep == ids0).all()
        elif tree:
            rc = fn(dp, q, fp, ids.ctypes.data, off.ctypes.data, len(off) - 1, scores, None, None, FAKE, ws_bytes, None)
        else:
            rc = fn(dp, q, fp, ids.ctypes.data, off.ctypes.data, len(off) - 1, scores, None, FAKE, ws_bytes, None)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        assert N.last_error().startswith((who + ":") if own else "b2t_clm_llama"), N.last_error()

    # the unit's own
    refused("null fp8 descriptor", _packed_model(), fp8=None)
    refused("null layers_host in the fp8 descriptor", _packed_model(), fp8=_fp8(layers=False))
    for f, _ in N.ClmLlamaFp8Layer._fields_:
        refused("null pointer in layer 0 of the fp8 descriptor", _packed_model(), fp8=_fp8(**{f: 1}))
    refused("null pointer in layer 1 of the fp8 descriptor", _packed_model(n_layers=2), fp8=_fp8(2, down_s=2))
    refused("layer 0 of the model has qkv_w / o_w / gate_up_w / down_w beside the packed projections", _model(bias=False))
    for f in ("qkv_w", "o_w", "gate_up_w", "down_w"):
        both = _packed_model(n_layers=2)
        setattr(both.layers_host[1], f, FAKE)
        refused("layer 1 of the model has qkv_w / o_w / gate_up_w / down_w beside the packed projections", both)
    for bk in (0, -64, 32, 96, 100):                      # no multiple of 64
        refused(f"block_k {bk} must be a multiple of 64 that divides d_model 256 and ffn_dim 512", _packed_model(), fp8=_fp8(block_k=bk))
    refused("block_k 192 must be a multiple of 64 that divides d_model 256", _packed_model(), fp8=_fp8(block_k=192))
    refused("block_k 128 must be a multiple of 64 that divides d_model 256 and ffn_dim 320", _packed_model(ffn=320))
    refused("block_k 512 must be a multiple of 64", _packed_model(), fp8=_fp8(block_k=512))
    # the twins', as the twins word them
    refused("null model", None, own=False)
    refused("head dim 32", _packed_model(d=256, heads=8, kv=8), own=False)
    refused("multiple of n_kv_heads", _packed_model(d=512, heads=8, kv=3), own=False)
    refused("multiples of 64", _packed_model(d=256, heads=4, ffn=500), own=False)
    refused("bad dimensions", _packed_model(kv=0), own=False)
    refused("rms_eps", _packed_model(eps=-1.0), own=False)
    nonorm = _packed_model()
    nonorm.layers_host[0].norm2_w = None
    refused("null weight pointer in layer 0", nonorm, own=False)
    if qwen3:
        refused("null q / k norm weight in layer 0", _packed_model(), qkn=_qkn(1, k=None))
        refused("layer 0 has q / k / v biases", _packed_model(bias=True))
    # the lists' and the workspace's
    refused("null argument", _packed_model(), scores=None)
    refused("empty", _packed_model(), off=(0, 1, 1, 4))
    refused("outside", _packed_model(vocab=1000), ids=(2, 5, 1000, 9))
    refused("max_pos", _packed_model(max_pos=3), off=(0, 4), cache=_cache(cap=3) if cached else None)
    desc = _packed_model(bias=not qwen3)
    ids, off = (2, 5, 7, 2, 5, 8, 2, 5, 7), (0, 3, 6, 9)    # 9 tokens, 4 nodes
    p = C.byref(desc)
    need = (lib.b2t_clm_llama_tree_cached_ws_bytes(p, 4, 9, 3) if cached else lib.b2t_clm_llama_tree_ws_bytes(p, 4, 9, 3) if tree
            else lib.b2t_clm_llama_ws_bytes(p, 9, 3))
    assert need > 0
    refused("workspace of %d bytes, %d needed" % (need - 1, need), desc, ids=ids, off=off, ws_bytes=need - 1,
            cache=_cache(ids=()) if cached else None)
    if cached:
        refused("null cache member", desc, cache=_cache(kv=None))
        rc = fn(p, _qkn(1) if qwen3 else None, C.byref(_fp8()), None, 1, np.int32([2, 5]).ctypes.data, np.int32([0, 2]).ctypes.data, 1,
                FAKE, None, None, None, FAKE, 1 << 30, None)
        assert rc != 0 and re.search("null cache .*b2t_clm_llama_fp8_score_tree_f16", N.last_error())


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_unpack_refusals_before_device_work(fmt):
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_fp8_unpack_" + fmt
    fn = getattr(lib, who)
    for args, match in (((FAKE, FAKE, 4, 256, 96, FAKE, None), "block_k 96"), ((FAKE, FAKE, 4, 256, 0, FAKE, None), "block_k 0"),
                        ((FAKE, FAKE, 4, 320, 128, FAKE, None), "K 320"), ((FAKE, FAKE, 4, 0, 64, FAKE, None), "K 0"),
                        ((FAKE, FAKE, -1, 64, 64, FAKE, None), "rows -1"), ((None, FAKE, 4, 64, 64, FAKE, None), "null argument"),
                        ((FAKE, None, 4, 64, 64, FAKE, None), "null argument"), ((FAKE, FAKE, 4, 64, 64, None, None), "null argument"),
                        ((FAKE, FAKE, 1 << 40, 64, 64, FAKE, None), "too many")):
        assert fn(*args) != 0 and N.last_error().startswith(who + ":") and match in N.last_error(), (args, N.last_error())
    assert fn(None, None, 0, 64, 64, None, None) == 0            # no rows: nothing to do


def test_unit_uses_the_one_tile_rule_and_one_unpack():
    """The packed GEMMs go through causal_lm.hip's launch_gemm; the unit has no tile rule, no environment, no copy, no
    synchronisation and no atomics; the GEMM and the exported unpack call the one fp8_unpack8 of clm_gemm.h, which converts
    with the compiler's own round-to-nearest casts and no truncating pack."""
    import __graft_entry__ as G
    csrc = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")
    src = open(os.path.join(csrc, "causal_lm_llama_fp8.hip")).read()
    hdr = open(os.path.join(csrc, "clm_gemm.h")).read()
    assert "causal_lm_llama_fp8.hip" in G.HIP_SOURCES + G.HIP_SOURCES_FP8
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src
    assert len(re.findall(r"launch_gemm\(g, s, &clm_gemm_tiles<[^>]*, El, false, PK_FP8>\)", src)) == 3
    for word in ("hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc", "hipEventSynchronize", "atomicAdd",
                 "atomic_", "__atomic", "__hip_atomic"):
        assert word not in src, word
    assert src.count("fp8_unpack8<E>(") == 1 and hdr.count("fp8_unpack8<E>(") == 8 and "pkrtz" not in hdr and "pkrtz" not in src
