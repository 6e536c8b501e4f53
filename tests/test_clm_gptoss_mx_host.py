"""Host-side checks of gpt-oss with the experts kept in MXFP4 (csrc/causal_lm_gptoss_mx.hip, the packed form of the grouped tile in
csrc/clm_gemm.h, expert_weights="mxfp4" in llm_rescore; no GPU): gptoss_mx_device_layout against the dense loader as the
reference -- its packed arrays, dequantised and cast, are gate_up_w / down_w to the byte and every other array is identical --,
the refusals (the plain spelling, another family, a bad keyword, and the over-range and NaN-scale blocks that the dense loader
refuses, one planted at a time), the struct against the C compiler, the six new symbols' bindings, the descriptor refusals
before any device work, the bytes the experts take, and the kernels of the new unit with the resource figures of every causal-LM
unit against tests/golden/clm_kernel_resources.json, recorded before the packed tile was added to clm_gemm.h.

None of this exists without the feature: every test here fails on a tree that lacks the keyword, the layout and the symbols.

packed_state (shared with tests/test_gpu_clm_gptoss_mx.py) is a random gpt-oss state dict in the MXFP4 spelling whose blocks are
uniform random bytes and whose scale bytes are uniform in [110, 130] per block, so that neighbouring blocks of a row and of a k
tile differ: a neighbour's scale, a scale off by one or a swapped nibble moves the result."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_clm_gptoss_host import TINY, _oss, _wide, gptoss_config, mxfp4_state, random_state, ref_logp_gptoss
from test_clm_llama_host import FAKE, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden", "clm_kernel_resources.json")
HIPCC = "/opt/rocm/bin/hipcc"
SCORE = ("score_f16", "score_tree_f16", "score_bf16", "score_tree_bf16")
EXPERTS = ("gate_up_proj", "down_proj")
SCALE_LO, SCALE_HI = 110, 130


def packed_state(cfg, fmt="float16", seed=0, router_scale=0.125, device="cpu", lo=SCALE_LO, hi=SCALE_HI):
    """random_state(cfg, fmt, seed, ...) in the MXFP4 spelling: the expert matrices are replaced by gate_up_proj_blocks / _scales
    [E][2F][d / 32]([16]) and down_proj_blocks / _scales [E][d][F / 32]([16]) of uniform random bytes and scale bytes uniform in
    [lo, hi]; the largest value, 6 * 2^(130 - 127) = 48, is finite in either dtype."""
    import torch
    st = random_state(cfg, fmt, seed, router_scale, device=device)
    d, Fd, ne = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_local_experts"]
    g = torch.Generator(device=device).manual_seed(9100 + seed)
    for l in range(cfg["num_hidden_layers"]):
        for n, rows, K in (("gate_up_proj", 2 * Fd, d), ("down_proj", d, Fd)):
            k = f"model.layers.{l}.mlp.experts.{n}"
            del st[k]
            st[k + "_blocks"] = torch.randint(0, 256, (ne, rows, K // 32, 16), dtype=torch.uint8, generator=g, device=device)
            st[k + "_scales"] = torch.randint(lo, hi + 1, (ne, rows, K // 32), dtype=torch.uint8, generator=g, device=device)
    return st


def plain_of(st):
    """the plain spelling of a state dict in the MXFP4 spelling, fp32 (what HF's dequantisation makes of it)"""
    import llm_rescore as R
    out = {k: v for k, v in st.items() if not k.endswith(("_blocks", "_scales"))}
    for k in st:
        if k.endswith("_blocks"):
            n = k[:-len("_blocks")]
            out[n] = R.mxfp4_dequant(st[k], st[n + "_scales"]).transpose(1, 2).contiguous()
    return out


def save_checkpoint(path, cfg, st, dtype="bfloat16"):
    import torch
    from safetensors.torch import save_file
    os.makedirs(path)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg | {"dtype": dtype}, f)
    save_file({k: (v if v.dtype == torch.uint8 else v.to(getattr(torch, dtype))).cpu().contiguous() for k, v in st.items()},
              os.path.join(path, "model.safetensors"))


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16) if t.element_size() == 2 else t


def expert_bytes(dims):
    """the derived number: E (gus (d / 2 + d / 32) + dns (F / 2 + F / 32)) a layer"""
    import llm_rescore as R
    gus, dns = R.mixtral_strides(dims)
    d, Fd = dims["d_model"], dims["ffn_dim"]
    return dims["n_experts"] * (gus * (d // 2 + d // 32) + dns * (Fd // 2 + Fd // 32))


# ---- the layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
@pytest.mark.parametrize("which", ["representable", "varied scales"])
def test_layout_against_the_dense_loader(fmt, which):
    """The tiny MXFP4 checkpoint (mxfp4_state's, and packed_state's with scale bytes that vary by block): the packed arrays put
    through mxfp4_dequant(...).to(dtype) are the dense loader's gate_up_w and down_w byte for byte, row permutation and zero
    padding included; every other array is identical; the experts take the derived number of bytes, and no array was expanded."""
    import torch
    import llm_rescore as R
    cfg = gptoss_config()[1]
    st = mxfp4_state(random_state(cfg, fmt))[1] if which == "representable" else packed_state(cfg, fmt, seed=3)
    dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
    dense, mx = R.gptoss_device_layout(st, dims, rope, dtype=fmt), R.gptoss_mx_device_layout(st, dims, rope, dtype=fmt)
    wdt = R.clm_dtype(fmt)
    packed = {k for k in mx if k.endswith(("_q", "_s"))}
    assert sorted(set(mx) - packed) == sorted(k for k in dense if not k.endswith(("gate_up_w", "down_w")))
    assert [k.split(".")[-1] for k in mx if k.startswith("layers.0.")] == list(R._GPTOSS_MX_ORDER)
    for k in set(mx) - packed:
        assert mx[k].dtype == dense[k].dtype and torch.equal(_bits(mx[k]), _bits(dense[k])), k
    gus, dns = R.mixtral_strides(dims)
    ne, d, Fd = dims["n_experts"], dims["d_model"], dims["ffn_dim"]
    assert (d, Fd) == (TINY["hidden_size"], TINY["intermediate_size"]) and (gus, dns) == (256, 256) and 2 * Fd < gus and d < dns   # padded
    for l in range(dims["n_layers"]):
        held = 0
        for n, rows, K in (("gate_up", gus, d), ("down", dns, Fd)):
            q, s = mx[f"layers.{l}.{n}_q"], mx[f"layers.{l}.{n}_s"]
            assert q.dtype == s.dtype == torch.uint8 and tuple(q.shape) == (ne, rows, K // 2) and tuple(s.shape) == (ne, rows, K // 32)
            w = R.mxfp4_dequant(q.reshape(ne, rows, K // 32, 16), s).to(wdt)
            assert torch.equal(_bits(w), _bits(dense[f"layers.{l}.{n}_w"])), (l, n)
            held += q.numel() + s.numel()
        assert held == expert_bytes(dims) == 8 * (256 * (96 + 6) + 256 * (32 + 2))
        assert not (mx[f"layers.{l}.gate_up_q"][:, 2 * Fd:] != 0).any() and not (mx[f"layers.{l}.down_s"][:, d:] != 0).any()
    assert (dense["layers.0.gate_up_w"] != 0).any()


def test_scorer_holds_packed_experts_only(tmp_path):
    """build_scorer(..., expert_weights="mxfp4") on a saved checkpoint, on the CPU: a GptOssMxScorer whose w holds the uint8
    arrays of the derived size and no dense expert matrix, whose model descriptor has NULL gate_up_w / down_w and whose mx array
    points at them; the default is "dense", today's scorer; the context cache stays refused."""
    import inspect
    import torch
    import b2t_native as N
    import llm_rescore as R
    cfg = gptoss_config()[1]
    save_checkpoint(str(tmp_path / "mx"), cfg, packed_state(cfg, "bfloat16", seed=1))
    for fn in (R.build_scorer, R.build_opt):
        par = inspect.signature(fn).parameters
        assert list(par)[-2:] == ["expert_weights", "dtype"] and par["expert_weights"].default == "dense"
        assert par["expert_weights"].kind is inspect.Parameter.KEYWORD_ONLY
    assert R.EXPERT_WEIGHTS == ("dense", "mxfp4")
    for dt, want in ((None, torch.float16), ("bfloat16", torch.bfloat16), ("auto", torch.bfloat16)):
        sc = R.build_scorer(str(tmp_path / "mx"), device="cpu", dtype=dt, expert_weights="mxfp4")
        assert type(sc) is R.GptOssMxScorer and isinstance(sc, R.GptOssScorer) and sc.dtype is want
        assert sc._family == "gptoss_mx" and sc._SIZES == "b2t_clm_gptoss_" and sc._size_args == (sc._oss,) and sc._qk == (sc._oss, sc._mx)
        assert isinstance(sc._mx, C.Array) and sc._mx._type_ is N.ClmGptOssMx and len(sc._mx) == 2
        assert not [k for k in sc.w if k.endswith(("gate_up_w", "down_w"))]
        held = [v for k, v in sc.w.items() if k.endswith(("_q", "_s"))]
        assert len(held) == 8 and all(v.dtype is torch.uint8 for v in held)
        assert sum(v.numel() for v in held) == sc.expert_bytes() == 2 * expert_bytes(sc.dims)
        for l in range(2):
            assert not sc.desc.layers_host[l].gate_up_w and not sc.desc.layers_host[l].down_w
            for f in R._GPTOSS_MX_FIELDS:
                assert getattr(sc._mx[l], f) == sc.w[f"layers.{l}.{f}"].data_ptr()
            assert sc._oss.layers_host[l].gate_up_b == sc.w[f"layers.{l}.gate_up_b"].data_ptr()
        assert sc.score([]).shape == (0,)
    dense = R.build_scorer(str(tmp_path / "mx"), device="cpu")
    assert type(dense) is R.GptOssScorer and "layers.0.gate_up_w" in dense.w and type(
        R.build_scorer(str(tmp_path / "mx"), device="cpu", expert_weights="dense")) is R.GptOssScorer
    with pytest.raises(ValueError, match="context cache"):
        R.build_scorer(str(tmp_path / "mx"), device="cpu", context_cache_tokens=64, expert_weights="mxfp4")
    dims, arr = R.load_gptoss_arrays(str(tmp_path / "mx"), dtype="bfloat16", expert_weights="mxfp4")
    assert "layers.1.down_q" in arr and "layers.1.down_w" not in arr
    with pytest.raises(KeyError, match="gate_up_q"):
        R.GptOssMxScorer(dims, R.load_gptoss_arrays(str(tmp_path / "mx"), dtype="bfloat16")[1], "cpu", dtype="bfloat16")
    with pytest.raises(ValueError, match="layers.0.gate_up_s is torch.int32, expected torch.uint8"):
        R.GptOssMxScorer(dims, dict(arr, **{"layers.0.gate_up_s": arr["layers.0.gate_up_s"].int()}), "cpu", dtype="bfloat16")


# ---- the refusals ----------------------------------------------------------------------------------------------------------------
def test_keyword_refusals(tmp_path):
    """"mxfp4" on the plain spelling names the _blocks tensor it lacks; on another family (a bare Llama config.json: no weight is
    looked for) and with a bad value the keyword itself is refused."""
    import llm_rescore as R
    cfg = gptoss_config()[1]
    st = random_state(cfg, "bfloat16")
    save_checkpoint(str(tmp_path / "plain"), cfg, st)
    with pytest.raises(ValueError, match=r"lacks model\.layers\.0\.mlp\.experts\.gate_up_proj_blocks"):
        R.build_scorer(str(tmp_path / "plain"), device="cpu", expert_weights="mxfp4")
    half = dict(mxfp4_state(st)[1])
    del half["model.layers.1.mlp.experts.down_proj_blocks"]
    with pytest.raises(ValueError, match=r"lacks model\.layers\.1\.mlp\.experts\.down_proj_blocks"):
        R.gptoss_mx_device_layout(half, R.gptoss_dims(cfg), R.gptoss_rope(cfg))
    assert type(R.build_scorer(str(tmp_path / "plain"), device="cpu")) is R.GptOssScorer
    os.makedirs(tmp_path / "llama")
    with open(tmp_path / "llama" / "config.json", "w") as f:
        json.dump({"model_type": "llama", "hidden_size": 256, "num_attention_heads": 4, "num_hidden_layers": 2}, f)
    with pytest.raises(ValueError, match=r"expert_weights='mxfp4' is for gpt_oss checkpoints.*'llama'"):
        R.build_scorer(str(tmp_path / "llama"), device="cpu", expert_weights="mxfp4")
    for bad in ("fp4", "MXFP4", None, ""):
        for sub in ("plain", "llama"):
            with pytest.raises(ValueError, match="expert_weights .* is not one of"):
                R.build_scorer(str(tmp_path / sub), device="cpu", expert_weights=bad)


PLANTED = [   # (tensor, (expert, row, block), scale byte, largest nibble code): one block at a time
    ("down_proj", (0, 0, 0), 127 + 16, 7),        # 6 * 2^16: over range in fp16, not in bf16
    ("down_proj", (7, 191, 1), 127 + 16, 1),      # 0.5 * 2^16 = 32768: finite in both
    ("gate_up_proj", (3, 127, 5), 127 + 15, 3),   # 1.5 * 2^15 = 49152: the largest fp16 value these blocks can hold
    ("gate_up_proj", (3, 127, 5), 127 + 15, 4),   # 2 * 2^15 = 65536: over range in fp16
    ("gate_up_proj", (1, 2, 3), 127 + 14, 7),     # 6 * 2^14 = 98304: over range in fp16
    ("gate_up_proj", (1, 2, 3), 127 + 13, 7),     # 6 * 2^13 = 49152
    ("down_proj", (2, 5, 0), 254, 7),             # 6 * 2^127: over range in bf16 (and in fp32)
    ("down_proj", (2, 5, 0), 252, 7),             # 6 * 2^125 = 1.5 * 2^127: finite in bf16
    ("down_proj", (2, 5, 0), 253, 5),             # 3 * 2^126 = 1.5 * 2^127: finite in bf16
    ("down_proj", (2, 5, 0), 253, 6),             # 4 * 2^126 = 2^128: over range in bf16
    ("gate_up_proj", (0, 0, 0), 255, 7),          # a NaN scale
    ("gate_up_proj", (5, 64, 2), 255, 0),         # a NaN scale over a block of zeros: 0 * 2^128 is still no number
    ("down_proj", (4, 100, 1), 200, 0),           # a huge scale over a block of zeros: zeros, accepted
    ("down_proj", (4, 100, 1), 0, 7),             # the smallest scale: zeros in fp16, bf16 subnormals, accepted
]


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_blocks_refused_as_the_dense_loader_refuses_them(fmt):
    """The dense loader on the same checkpoint is the reference for whether a planted block is refused, and with which message
    and tensor name; the packed loader decides it per block without expanding (mxfp4_block_finite).  Of the planted blocks some
    are refused in fp16 alone, some in both, some in neither."""
    import torch
    import llm_rescore as R
    cfg = gptoss_config()[1]
    base = packed_state(cfg, fmt, seed=2)
    dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
    refused = []
    for layer, (n, at, scale, code) in enumerate(PLANTED):
        k = f"model.layers.{layer % 2}.mlp.experts.{n}"
        blocks, scales = base[k + "_blocks"].clone(), base[k + "_scales"].clone()
        blocks[at] = 0
        blocks[at][5] = code << 4 | 8                 # the largest magnitude in a high nibble, beside a -0
        if code:
            blocks[at][11] = (code - 1) | 0x80         # a smaller one, negative, in a low nibble
        scales[at] = scale
        st = dict(base, **{k + "_blocks": blocks, k + "_scales": scales})
        outcome = []
        for layout in (R.gptoss_device_layout, R.gptoss_mx_device_layout):
            try:
                layout(st, dims, rope, dtype=fmt)
                outcome.append(None)
            except ValueError as e:
                outcome.append(str(e))
        assert outcome[0] == outcome[1], (n, at, scale, code, outcome)
        assert outcome[0] is None or (k + "_blocks / _scales: a value is not finite in torch." + fmt) == outcome[0]
        refused.append(outcome[0] is not None)
        fin = R.mxfp4_block_finite(blocks, scales, R.clm_dtype(fmt))
        assert fin.shape == scales.shape and bool(fin[at]) == (outcome[0] is None) and int((~fin).sum()) == int(not fin[at])
    want = {"float16": [1, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 0, 0], "bfloat16": [0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 0]}[fmt]
    assert refused == [bool(x) for x in want]
    with pytest.raises(ValueError, match="gate_up_proj_blocks / _scales: shapes"):
        k = "model.layers.0.mlp.experts.gate_up_proj_blocks"
        R.gptoss_mx_device_layout(dict(base, **{k: base[k][:, :100]}), dims, rope, dtype=fmt)
    with pytest.raises(ValueError, match="must be uint8"):
        k = "model.layers.1.mlp.experts.down_proj_scales"
        R.gptoss_mx_device_layout(dict(base, **{k: base[k].int()}), dims, rope, dtype=fmt)


@pytest.mark.parametrize("fmt", ["float16", "bfloat16"])
def test_varied_scales_leave_the_reference_finite(fmt):
    """The precondition of the GPU tests' byte comparisons: with scale bytes in [110, 130] the restatement of the contract
    (ref_logp_gptoss on the dequantised plain spelling, rounded as the kernels round) keeps every log-prob finite for the seeds
    those tests use, so a NaN in the kernels' output is the kernels'."""
    import llm_rescore as R
    cfg = gptoss_config(sliding_window=40)[1]
    dims, rope = R.gptoss_dims(cfg), R.gptoss_rope(cfg)
    seqs = tiny_seqs(cfg["vocab_size"], seed=1, lens=(1, 17, 64, 65, 100))
    for seed in (0, 1):
        st = packed_state(cfg, fmt, seed=seed)
        s = st["model.layers.0.mlp.experts.gate_up_proj_scales"]
        assert int(s.min()) == SCALE_LO and int(s.max()) == SCALE_HI and (s[:, :, 1:] != s[:, :, :-1]).float().mean() > 0.9
        logp = ref_logp_gptoss(plain_of(st), dims, rope, seqs, fmt)[0]
        assert all(np.isfinite(t).all() for t in logp) and min(t.min() for t in logp) < -1.0


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs a C compiler")
def test_symbols_struct_and_bindings(tmp_path):
    """The six new symbols are declared (the four score calls in parentheses, which header_symbols reads), exported and bound with
    the gpt-oss twins' lists plus the mx array; b2t_clm_gptoss_mx_t has the C compiler's layout; the header compiles as C."""
    import b2t_native as N
    lib = N.load()
    names = ["b2t_clm_gptoss_mx_" + t for t in SCORE] + ["b2t_clm_mxfp4_unpack_f16", "b2t_clm_mxfp4_unpack_bf16"]
    assert set(names) <= set(N.header_symbols()) and "b2t_bucket_cb" not in N.header_symbols()
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "b2t.h")).read())
    for t in SCORE:
        new, twin = "b2t_clm_gptoss_mx_" + t, "b2t_clm_gptoss_" + t
        f, g = getattr(lib, new), getattr(lib, twin)
        assert f.restype == g.restype and list(f.argtypes) == list(g.argtypes[:2]) + [C.POINTER(N.ClmGptOssMx)] + list(g.argtypes[2:])
        args = lambda pat: [a.strip() for a in re.search(pat + r"\((.*?)\);", hdr).group(1).split(",")]
        want = args(r"int " + twin)
        assert args(r"int \(" + new + r"\)") == want[:2] + ["const b2t_clm_gptoss_mx_t* mx"] + want[2:]
    for t in ("f16", "bf16"):
        f = getattr(lib, "b2t_clm_mxfp4_unpack_" + t)
        assert f.restype is C.c_int and list(f.argtypes) == [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
        assert f"int b2t_clm_mxfp4_unpack_{t}(const void* q, const void* s, long long rows, int K, void* out, void* stream);" in hdr
    body = 'printf("D %zu\\n", sizeof(b2t_clm_gptoss_mx_t));' + "".join(
        f'printf("{f} %zu\\n", offsetof(b2t_clm_gptoss_mx_t, {f}));' for f, _ in N.ClmGptOssMx._fields_)
    body += "int (*fn)(const b2t_clm_llama_t*, const b2t_clm_gptoss_t*, const b2t_clm_gptoss_mx_t*, const int32_t*, const int32_t*, int, " \
            "float*, float*, void*, size_t, void*) = b2t_clm_gptoss_mx_score_bf16; (void)fn;"
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "b2t.h"\nint main(void){' + body + "return 0;}")
    cc = "/opt/rocm/lib/llvm/bin/clang" if os.path.exists("/opt/rocm/lib/llvm/bin/clang") else "cc"
    subprocess.check_call([cc, "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "lay.o")])
    lay = re.sub(r"b2t_clm_gptoss_mx_score_bf16; \(void\)fn;", "0; (void)fn;", src.read_text())
    src.write_text(lay)
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "lay")])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / "lay")], text=True).splitlines())
    assert int(got["D"]) == C.sizeof(N.ClmGptOssMx) == 32 and [f for f, _ in N.ClmGptOssMx._fields_] == list(_fields())
    for f, _ in N.ClmGptOssMx._fields_:
        assert int(got[f]) == getattr(N.ClmGptOssMx, f).offset, f


def _fields():
    import llm_rescore as R
    return R._GPTOSS_MX_FIELDS


def _mx(n_layers=1, **null):
    import b2t_native as N
    arr = (N.ClmGptOssMx * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmGptOssMx._fields_:
            setattr(arr[i], f, None if null.get(f) else FAKE)
    return arr


def _packed_model(**kw):
    """_wide's descriptor as a caller of the mx calls holds it: no dense experts"""
    desc = _wide(**kw)
    for i in range(desc.n_layers):
        desc.layers_host[i].gate_up_w = None
        desc.layers_host[i].down_w = None
    return desc


@pytest.mark.parametrize("entry", SCORE)
def test_refusals_before_device_work(entry):
    """With fake pointers and no GPU: a null mx, a null pointer inside it and a model that holds dense experts as well are
    refused under the call's own name; what the gpt-oss twin refuses of the descriptors and of the lists is refused as the twin
    refuses it; the workspace is the twin's size function's."""
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_gptoss_mx_" + entry
    fn = getattr(lib, who)
    tree = "tree" in entry
    NOM = object()

    def refused(match, desc, oss=NOM, mx=NOM, ids=(2, 5, 7, 9), off=(0, 1, 4), own=True, ws_bytes=1 << 30, scores=FAKE):
        ids, off = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(off, np.int32)
        q = _oss(desc.n_layers if desc is not None else 1) if oss is NOM else oss
        m = _mx(desc.n_layers if desc is not None else 1) if mx is NOM else mx
        dp = C.byref(desc) if desc is not None else None
        tail = (None, FAKE, ws_bytes, None) if tree else (FAKE, ws_bytes, None)
        rc = fn(dp, q, m, ids.ctypes.data, off.ctypes.data, len(off) - 1, scores, None, *tail)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        assert N.last_error().startswith((who + ":") if own else "b2t_clm_gptoss:"), N.last_error()

    refused("null mx descriptor", _packed_model(), mx=None)
    for f in _fields():
        refused("null pointer in layer 0 of mx", _packed_model(), mx=_mx(**{f: True}))
    short = _mx(2)
    short[1].down_s = None
    refused("null pointer in layer 1 of mx", _packed_model(n_layers=2), mx=short)
    refused("layer 0 of the model has gate_up_w / down_w beside the packed experts", _wide())
    for f in ("gate_up_w", "down_w"):
        both = _packed_model(n_layers=2)
        setattr(both.layers_host[1], f, FAKE)
        refused("layer 1 of the model has gate_up_w / down_w beside the packed experts", both)
    # the twin's, as the twin words them
    refused("null model", None, own=False)
    refused("null gptoss descriptor", _packed_model(), oss=None, own=False)
    refused("head dim 128", _packed_model(), oss=_oss(hd=128), own=False)
    refused("multiples of 64", _packed_model(ffn=500), own=False)
    refused("n_experts 129 outside", _packed_model(), oss=_oss(ne=129), own=False)
    refused("expert strides 768 / 256", _packed_model(), oss=_oss(gus=768), own=False)
    refused("null weight pointer in layer 0", _packed_model(), oss=_oss(down_b=True), own=False)
    nonorm = _packed_model()
    nonorm.layers_host[0].norm2_w = None
    refused("null weight pointer in layer 0", nonorm, own=False)
    refused("layer 0 has no q / k / v biases", _packed_model(bias=False), own=False)
    refused("null argument", _packed_model(), scores=None)
    refused("empty", _packed_model(), off=(0, 1, 1, 4))
    refused("outside", _packed_model(vocab=1000), ids=(2, 5, 1000, 9))
    refused("max_pos", _packed_model(max_pos=3), off=(0, 4))
    desc, oss = _packed_model(), _oss()
    ids, off = (2, 5, 7, 2, 5, 8, 2, 5, 7), (0, 3, 6, 9)    # 9 tokens, 4 nodes
    p, q = C.byref(desc), C.byref(oss)
    need = lib.b2t_clm_gptoss_tree_ws_bytes(p, q, 4, 9, 3) if tree else lib.b2t_clm_gptoss_ws_bytes(p, q, 9, 3)
    assert need > 0
    refused("workspace of %d bytes, %d needed" % (need - 1, need), desc, oss, ids=ids, off=off, ws_bytes=need - 1)


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_unpack_refusals_before_device_work(fmt):
    import b2t_native as N
    lib = N.load()
    who = "b2t_clm_mxfp4_unpack_" + fmt
    fn = getattr(lib, who)
    for args, match in (((FAKE, FAKE, 4, 48, FAKE, None), "K 48"), ((FAKE, FAKE, 4, 0, FAKE, None), "K 0"),
                        ((FAKE, FAKE, -1, 64, FAKE, None), "rows -1"), ((None, FAKE, 4, 64, FAKE, None), "null argument"),
                        ((FAKE, None, 4, 64, FAKE, None), "null argument"), ((FAKE, FAKE, 4, 64, None, None), "null argument"),
                        ((FAKE, FAKE, 1 << 40, 64, FAKE, None), "too many")):
        assert fn(*args) != 0 and N.last_error().startswith(who + ":") and match in N.last_error(), (args, N.last_error())
    assert fn(None, None, 0, 64, None, None) == 0            # no rows: nothing to do


# ---- the kernels -----------------------------------------------------------------------------------------------------------------
FIGURES = ("VGPRs", "AGPRs", "LDS", "ScratchSize")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_kernels_of_the_unit_and_of_every_other_unit():
    """causal_lm_gptoss_mx.hip instantiates the packed grouped GEMM with EP_OSS_GLU (14) and EP_F32_BIAS (15) on two tiles and in two
    element types, the router, the gather, the flat and the tree attention with sink and window and the unpack kernel in two
    element types, the plan and combine kernels once, and nothing else: 20 kernels, none of them a dense GEMM, ScratchSize 0.
    The packed tile is a trailing template parameter of the one tile, so every other causal-LM unit must compile to the kernels
    it had, by name, with the registers, LDS and scratch it had: tests/golden/clm_kernel_resources.json, recorded before."""
    from concurrent.futures import ThreadPoolExecutor
    import __graft_entry__ as G
    import wave_kernel_resources as W
    assert "causal_lm_gptoss_mx.hip" in G.HIP_SOURCES
    with open(GOLD) as f:
        gold = json.load(f)
    units = sorted(s for s in G.HIP_SOURCES if s.startswith("causal_lm"))
    assert sorted(gold) == [u for u in units if u != "causal_lm_gptoss_mx.hip"] and len(gold) == 13
    with ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        dump = dict(zip(units, ex.map(lambda u: W.resources(src=u), units)))
    res = {k: v for k, v in dump["causal_lm_gptoss_mx.hip"].items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_grouped_mx_kernel" in k]
    assert len(res) == 20 and len(gemm) == 8 and not [k for k in res if "clm_gemm_kernel" in k or "clm_gemm_grouped_kernel" in k], sorted(res)
    assert sum("ELi14E" in k for k in gemm) == 4 and sum("ELi15E" in k for k in gemm) == 4
    assert sum("ILi256ELi256E" in k for k in gemm) == 4 and sum("ILi128ELi128E" in k for k in gemm) == 4
    assert sum("DF16_E" in k for k in gemm) == 4 and sum("DF16bE" in k for k in gemm) == 4
    for kern, n in (("clm_gptoss_route_kernel", 2), ("clm_moe_gather_kernel", 2), ("clm_moe_plan_kernel", 1), ("clm_moe_combine_kernel", 1),
                    ("clm_attn_sink_kernelILi64E", 2), ("clm_attn_tree_sink_kernelILi64E", 2), ("clm_mxfp4_unpack_kernel", 2)):
        assert sum(kern in k for k in res) == n, (kern, sorted(res))
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res
    for u, want in gold.items():
        got = {k: {f: v.get(f) for f in FIGURES} for k, v in dump[u].items()}
        assert got == want, (u, {k: (want.get(k), got.get(k)) for k in set(want) | set(got) if want.get(k) != got.get(k)})


def test_unit_uses_the_one_tile_rule_and_one_unpack():
    """Both packed GEMMs go through causal_lm.hip's launch_gemm; the unit has no tile rule, no environment, no copy, no
    synchronisation and no atomics; the GEMM and the exported unpack call the one mxfp4_unpack8 of clm_gemm.h."""
    csrc = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")
    src = open(os.path.join(csrc, "causal_lm_gptoss_mx.hip")).read()
    hdr = open(os.path.join(csrc, "clm_gemm.h")).read()
    assert "B2T_CLM_GEMM_256" not in src.split("#include")[1] and "getenv" not in src
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_OSS_GLU, El, true, true>)") == 1
    assert src.count("launch_gemm(g, s, &clm_gemm_tiles<EP_F32_BIAS, El, true, true>)") == 1
    for word in ("hipMemcpy", "hipStreamSynchronize", "hipDeviceSynchronize", "hipMalloc", "hipEventSynchronize", "atomicAdd",
                 "atomic_", "__atomic", "__hip_atomic"):
        assert word not in src, word
    assert src.count("mxfp4_unpack8<E>(") == 1 and hdr.count("mxfp4_unpack8<E>(") == 8 and "mxfp4_unpack8" not in open(
        os.path.join(csrc, "clm_gptoss.h")).read()
    assert len(re.findall(r"\nint \(?b2t_clm_gptoss_mx_\w+\)?\(", open(os.path.join(ROOT, "include", "b2t.h")).read())) == 4
