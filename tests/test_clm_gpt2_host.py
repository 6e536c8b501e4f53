"""Host-side checks of the GPT-2 rescorer (csrc/causal_lm_gpt2.hip, llm_rescore.Gpt2Scorer; no GPU): the loader's device layout
against the state dict under the inverse transform, its refusals, the float64 restatement of the forward (ref_logp_gpt2, the
reference of tests/test_gpu_clm_gpt2.py) against the HF fp32 models, the refusals of the three entry points before any device
work, the symbols, sizes and struct layouts, the two kernels' resources and the Python surface.

The tiny models (TINY) are random HF GPT2LMHeadModel instances built in memory, no download: two layers, n_positions 128, head
dims 64, 80 and 128, vocabularies that are no multiple of 64, with the weight recipe of tests/test_clm_llama_host.py."""
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
from test_clm_host import FAKE, _model
from test_clm_llama_host import hf_logp, tiny_seqs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc")

TINY = {
    "hd64": dict(n_embd=128, n_head=2, vocab_size=503),
    "hd80": dict(n_embd=320, n_head=4, vocab_size=777),
    "hd128": dict(n_embd=256, n_head=2, vocab_size=1003),
}
ENTRY = ("b2t_clm_gpt2_score_f16", "b2t_clm_gpt2_score_tree_f16", "b2t_clm_gpt2_score_tree_cached_f16")
# max |dlogp| of the unrounded float64 restatement against the HF fp32 CPU model over tiny_seqs (lengths 1 .. 100, log-probs
# down to -15), measured here; the test asserts at 10 x
HF_MEASURED = {"hd64": 2.6e-6, "hd80": 6.6e-6, "hd128": 3.9e-6}


def tiny_gpt2(name, n_layers=2, **over):
    """(HF fp32 CPU GPT2LMHeadModel in eval mode with fp16-representable random weights, its config as config.json's dict)."""
    import torch
    import transformers
    kw = dict(TINY[name], **over)
    cfg = transformers.GPT2Config(n_layer=n_layers, n_positions=128, attn_implementation="eager", bos_token_id=2, eos_token_id=2,
                                  attn_pdrop=0.0, embd_pdrop=0.0, resid_pdrop=0.0, **kw)
    torch.manual_seed(sorted(TINY).index(name))
    model = transformers.GPT2LMHeadModel(cfg).float().eval()
    d = cfg.n_embd
    g = torch.Generator().manual_seed(300 + sorted(TINY).index(name))
    with torch.no_grad():
        for k, p in model.named_parameters():
            if re.search(r"ln_(1|2|f)\.weight$", k):
                v = 1 + 0.2 * torch.randn(p.shape, generator=g)
            elif k.endswith(".bias"):
                v = 0.3 * torch.randn(p.shape, generator=g)
            elif "wte" in k or "lm_head" in k:
                v = torch.randn(p.shape, generator=g) * 2.0 / d ** 0.5      # logits with a spread of about 2
            elif "wpe" in k:
                v = torch.randn(p.shape, generator=g) / d ** 0.5
            else:
                v = torch.randn(p.shape, generator=g) / p.shape[0] ** 0.5    # Conv1D [in][out]: the fan-in is shape[0]
            p.copy_(v.half().float())
    assert model.lm_head.weight is model.transformer.wte.weight
    return model, json.loads(cfg.to_json_string())


def gpt2_state(model):
    return {k: v.detach() for k, v in model.state_dict().items()}


def gelu_new(v):
    import torch
    return 0.5 * v * (1 + torch.tanh((2 / np.pi) ** 0.5 * (v + 0.044715 * v ** 3)))


def ref_logp_gpt2(st, dims, seqs, rounded=True, act=gelu_new):
    """The forward restated in float64 from a state dict under HF's names (Conv1D weights [in][out], nothing transposed or
    split); per sequence the log-probs (0 at the first token).  rounded=True rounds to fp16 exactly where the contract of
    csrc/causal_lm_gpt2.hip says the kernels round, and nowhere else: the LayerNorm outputs; q after its bias and the factor
    head_dim^-0.5 (once); k; v; the attention's probabilities per 32-key block relative to the running maximum (the kernel's
    P.V operand; the normaliser sums them unrounded) and its output; gelu_new(fc1).  rounded=False rounds nowhere.  `act`
    replaces the activation (the planted differences of the GPU tests)."""
    import torch
    F = torch.nn.functional
    W = lambda k: st["transformer." + k].double()
    r16 = (lambda t: t.half().double()) if rounded else (lambda t: t)
    d, H, nl, V = dims["d_model"], dims["n_heads"], dims["n_layers"], dims["vocab"]
    hd = d // H
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["transformer.wte.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    ln = lambda t, p: F.layer_norm(t, (d,), W(p + ".weight"), W(p + ".bias"), 1e-5)
    conv = lambda t, p: t @ W(p + ".weight") + W(p + ".bias")
    x = W("wte.weight")[ids] + W("wpe.weight")[pos]
    M = x.shape[0]
    for l in range(nl):
        p = f"h.{l}."
        h = r16(ln(x, p + "ln_1"))
        q, k, v = conv(h, p + "attn.c_attn").split(d, -1)
        q, k, v = r16(q * hd ** -0.5).view(M, H, hd), r16(k).view(M, H, hd), r16(v).view(M, H, hd)
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
        x = x + conv(r16(o), p + "attn.c_proj")
        h = r16(ln(x, p + "ln_2"))
        x = x + conv(r16(act(conv(h, p + "mlp.c_fc"))), p + "mlp.c_proj")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = r16(ln(x[src], "ln_f"))
    E = st["transformer.wte.weight"]
    chunk = max(64, (1 << 27) // h.shape[0])
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


# ---- the loader --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_loader_layout_is_the_state_dict_under_the_inverse_transform(name, tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_gpt2(name)
    model.save_pretrained(str(tmp_path))
    assert cfg["n_inner"] is None and cfg["activation_function"] == "gelu_new"
    dims, arr = R.load_gpt2_arrays(str(tmp_path))
    d, H, V = cfg["n_embd"], cfg["n_head"], cfg["vocab_size"]
    assert dims == dict(n_layers=2, d_model=d, n_heads=H, ffn_dim=4 * d, vocab=V, max_pos=128)
    sd = model.state_dict()
    eq = lambda a, b: torch.equal(a, b.half())
    rup = lambda n: -(-n // 256) * 256

    def check(arr):
        assert arr["embed_tokens"].shape == (rup(V), d) and eq(arr["embed_tokens"][:V], sd["transformer.wte.weight"])
        assert not arr["embed_tokens"][V:].any()
        ep = arr["embed_positions"]
        assert ep.shape == (130, d) and not ep[:2].any() and eq(ep[2:], sd["transformer.wpe.weight"])
        assert eq(arr["final_ln_w"], sd["transformer.ln_f.weight"]) and eq(arr["final_ln_b"], sd["transformer.ln_f.bias"])
        for l in range(2):
            p, a = f"transformer.h.{l}.", lambda f: arr[f"layers.{l}.{f}"]
            for ours, theirs in (("ln1", "ln_1"), ("ln2", "ln_2")):
                assert eq(a(ours + "_w"), sd[p + theirs + ".weight"]) and eq(a(ours + "_b"), sd[p + theirs + ".bias"])
            for ours, theirs, n_in, n_out in (("qkv", "attn.c_attn", d, 3 * d), ("out", "attn.c_proj", d, d),
                                              ("fc1", "mlp.c_fc", d, 4 * d), ("fc2", "mlp.c_proj", 4 * d, d)):
                w, b = a(ours + "_w"), a(ours + "_b")
                assert w.shape == (rup(n_out), n_in) and not w[n_out:].any(), ours
                assert eq(w[:n_out].t(), sd[p + theirs + ".weight"]), ours          # transposed back: Conv1D's [in][out]
                assert b.shape == (n_out,) and eq(b, sd[p + theirs + ".bias"]), ours
            # rows q | k | v: what HF's split of c_attn's output columns gives
            qw, kw, vw = sd[p + "attn.c_attn.weight"].split(d, 1)
            w = a("qkv_w")
            assert eq(w[:d], qw.t()) and eq(w[d:2 * d], kw.t()) and eq(w[2 * d:3 * d], vw.t())
        assert all(t.is_contiguous() and t.dtype == torch.float16 for t in arr.values())
        assert len(arr) == 4 + 2 * 12

    check(arr)
    # keys without the 'transformer.' prefix, and the attn.bias / attn.masked_bias buffers of old checkpoints
    bare = {k[len("transformer."):] if k.startswith("transformer.") else k: v for k, v in sd.items()}
    bare["h.0.attn.bias"] = torch.ones(1, 1, 128, 128)
    bare["h.1.attn.masked_bias"] = torch.tensor(-1e4)
    check(R.gpt2_device_layout(bare, dims))
    old = dict(sd)
    old["transformer.h.0.attn.bias"] = torch.ones(1, 1, 128, 128)
    old["transformer.h.0.attn.masked_bias"] = torch.tensor(-1e4)
    check(R.gpt2_device_layout(old, dims))
    # fp32 values that fp16 does not hold are rounded once
    odd = dict(sd)
    odd["transformer.ln_f.weight"] = sd["transformer.ln_f.weight"] + 1e-4
    assert torch.equal(R.gpt2_device_layout(odd, dims)["final_ln_w"], odd["transformer.ln_f.weight"].half())


def test_loader_refusals():
    import torch
    import llm_rescore as R
    model, cfg = tiny_gpt2("hd64", n_layers=1)
    dims = R.gpt2_dims(cfg)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            R.gpt2_dims(cfg | kw)
    refused(r"activation_function 'gelu'.*erf.*not built", activation_function="gelu")
    refused("activation_function 'relu'", activation_function="relu")
    refused("activation_function 'gelu_fast'", activation_function="gelu_fast")
    refused("scale_attn_weights", scale_attn_weights=False)
    refused("scale_attn_by_inverse_layer_idx", scale_attn_by_inverse_layer_idx=True)
    refused("add_cross_attention", add_cross_attention=True)
    refused("layer_norm_epsilon", layer_norm_epsilon=1e-6)
    refused("head dim", n_head=4)                      # head dim 32
    refused("head dim", n_embd=192, n_head=2)          # head dim 96
    refused("head dim", n_embd=128, n_head=3)          # not a divisor
    refused("multiples of 64", n_embd=160, n_head=2)   # head dim 80, n_embd no multiple of 64
    refused("multiples of 64", n_inner=500)
    # what is accepted: the other name of the activation, n_inner None and given, reorder_and_upcast_attn either way
    assert R.gpt2_dims(cfg | {"activation_function": "gelu_pytorch_tanh"}) == dims
    assert R.gpt2_dims(cfg | {"n_inner": None})["ffn_dim"] == 512 and R.gpt2_dims(cfg | {"n_inner": 320})["ffn_dim"] == 320
    assert R.gpt2_dims(cfg | {"reorder_and_upcast_attn": True}) == R.gpt2_dims(cfg | {"reorder_and_upcast_attn": False}) == dims
    # the layout: an lm_head that is not wte, a c_attn that was not stored as Conv1D, a missing tensor
    st = gpt2_state(model)
    R.gpt2_device_layout(st, dims)
    with pytest.raises(ValueError, match="lm_head"):
        R.gpt2_device_layout(dict(st, **{"lm_head.weight": st["lm_head.weight"] + 1}), dims)
    with pytest.raises(ValueError, match=r"c_attn.weight: shape \(384, 128\), expected \(128, 384\)"):
        R.gpt2_device_layout(dict(st, **{"transformer.h.0.attn.c_attn.weight": st["transformer.h.0.attn.c_attn.weight"].t()}), dims)
    with pytest.raises(ValueError, match=r"c_fc.weight: shape"):
        R.gpt2_device_layout(dict(st, **{"transformer.h.0.mlp.c_fc.weight": st["transformer.h.0.mlp.c_fc.weight"].t()}), dims)
    with pytest.raises(KeyError, match="ln_f.bias"):
        R.gpt2_device_layout({k: v for k, v in st.items() if k != "transformer.ln_f.bias"}, dims)
    with pytest.raises(ValueError, match=r"wpe.weight: shape"):
        R.gpt2_device_layout(st, dict(dims, max_pos=64))
    assert torch.equal(st["lm_head.weight"], st["transformer.wte.weight"])


# ---- the restatement against HF ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_fp64_restatement_matches_hf_fp32(name):
    """The unrounded float64 restatement against the HF fp32 CPU model (eager attention) at lengths 1, 2, 17, 31, 32, 33, 64,
    65, 100: what separates them is HF's fp32 arithmetic.  Asserted at 10 x the measured HF_MEASURED.  The restatement is the
    right function: gelu_new, q scaled by head_dim^-0.5, wpe read at the position itself, Conv1D as x @ W + b."""
    import llm_rescore as R
    model, cfg = tiny_gpt2(name)
    dims = R.gpt2_dims(cfg)
    seqs = tiny_seqs(cfg["vocab_size"], seed=4)
    assert [len(s) for s in seqs] == [1, 2, 17, 31, 32, 33, 64, 65, 100]
    ref = np.concatenate(ref_logp_gpt2(gpt2_state(model), dims, seqs, rounded=False))
    hf = np.concatenate(hf_logp(model, seqs))
    err = float(np.abs(ref - hf).max())
    print(f"CLM gpt2 fp64 restatement vs HF fp32 {name}: max |dlogp| {err:.3e} (min logp {hf.min():.2f})")
    assert hf.min() < -10
    assert err <= 10 * HF_MEASURED[name], (name, err)


# ---- the entry points --------------------------------------------------------------------------------------------------------
def _flat(lib, desc, ids, off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None, tree=False):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    d = C.byref(desc) if desc is not None else None
    n = len(off) - 1 if n_seq is None else n_seq
    if tree:
        return lib.b2t_clm_gpt2_score_tree_f16(d, ids.ctypes.data, off.ctypes.data, n, scores, None, None, ws, ws_bytes, None)
    return lib.b2t_clm_gpt2_score_f16(d, ids.ctypes.data, off.ctypes.data, n, scores, None, ws, ws_bytes, None)


@pytest.mark.parametrize("tree", [False, True])
def test_score_refusals_before_device_work(tree):
    import b2t_native as N
    lib = N.load()
    who = ENTRY[1] if tree else ENTRY[0]
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, named=True, **kw):
        rc = _flat(lib, desc, ids, off, tree=tree, **kw)
        err = N.last_error()
        assert rc != 0 and re.search(match, err), (match, rc, err)
        assert not named or err.startswith(who + ":"), err      # the entry point's own name

    refused("null model", None, named=False)
    refused("head dim 32", _model(d=256, heads=8), named=False)
    refused("multiples of 64", _model(d=80, heads=1), named=False)
    refused("multiples of 64", _model(d=256, heads=4, ffn=500), named=False)
    refused("null weight", N.ClmDesc(0, 256, 4, 512, 1000, 64, FAKE, 0, FAKE, FAKE, None), named=False)
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    desc = _model()
    need = lib.b2t_clm_tree_ws_bytes(C.byref(desc), 4, 4, 2) if tree else lib.b2t_clm_ws_bytes(C.byref(desc), 4, 2)
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
        return lib.b2t_clm_gpt2_score_tree_cached_f16(C.byref(desc) if desc is not None else None,
                                                      C.byref(cache) if cache is not None else None, update, ids.ctypes.data,
                                                      off.ctypes.data, len(off) - 1 if n_seq is None else n_seq, scores, None,
                                                      None, None, ws, ws_bytes, None)

    def refused(match, desc, cache=None, named=True, **kw):
        cache = _cache() if cache is None else cache
        n0, ids0 = cache.n, cache._keep.copy()
        rc = call(desc, cache, **kw)
        err = N.last_error()
        assert rc != 0 and re.search(match, err), (match, rc, err)
        assert not named or err.startswith(who + ":"), err
        assert cache.n == n0 and (cache._keep == ids0).all()      # a refusal leaves the cache alone

    refused("null model", None, named=False)
    refused("head dim 32", _model(d=256, heads=8), named=False)
    refused("multiples of 64", _model(d=256, heads=4, ffn=500), named=False)
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("max_pos", _model(max_pos=3), cache=_cache(cap=3), ids=[2, 5, 7, 9], off=[0, 4])
    rc = call(_model(), None)
    assert rc != 0 and re.search(r"null cache \(callers without one use b2t_clm_gpt2_score_tree_f16\)", N.last_error())
    refused("null cache member", _model(), cache=_cache(kv=None))
    refused("null cache member", _model(), cache=_cache(logp=None))
    refused("cap 0", _model(), cache=_cache(ids=(), cap=0))
    refused("above max_pos", _model(max_pos=64), cache=_cache(cap=65))
    refused(r"n 9 outside", _model(), cache=_cache(cap=8, n=9))
    refused(r"n -1 outside", _model(), cache=_cache(cap=8, n=-1))
    refused("cached token 1 has id 1000", _model(vocab=1000), cache=_cache(ids=(2, 1000)))
    desc = _model()
    ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]              # 9 tokens, 4 nodes, trunk 2
    need = lib.b2t_clm_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
    refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
    need3 = lib.b2t_clm_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)  # the cache (2, 5) spares one row
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
    refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)


def test_symbols_sizes_and_struct_layouts(tmp_path):
    """The header declares the three entry points and the library exports them with the OPT twins' signatures; the family has
    no size function of its own (the OPT ones serve both); b2t_clm_t, b2t_clm_layer_t and b2t_clm_cache_t are what they were."""
    import b2t_native as N
    lib = N.load()
    declared = [s for s in N.header_symbols() if "gpt2" in s]
    assert sorted(declared) == sorted(ENTRY)
    twins = {"b2t_clm_gpt2_score_f16": "b2t_clm_score_f16", "b2t_clm_gpt2_score_tree_f16": "b2t_clm_score_tree_f16",
             "b2t_clm_gpt2_score_tree_cached_f16": "b2t_clm_score_tree_cached_f16"}
    for name in ENTRY:
        assert hasattr(lib, name) and N._SIGNATURES[name] == N._SIGNATURES[twins[name]]
    with open(os.path.join(ROOT, "include", "b2t.h")) as f:
        hdr = f.read()
    for size_fn in ("b2t_clm_ws_bytes", "b2t_clm_tree_ws_bytes", "b2t_clm_cache_kv_bytes", "b2t_clm_tree_cached_ws_bytes"):
        assert size_fn in hdr[hdr.index("the same scoring for GPT-2"):hdr.index("int b2t_clm_gpt2_score_f16")]
    assert not re.search(r"b2t_clm_gpt2_\w*bytes", hdr)
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    structs = {"b2t_clm_layer_t": (N.ClmLayer, 96), "b2t_clm_t": (N.ClmDesc, 64), "b2t_clm_cache_t": (N.ClmCache, 32)}
    body = ""
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
        name, val = line.split()
        if "." in name:
            cname, field = name.split(".")
            assert getattr(structs[cname][0], field).offset == int(val), name
        else:
            assert C.sizeof(structs[name][0]) == int(val) == structs[name][1], name
        seen += 1
    assert seen == 3 + 12 + 11 + 5


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_gpt2_unit_has_two_gemm_kernels_without_scratch():
    """causal_lm_gpt2.hip instantiates the EP_GELU GEMM on both tiles and nothing else; neither spills (at the time of writing
    222 VGPRs on the 256-tile, 86 VGPRs + 64 AGPRs on the 128-tile).  The tile rule is not restated there."""
    import wave_kernel_resources as W
    res = W.resources(src="causal_lm_gpt2.hip")
    assert len(res) == 2 and all("clm_gemm_kernel" in k for k in res), sorted(res)
    assert sorted("256" in k.split("clm_gemm_kernel")[1][:8] for k in res) == [False, True], sorted(res)
    for k, v in res.items():
        assert v.get("ScratchSize", -1) == 0 and 0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256, (k, v)
    src = open(os.path.join(CSRC, "causal_lm_gpt2.hip")).read()
    assert "getenv" not in src and "B2T_CLM_GEMM_256" not in src
    assert "launch_gemm(g, s, &clm_gemm_tiles<EP_GELU>)" in src
    import __graft_entry__ as G
    assert "causal_lm_gpt2.hip" in G.HIP_SOURCES


# ---- the Python surface -------------------------------------------------------------------------------------------------------
def test_python_surface(tmp_path):
    import torch
    import llm_rescore as R
    model, cfg = tiny_gpt2("hd64")
    model.save_pretrained(str(tmp_path))
    sc = R.build_scorer(str(tmp_path), device="cpu")
    assert type(sc) is R.Gpt2Scorer and isinstance(sc, R.OptScorer) and sc.dtype is torch.float16
    assert sc._ENTRY == "b2t_clm_gpt2_" and R.OptScorer._ENTRY == "b2t_clm_"
    assert sc.dims == R.gpt2_dims(cfg) and sc.desc.max_pos == 128 and sc.desc.ffn_dim == 512
    assert sc.share_prefixes is False and sc.cache_len == 0 and sc.eval() is sc
    for dtype in ("auto", "float16", torch.float16, None):
        assert R.build_scorer(str(tmp_path), device="cpu", dtype=dtype).dtype is torch.float16
    # a config that says bfloat16: "auto" is still fp16
    with open(tmp_path / "config.json") as f:
        saved = json.load(f)
    with open(tmp_path / "config.json", "w") as f:
        json.dump(saved | {"torch_dtype": "bfloat16"}, f)
    assert R.build_scorer(str(tmp_path), device="cpu", dtype="auto").dtype is torch.float16
    # bfloat16 is refused with the family's own message, before any weight is read
    os.rename(tmp_path / "model.safetensors", tmp_path / "model.safetensors.away")
    with pytest.raises(ValueError, match="Gpt2Scorer: dtype 'bfloat16' is not supported for GPT-2"):
        R.build_scorer(str(tmp_path), device="cpu", dtype="bfloat16")
    with pytest.raises(ValueError, match="is not supported"):
        R.build_scorer(str(tmp_path), device="cpu", dtype="float32")
    with pytest.raises(FileNotFoundError):
        R.build_scorer(str(tmp_path), device="cpu")
    dims = R.gpt2_dims(cfg)
    with pytest.raises(ValueError, match="Gpt2Scorer: dtype 'bfloat16'"):
        R.Gpt2Scorer(dims, {}, "cpu", dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="OptScorer: dtype 'bfloat16'"):     # OPT's message is still OPT's
        R.OptScorer(dims, {}, "cpu", dtype="bfloat16")
    # an erf-GELU config is refused by build_scorer, naming the field
    with open(tmp_path / "config.json", "w") as f:
        json.dump(saved | {"activation_function": "gelu"}, f)
    with pytest.raises(ValueError, match="activation_function 'gelu'"):
        R.build_scorer(str(tmp_path), device="cpu")
