"""Host-side checks of the Llama family's context cache (b2t_clm_llama_cache_kv_bytes, b2t_clm_llama_tree_cached_ws_bytes,
b2t_clm_llama_score_tree_cached_f16 in csrc/causal_lm_llama.hip; LlamaScorer(context_cache_tokens=...); no GPU): the two size
functions as host arithmetic, every refusal of the entry point (all before any device work, so fake non-null pointers will
do, and the cache is left as it was), the Python surface with its refusal on a device without GPU memory, and the kernels of
the translation unit.  The rule itself is family-independent (b2t_clm_cache_plan_host, tests/test_clm_cache_host.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_clm_cache_host import _cache
from test_clm_llama_host import FAKE, _model, state_of, tiny_model


def _al(x):
    return -(-x // 256) * 256


def test_cache_and_workspace_sizes_are_host_arithmetic():
    import b2t_native as N
    lib = N.load()
    desc = _model(n_layers=3, d=256, heads=4, kv=2, ffn=512, vocab=1000, max_pos=64)
    kvb = lambda cap, m=desc: lib.b2t_clm_llama_cache_kv_bytes(C.byref(m) if m is not None else None, cap)
    for cap in (1, 2, 33, 64):
        assert kvb(cap) == 3 * cap * 2 * 2 * 64 * 2        # n_layers * cap * (K | V) * n_kv_heads * head_dim * fp16
    assert kvb(0) == 0 and kvb(-1) == 0 and kvb(65) == 0 and kvb(8, None) == 0
    assert kvb(8, _model(n_layers=0)) == 0 and kvb(8, _model(kv=0)) == 0 and kvb(8, _model(heads=0)) == 0
    assert kvb(8, _model(d=250, heads=4)) == 0             # d_model no multiple of n_heads: no head dim
    # the row is the K / V heads', not d_model's: group sizes 1 and 8 at the same d_model
    assert kvb(4, _model(d=512, heads=8, kv=8)) == 4 * 2 * 512 * 2 and kvb(4, _model(d=512, heads=8, kv=1)) == 4 * 2 * 64 * 2
    # Llama-3-8B: 128 KiB per position, 256 MiB for 2048
    big = _model(n_layers=32, d=4096, heads=32, kv=8, ffn=14336, vocab=128256, max_pos=2048)
    assert kvb(1, big) == 128 << 10 and kvb(2048, big) == 256 << 20

    ws = lambda r, t, s, m=desc: lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(m), r, t, s)
    tree = lambda r, t, s: lib.b2t_clm_llama_tree_ws_bytes(C.byref(desc), r, t, s)
    assert lib.b2t_clm_llama_tree_cached_ws_bytes(None, 5, 10, 1) == 0
    assert ws(5, 10, 1, _model(kv=0)) == 0 and ws(5, 10, 1, _model(heads=0)) == 0
    for r, t, s in ((0, 5, 1), (-1, 5, 1), (6, 5, 1), (5, 0, 1), (1, -1, 1), (3, 5, 0), (3, 5, -1), (3, 5, 6)):
        assert ws(r, t, s) == 0, (r, t, s)
    for r, t, s in ((1, 1, 1), (1, 40, 1), (40, 400, 7), (257, 3000, 100), (3000, 3000, 100)):
        # what the tree call needs for r rows, plus m, l per (row, query head) and the unnormalised o per row in fp32
        assert ws(r, t, s) == tree(r, t, s) + _al(4 * r * 4 * 2) + _al(4 * r * 256), (r, t, s)
    for s_ in ([ws(r, 3000, 7) for r in range(1, 3001, 11)], [ws(40, t, 7) for t in range(40, 3000, 13)],
               [ws(40, 3000, n) for n in range(1, 3001, 17)]):
        assert all(a > 0 for a in s_) and all(a <= b for a, b in zip(s_, s_[1:]))
    # the tree call's own size function has no term for the state
    qw, ncg = (4 + 2 * 2) * 64, -(-1000 // 64)
    parts = [4 * (4 * 40 + 2 * 400 + 2 * 7 + 1), 4 * 40 * 256, 2 * 256 * 256, 2 * 40 * qw, 2 * 256 * 512,
             4 * 40 * ncg, 4 * 40 * ncg, 4 * 40, 4 * 40]
    assert tree(40, 400, 7) == sum(_al(p) for p in parts)


def test_cached_score_refusals_before_device_work():
    """Every refusal of the Llama tree call is one here, plus the cache's own, word for word b2t_clm_score_tree_cached_f16's."""
    import b2t_native as N
    lib = N.load()
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def call(desc, cache, ids=ok_ids, off=ok_off, ws_bytes=1 << 30, scores=FAKE, ws=FAKE, n_seq=None, update=1):
        ids = np.ascontiguousarray(ids, np.int32)
        off = np.ascontiguousarray(off, np.int32)
        return lib.b2t_clm_llama_score_tree_cached_f16(C.byref(desc) if desc is not None else None,
                                                       C.byref(cache) if cache is not None else None, update, ids.ctypes.data,
                                                       off.ctypes.data, len(off) - 1 if n_seq is None else n_seq, scores, None,
                                                       None, None, ws, ws_bytes, None)

    def refused(match, desc, cache=None, **kw):
        cache = _cache() if cache is None else cache
        n0, ids0 = cache.n, cache._keep.copy()
        rc = call(desc, cache, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())
        assert cache.n == n0 and (cache._keep == ids0).all()      # a refusal leaves the cache alone

    # the model's
    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8, kv=8))
    refused("head dim 80", _model(d=320, heads=4, kv=4))
    refused("multiple of n_heads", _model(d=256, heads=3, kv=3))
    refused("multiple of n_kv_heads", _model(d=512, heads=8, kv=3))
    refused("multiples of 64", _model(d=256, heads=4, ffn=500))
    refused("bad dimensions", _model(kv=0))
    refused("bad dimensions", _model(max_pos=0))
    refused("rms_eps", _model(eps=-1.0))
    refused("null weight", N.ClmLlamaDesc(0, 256, 4, 2, 512, 1000, 64, 1e-5, FAKE, FAKE, FAKE, FAKE, 0, None))
    bad = _model()
    bad.layers_host[0].down_w = None
    refused("null weight pointer in layer 0", bad)
    # the list's
    refused("null argument", _model(), scores=None)
    refused("null argument", _model(), ws=None)
    refused("n_seq 0", _model(), n_seq=0)
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), cache=_cache(cap=3), ids=[2, 5, 7, 9], off=[0, 4])
    # the cache's own
    rc = call(_model(), None)
    assert rc != 0 and re.search("null cache .*b2t_clm_llama_score_tree_f16", N.last_error())
    refused("null cache member", _model(), cache=_cache(kv=None))
    refused("null cache member", _model(), cache=_cache(logp=None))
    c = _cache()
    c.ids_host = None
    rc = call(_model(), c)
    assert rc != 0 and re.search("null cache member", N.last_error())
    refused("cap 0", _model(), cache=_cache(ids=(), cap=0))
    refused("cap -1", _model(), cache=_cache(ids=(), cap=-1))
    refused("above max_pos", _model(max_pos=64), cache=_cache(cap=65))
    refused(r"n 9 outside", _model(), cache=_cache(cap=8, n=9))
    refused(r"n -1 outside", _model(), cache=_cache(cap=8, n=-1))
    refused("cached token 1 has id 1000", _model(vocab=1000), cache=_cache(ids=(2, 1000)))
    refused("cached token 0 has id -3", _model(vocab=1000), cache=_cache(ids=(-3, 5)))
    # the workspace: one byte less than the rows computed need, with and without reuse, updating or not, with and without
    # q / k / v biases
    for desc in (_model(), _model(bias=False)):
        ids, off = [2, 5, 7, 2, 5, 8, 2, 5, 7], [0, 3, 6, 9]              # 9 tokens, 4 nodes, trunk 2
        need = lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(desc), 4, 9, 3)
        refused("workspace", desc, cache=_cache(ids=()), ids=ids, off=off, ws_bytes=need - 1)
        need3 = lib.b2t_clm_llama_tree_cached_ws_bytes(C.byref(desc), 3, 9, 3)  # the cache (2, 5) spares one row
        assert 0 < need3 <= need
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1)
        refused("workspace", desc, cache=_cache(ids=(2, 5)), ids=ids, off=off, ws_bytes=need3 - 1, update=0)


def test_python_surface(tmp_path):
    """The cache is off unless asked for; its management is _Scorer's, one definition for both families; on a device without
    GPU memory LlamaScorer refuses context_cache_tokens > 0 in one message that names both the parameter and the cache."""
    import llm_rescore as R
    assert inspect.signature(R.LlamaScorer.__init__).parameters["context_cache_tokens"].default == 0
    assert inspect.signature(R.build_scorer).parameters["context_cache_tokens"].default == 0
    assert list(inspect.signature(R.LlamaScorer.__init__).parameters)[:6] == ["self", "dims", "arrays", "device", "share_prefixes",
                                                                              "context_cache_tokens"]
    assert list(inspect.signature(R.build_scorer).parameters)[:4] == ["model_dir", "device", "share_prefixes", "context_cache_tokens"]
    for fn in (R.LlamaScorer.score, R.LlamaScorer.token_logprobs):
        assert inspect.signature(fn).parameters["use_cache"].default is None
        assert inspect.signature(fn).parameters["update_cache"].default is True
    for name in ("cache_len", "cache_ids", "cache_reset", "_alloc_cache"):
        assert getattr(R.LlamaScorer, name) is getattr(R._Scorer, name) is getattr(R.OptScorer, name), name
    assert isinstance(R._Scorer.cache_len, property) and isinstance(R._Scorer.cache_ids, property)
    assert "context cache" in R.LlamaScorer._NO_CACHE

    model, cfg = tiny_model("llama", n_layers=1)
    model.save_pretrained(str(tmp_path))
    dims = R.llama_dims(cfg)
    lay = R.llama_device_layout(state_of(model, False), dims, R.rope_inv_freq(cfg))
    for make in (lambda n: R.LlamaScorer(dims, dict(lay), "cpu", False, n),
                 lambda n: R.build_scorer(str(tmp_path), device="cpu", context_cache_tokens=n)):
        with pytest.raises(ValueError) as e:
            make(64)
        msg = str(e.value)
        assert "context cache" in msg and "context_cache_tokens" in msg and "GPU memory" in msg and "cpu" in msg
        sc = make(0)
        assert sc.context_cache_tokens == 0 and sc.cache_len == 0 and sc.cache_ids.shape == (0,)
        sc.cache_reset()
        with pytest.raises(ValueError, match="context cache"):
            sc.score([[2, 3]], use_cache=True)
        with pytest.raises(ValueError, match="context cache"):
            sc.token_logprobs([[2, 3]], use_cache=True)
    with pytest.raises(ValueError, match="context_cache_tokens < 0"):
        R.LlamaScorer(dims, dict(lay), "cpu", False, -1)
    # the two classes size their cache through different library functions, each one the library has
    import torch
    import b2t_native as N
    lib = N.load()

    class Names:
        def __init__(self):
            self.seen = []

        def __getattr__(self, name):
            self.seen.append(name)
            return getattr(lib, name)

    odims = dict(n_layers=0, d_model=64, n_heads=1, ffn_dim=64, vocab=8, max_pos=16)
    oarr = {k: torch.zeros(n, 64, dtype=torch.float16) for k, n in (("embed_tokens", 8), ("embed_positions", 18))}
    oarr.update({k: torch.zeros(64, dtype=torch.float16) for k in ("final_ln_w", "final_ln_b")})
    asked = {}
    for sc in (R.LlamaScorer(dims, dict(lay), "cpu"), R.OptScorer(odims, oarr, "cpu")):
        names = Names()
        sc._cache_kv_bytes(names, 8)
        assert len(names.seen) == 1 and hasattr(lib, names.seen[0]), names.seen
        asked[type(sc)] = names.seen[0]
    assert asked == {R.LlamaScorer: "b2t_clm_llama_cache_kv_bytes", R.OptScorer: "b2t_clm_cache_kv_bytes"}
    # build_scorer refuses before it reads the weights: a directory with nothing but config.json
    bare = tmp_path / "bare"
    bare.mkdir()
    (bare / "config.json").write_text((tmp_path / "config.json").read_text())
    with pytest.raises(ValueError, match="GPU memory"):
        R.build_scorer(str(bare), device="cpu", context_cache_tokens=64)
    with pytest.raises(FileNotFoundError):
        R.build_scorer(str(bare), device="cpu")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_llama_unit_keeps_its_six_kernels():
    """The cached entry point added no kernel to causal_lm_llama.hip: its attention, append and sums are causal_lm_cache.hip's
    (whose nine kernels tests/test_clm_cache_host.py counts), reached through the launchers of clm_internal.h."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm_llama.hip").items() if "clm_" in k}
    assert len(res) == 6 and not [k for k in res if "attn" in k or "cache" in k], sorted(res)
    assert all(v.get("ScratchSize", -1) == 0 for v in res.values()), res
