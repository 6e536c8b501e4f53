"""Host-side checks of csrc/causal_lm.hip (no GPU): every kernel compiles without scratch, b2t_clm_ws_bytes' sizes, and the
refusals of b2t_clm_score_f16, which all return before any device work (so fake non-null weight pointers will do)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
FAKE = 0x10000   # a non-null "device" pointer that is never dereferenced


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_clm_kernels_do_not_spill():
    # spilled MFMA operand tuples came back wrong on ROCm 7.2 (NOTES.md R6.2); at the time of writing all 15 kernels have
    # scratch 0 and at most 224 VGPRs (the 256-tile GEMM 222; the attention 175 / 204 / 224 VGPRs and 62 / 68 / 124 AGPRs at
    # head dim 64 / 80 / 128).  clm_attn_kernel is the Llama family's flat attention too
    import wave_kernel_resources as W
    res = {k: v for k, v in W.resources(src="causal_lm.hip").items() if "clm_" in k}
    gemm = [k for k in res if "clm_gemm_kernel" in k]
    attn = [k for k in res if "clm_attn_kernel" in k]
    assert len(gemm) == 8 and len(attn) == 3 and len(res) == 15, sorted(res)
    spilled = {k: v for k, v in res.items() if v.get("ScratchSize", -1) != 0}
    assert not spilled, spilled
    assert all(0 <= v.get("VGPRs", -1) <= 256 and 0 <= v.get("AGPRs", -1) <= 256 for v in res.values()), res


def test_tile_rule_is_the_one_the_gpu_tests_mirror():
    # tests/test_gpu_clm_contract.py asserts from the dims which GEMMs the default rule puts on 256-tiles; a retune of the rule
    # in launch_gemm has to update that mirror (_tile) too
    src = open(os.path.join(ROOT, "nejm-brain-to-text_amd", "csrc", "causal_lm.hip")).read()
    body = src[src.index("int launch_gemm("):]
    body = body[:body.index("\n}\n")]
    assert re.search(r"mode == 2 \|\| \(mode != 0 && \(long long\)m256 \* n256 >= 256\)", body), body
    assert 'getenv("B2T_CLM_GEMM_256")' in body


def _model(n_layers=1, d=256, heads=4, ffn=512, vocab=1000, max_pos=64):
    import b2t_native as N
    layers = (N.ClmLayer * max(1, n_layers))()
    for i in range(n_layers):
        for f, _ in N.ClmLayer._fields_:
            setattr(layers[i], f, FAKE)
    desc = N.ClmDesc(n_layers, d, heads, ffn, vocab, max_pos, FAKE, FAKE, FAKE, FAKE, layers)
    desc._keep = layers
    return desc


def _ws(lib, desc, n_tokens, n_seq):
    return lib.b2t_clm_ws_bytes(C.byref(desc), n_tokens, n_seq)


def test_ws_bytes():
    import b2t_native as N
    lib = N.load()
    desc = _model()
    assert lib.b2t_clm_ws_bytes(None, 10, 1) == 0
    for n_tok, n_seq in ((0, 1), (-1, 1), (5, 0), (5, -1), (5, 6)):
        assert _ws(lib, desc, n_tok, n_seq) == 0, (n_tok, n_seq)
    d, F, V = 256, 512, 1000
    ncg = (V + 63) // 64
    prev = 0
    for M in list(range(1, 600, 7)) + [4095, 4096, 4097]:
        for n_seq in sorted({1, max(1, M // 3), M}):
            b = _ws(lib, desc, M, n_seq)
            Mh, Mp = M - n_seq, -(-M // 256) * 256
            parts = [4 * (2 * M + 2 * Mh + 2 * (n_seq + 1)), 4 * M * d, 2 * Mp * d, 2 * M * 3 * d, 2 * Mp * F,
                     4 * Mh * ncg, 4 * Mh * ncg, 4 * Mh, 4 * Mh]
            assert b >= sum(parts) and b % 256 == 0, (M, n_seq, b, sum(parts))
        b1 = _ws(lib, desc, M, 1)
        assert b1 >= prev, M   # monotone in n_tokens (one sequence)
        prev = b1
    # at a fixed n_seq too
    sizes = [_ws(lib, desc, M, 4) for M in range(4, 2000, 13)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))


def _call(lib, desc, ids, off, ws_bytes=1 << 30):
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(off, np.int32)
    return lib.b2t_clm_score_f16(C.byref(desc) if desc is not None else None, ids.ctypes.data, off.ctypes.data, len(off) - 1,
                                 FAKE, None, FAKE, ws_bytes, None)


def test_score_refusals_before_device_work():
    import b2t_native as N
    lib = N.load()
    ok_ids, ok_off = [2, 5, 7, 9], [0, 1, 4]

    def refused(match, desc, ids=ok_ids, off=ok_off, **kw):
        rc = _call(lib, desc, ids, off, **kw)
        assert rc != 0 and re.search(match, N.last_error()), (match, rc, N.last_error())

    refused("null model", None)
    refused("head dim 32", _model(d=256, heads=8))
    refused("multiples of 64", _model(d=80, heads=1))          # head dim 80, d not a multiple of 64
    refused("multiples of 64", _model(d=256, heads=4, ffn=500))
    refused("null weight", N.ClmDesc(0, 256, 4, 512, 1000, 64, FAKE, 0, FAKE, FAKE, None))
    refused("empty", _model(), off=[0, 1, 1, 4])
    refused(r"seq_off\[0\] = 1", _model(), off=[1, 2, 4])
    refused("outside", _model(vocab=1000), ids=[2, 5, 1000, 9])
    refused("outside", _model(vocab=1000), ids=[2, 5, -1, 9])
    refused("max_pos", _model(max_pos=3), ids=[2, 5, 7, 9], off=[0, 4])
    desc = _model()
    need = _ws(lib, desc, 4, 2)
    refused("workspace", desc, ws_bytes=need - 1)
