"""The exact-fp32 GRU sweeps -- step-launch (mode 0: gru_step_fwd_kernel / gru_step_bwd_kernel, csrc/gru.hip), persistent (mode 1:
gru_persist_fwd_kernel / gru_persist_bwd_kernel, csrc/gru_persistent.hip), 32-unit workgroups (mode 1 | WIDE), the XCD-local hand-off
and the fused forward -- through the C ABI, one layer per launch, against the operand-forced fp64 oracle of oracle/gru_bf16.py with
round = identity: every step is the fp64 cell function of the tensors the kernel itself wrote, the bound is M x the float32 roundoff
e32 of the numpy stand-in against the same oracle (M = 16 / 16 / 8 / 8, the bf16 sweeps' constants; capped at 1e-4 resp. 1e-3 of
the oracle tensor's rms) and does not grow with T.  The backward sweep reads the forward sweep's own tensors, as in the product.

Every output is filled with NaN before the launch and sits between two guards of 64 sentinel words that must come back unchanged
(rows beyond B in the last row group, units of the last workgroup); the sync block's error word stays 0.
Shapes: oracle/gru_bf16.py FP32_SWEEP_SHAPES.  Measured err / e32 per case: NOTES.md, "The operand-forced oracle on the exact-fp32
sweeps"; what the bound refuses that the sweeps' self-comparison lets through: tests/test_gru_fp32_oracle_host.py."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nejm-brain-to-text_amd"))
sys.path.insert(0, ROOT)

from oracle import gru_bf16 as G

pytestmark = pytest.mark.gpu

WIDE, LOCAL, PARITY = 0x200, 0x400, 0x800
GUARD = 64                      # sentinel words in front of and behind every output
SENTINEL = 0x5A5AC3C3           # as float32 a finite 1.5e16: a guard word that is touched cannot come back equal by accident

SHAPES = list(G.FP32_SWEEP_SHAPES)
WIDE_OK = [s for s in SHAPES if s[2] % 32 == 0 and s[2] <= 512]
# where gru_persistent_fwd / _bwd take B2T_GRU_LOCAL: H <= 512, H % 32 == 0, at most four row groups
LOCAL_OK = [s for s in SHAPES if s[2] % 32 == 0 and s[2] <= 512 and (s[1] + 15) // 16 <= 4]
FUSED_OK = [s for s in SHAPES if s[2] <= 512]
EDGE_SHAPES = [(4, 17, 128), (6, 64, 512)]


def _dev():
    return torch.device("cuda:0")


class _Out:
    """A NaN-filled device tensor between two sentinel guards."""

    def __init__(self, *shape):
        self.n = math.prod(shape)
        self.raw = torch.empty(2 * GUARD + self.n, device=_dev())
        words = self.raw.view(torch.int32)
        words[:GUARD] = SENTINEL
        words[GUARD + self.n:] = SENTINEL
        self.t = self.raw[GUARD:GUARD + self.n].view(*shape)
        self.t.fill_(float("nan"))

    def check(self, name):
        words = self.raw.view(torch.int32)
        assert bool((words[:GUARD] == SENTINEL).all()), f"{name}: the guard in front was written"
        assert bool((words[GUARD + self.n:] == SENTINEL).all()), f"{name}: the guard behind was written"
        assert not bool(torch.isnan(self.t).any()), f"{name}: elements left unwritten"
        return self.t


_cases = {}


def _case(T, B, H):
    """Operands of a shape on host and device, its float32 floor and one sync block: made once, shared, never modified (the sync
    block cleans itself between calls, as in the product)."""
    key = (T, B, H)
    if key not in _cases:
        import b2t_native as N
        I = G.random_inputs(1, T, B, H, G.fp32_sweep_seed(T, B, H))
        up = lambda a: torch.from_numpy(a).to(_dev())
        d = dict(gi=up(I["gi0"]), w=up(I["whh"][0]), b=up(I["bhh"][0]), h0=up(I["h0"][0]), dY=up(I["dY"]), dhl=up(I["dhl"][0]))
        d["wt"] = d["w"].t().contiguous()
        g = torch.Generator().manual_seed(G.fp32_sweep_seed(T, B, H) + 1)      # the next layer's projection, for the fused forward
        d["w2"] = (torch.randn(3 * H, H, generator=g) * (1.0 / H ** 0.5)).to(_dev())
        d["b2"] = (torch.randn(3 * H, generator=g) * 0.1).to(_dev())
        d["sync"] = torch.zeros(N.load().b2t_gru_sync_bytes(T) // 4 + 16, dtype=torch.int32, device=_dev())
        _cases[key] = (I, d, G.floor_e32(I, round=G.identity), {})
    return _cases[key]


def _clean(d, what):
    torch.cuda.synchronize()
    assert int(d["sync"][0].item()) == 0, f"{what}: a hand-off spin gave up (sync word 0)"


def _forward(d, T, B, H, mode, reserve=True, h_last=False, fused=False):
    import b2t_native as N, b2t_ops as ops
    lib, p = N.load(), ops._p
    out, res = _Out(T, B, H), (_Out(T, B, 4 * H) if reserve else None)
    hl, gi2 = (_Out(B, H) if h_last else None), (_Out(T, B, 3 * H) if fused else None)
    pr, ph = (p(res.t) if reserve else None), (p(hl.t) if h_last else None)
    if fused:
        N.check(lib.b2t_gru_layer_fwd_fused_f32(p(d["gi"]), p(d["w"]), p(d["b"]), p(d["h0"]), p(out.t), pr, ph, p(d["w2"]), p(d["b2"]),
                                                p(gi2.t), T, B, H, mode, p(d["sync"]), ops._stream()), "fused fwd")
    else:
        N.check(lib.b2t_gru_layer_fwd_f32(p(d["gi"]), p(d["w"]), p(d["b"]), p(d["h0"]), p(out.t), pr, ph, T, B, H, mode, p(d["sync"]),
                                          ops._stream()), "fwd")
    _clean(d, f"forward, mode {mode:#x}")
    r = dict(out=out.check("out"))
    for k, o in (("res", res), ("h_last", hl), ("gi2", gi2)):
        if o is not None:
            r[k] = o.check(k)
    return r


def _backward(d, fw, T, B, H, mode, dh_last="given"):
    import b2t_native as N, b2t_ops as ops
    lib, p = N.load(), ops._p
    dG, dh = _Out(T, B, 4 * H), _Out(B, H)
    sc = torch.empty(B, H, device=_dev())
    dhl = {"given": d["dhl"], "zeros": torch.zeros(B, H, device=_dev()), None: None}[dh_last]
    N.check(lib.b2t_gru_layer_bwd_f32(p(d["dY"]), p(dhl), p(fw["res"]), p(fw["out"]), p(d["h0"]), p(d["wt"]), p(dG.t), p(dh.t), p(sc),
                                      T, B, H, mode, p(d["sync"]), ops._stream()), "bwd")
    _clean(d, f"backward, mode {mode:#x}")
    return dict(dG=dG.check("dG"), dh_init=dh.check("dh_init"))


def _run(T, B, H, mode):
    """Forward and backward sweep of a shape in `mode`: run once, shared, never modified."""
    runs = _case(T, B, H)[3]
    if mode not in runs:
        d = _case(T, B, H)[1]
        fw = _forward(d, T, B, H, mode)
        runs[mode] = {**fw, **_backward(d, fw, T, B, H, mode)}
    return runs[mode]


VARIANTS = [(s, 0, "step-launch") for s in SHAPES] + [(s, 1, "persistent") for s in SHAPES] + [(s, 1 | WIDE, "wide") for s in WIDE_OK]


@pytest.mark.parametrize("shape,mode,name", VARIANTS, ids=[f"{n}-{s[0]}-{s[1]}-{s[2]}" for s, _, n in VARIANTS])
def test_sweep_is_the_fp64_cell_function_of_its_own_tensors(shape, mode, name):
    T, B, H = shape
    I, _, e32, _ = _case(T, B, H)
    r = _run(T, B, H, mode)
    cpu = lambda t: t.cpu().numpy()
    G.check_kernel(I, dict(out=[cpu(r["out"])], outd=[None], res=[cpu(r["res"])], dG=[cpu(r["dG"])], dh_init=[cpu(r["dh_init"])]),
                   f"{name} ({T},{B},{H})", round=G.identity, e32=e32)


@pytest.mark.parametrize("parity", [0, PARITY], ids=["even", "odd"])
@pytest.mark.parametrize("T,B,H", LOCAL_OK)
def test_xcd_local_handoff_equals_the_device_scope_one_bit_for_bit(T, B, H, parity):
    base, got = _run(T, B, H, 1), _run(T, B, H, 1 | LOCAL | parity)
    for k in ("out", "res", "dG", "dh_init"):
        assert torch.equal(got[k], base[k]), k


@pytest.mark.parametrize("T,B,H", FUSED_OK)
def test_fused_forward_is_the_persistent_sweep_and_its_projection_the_fp64_product(T, B, H):
    d = _case(T, B, H)[1]
    base = _run(T, B, H, 1)
    got = _forward(d, T, B, H, 1, fused=True)
    assert torch.equal(got["out"], base["out"]) and torch.equal(got["res"], base["res"])
    # gi_next against the fp64 product of the kernel's own out rows: 16 x the float32 roundoff of the same product in numpy
    # (the constant of `out`: an fp32-accumulated contraction over H plus a bias), no looser than the fused sweep's existing tolerance
    x, w2, b2 = got["out"].cpu().numpy().reshape(T * B, H), d["w2"].cpu().numpy(), d["b2"].cpu().numpy()
    ref = x.astype(np.float64) @ w2.astype(np.float64).T + b2
    floor = float(np.abs((x @ w2.T + b2).astype(np.float64) - ref).max())
    err = float(np.abs(got["gi2"].cpu().numpy().reshape(T * B, 3 * H).astype(np.float64) - ref).max())
    print(f"[fp32 oracle] fused ({T},{B},{H}) gi_next: err {err:.3e}  e32 {floor:.3e}  ratio {err / floor if floor > 0 else float('inf'):.2f}  bound {16 * floor:.3e}")
    assert 0 < floor and 16 * floor <= 2e-5 * max(1.0, float(np.abs(ref).max()))
    assert err <= 16 * floor


@pytest.mark.parametrize("mode", [0, 1], ids=["step-launch", "persistent"])
@pytest.mark.parametrize("T,B,H", EDGE_SHAPES)
def test_optional_arguments_and_repeated_calls(T, B, H, mode):
    d = _case(T, B, H)[1]
    base = _run(T, B, H, mode)
    fw = _forward(d, T, B, H, mode, reserve=False, h_last=True)
    assert torch.equal(fw["out"], base["out"]), "reserve = NULL changed out"
    assert torch.equal(fw["h_last"], base["out"][T - 1])
    zeros, null = _backward(d, base, T, B, H, mode, dh_last="zeros"), _backward(d, base, T, B, H, mode, dh_last=None)
    for k in ("dG", "dh_init"):
        assert torch.equal(null[k], zeros[k]), f"dh_last = NULL: {k}"
    assert not torch.equal(zeros["dh_init"], base["dh_init"])        # (dh_last is read at all)
    if mode == 1:   # the sync block has served every call above: one more sweep pair on it repeats the first one
        again = _forward(d, T, B, H, mode)
        again.update(_backward(d, again, T, B, H, mode))
        for k in ("out", "res", "dG", "dh_init"):
            assert torch.equal(again[k], base[k]), f"second call on the same sync block: {k}"
