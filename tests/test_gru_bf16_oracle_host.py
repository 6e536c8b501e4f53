"""The bf16 GRU oracles of oracle/gru_bf16.py on the CPU: what the GPU tests of the layer wavefront and the bf16 persistent sweep
(tests/test_gpu_wave.py, tests/test_gpu_parity.py test_persistent_sweep_bf16_operands) rest on.

  * tie: without rounding and masks the free-running recurrences ARE oracle.b2t_oracle.gru_fwd / gru_bwd, which
    tests/golden/train_step.npz pins to the reference;
  * floor: the float32 stand-in against the operand-forced oracle (e32) is positive and, times M, inside the caps the GPU tests
    assert;
  * mutations: every deliberately wrong stand-in is >= 4 x over the operand-forced bound on some tensor -- and which of them the
    free-running comparison's tolerance accepts is recorded here, so that the gap stays documented.
M and its measured table: NOTES.md, "The operand-forced bf16 GRU oracle"."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import b2t_oracle as O
from oracle import gru_bf16 as G


def _inputs(L, T, B, H, p):
    I = G.random_inputs(L, T, B, H, seed=L * 1000 + H + B)       # the GPU test's own seed
    I["masks"] = G.bernoulli_masks(L, T, B, H, p, seed=7 + L + T)
    return I


_cache = {}


def _case(L, T, B, H, p):
    """Inputs and floor of a shape: computed once, shared, never modified."""
    key = (L, T, B, H, p)
    if key not in _cache:
        I = _inputs(*key)
        _cache[key] = (I, G.floor_e32(I))
    return _cache[key]


@pytest.mark.parametrize("L,T,B,H", [(3, 9, 17, 80), (2, 40, 33, 256)])
def test_free_running_without_rounding_is_the_pinned_oracle(L, T, B, H):
    """round = identity, no masks, layer 0's projection the identity (gi0 is the input), dh_last = 0: fp64 against the fp32 of
    b2t_oracle.  Bounds: out 2e-6, dh_init and layer 0's dgi 5e-7 (measured 1.8e-7 / 4.2e-7 and 2.2e-8 ... 6.7e-8)."""
    I = G.random_inputs(L, T, B, H, seed=L * 1000 + H + B, with_dhl=False)
    outs, _, _, dG, dh = G.free_running(I["gi0"], I["whh"], I["bhh"], I["wih"], I["bih"], I["h0"], None, I["dY"], None, round=G.identity)
    w_ih = [np.eye(3 * H, dtype=np.float32)] + I["wih"][1:]
    b_ih = [np.zeros(3 * H, np.float32)] + I["bih"][1:]
    bt = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))
    top, _, reserve = O.gru_fwd(bt(I["gi0"]), w_ih, I["whh"], b_ih, I["bhh"], np.stack(I["h0"]), save=True)
    dx, _, _, _, _, dh_o = O.gru_bwd(bt(I["dY"]), reserve, w_ih, I["whh"], np.stack(I["h0"]))
    e_out = max(float(np.abs(bt(reserve[l]["out"]) - outs[l]).max()) for l in range(L))
    e_dh = float(np.abs(dh_o - np.stack(dh)).max())
    dgi0 = np.concatenate([dG[0][..., :2 * H], dG[0][..., 3 * H:]], axis=2)
    e_dgi = float(np.abs(bt(dx) - dgi0).max())
    print(f"[tie] ({L},{T},{B},{H}): out {e_out:.2e}  dh_init {e_dh:.2e}  dgi0 {e_dgi:.2e}")
    assert np.array_equal(bt(top), bt(reserve[L - 1]["out"]))
    assert e_out <= 2e-6 and e_dh <= 5e-7 and e_dgi <= 5e-7
    assert float(np.abs(dgi0).max()) > 1e-2 and float(np.abs(np.stack(dh)).max()) > 1e-2      # (not a comparison of zeros)


FLOOR_SHAPES = [(1, 5, 16, 32, 0.0), (3, 9, 17, 80, 0.3), (5, 12, 64, 128, 0.4), (2, 40, 33, 256, 0.2), (5, 6, 40, 768, 0.4)]


@pytest.mark.parametrize("L,T,B,H,p", FLOOR_SHAPES)
def test_float32_floor_is_positive_and_inside_the_caps(L, T, B, H, p):
    I, e32 = _case(L, T, B, H, p)
    s = G.standin(I)
    cap = G.caps(G.operand_forced(I, s))
    for k in G.KINDS:
        for l in range(L):
            print(f"[floor] ({L},{T},{B},{H},{p}) {k}[{l}]: e32 {e32[k][l]:.3e}  M e32 {G.M[k] * e32[k][l]:.3e}  cap {cap[k][l]:.3e}")
            assert 0 < e32[k][l] and G.M[k] * e32[k][l] <= cap[k][l], (k, l)
    # the stand-in at fp64 sits on the oracle: what e32 measures is float32 roundoff, not a difference between the two restatements
    s64 = G.standin(I, dtype=np.float64)
    e64 = G.max_errors(s64, G.operand_forced(I, s64))
    assert max(max(v) for v in e64.values()) <= 1e-13


def _refused_by_the_free_running_tolerance(L, s, ref):
    """The tensor kinds on which the assertions of tests/test_gpu_wave.py _check_wavefront (free-running comparison) fail."""
    outs, _, res, dG_ref, dh_ref = ref
    bad = set()
    for l in range(L):
        tol = 3e-3 * (1 + l)
        if np.abs(s["out"][l] - outs[l]).max() > tol: bad.add("out")
        if np.abs(s["res"][l] - G.stack_reserve(res[l])).max() > tol: bad.add("res")
        if np.abs(s["dG"][l] - dG_ref[l]).max() > 3e-3 * L * max(1.0, float(np.abs(dG_ref[l]).max())): bad.add("dG")
        if np.abs(s["dh_init"][l] - dh_ref[l]).max() > 3e-3 * L * max(1.0, float(np.abs(dh_ref[l]).max())): bad.add("dh_init")
    return bad


# (shape, mutations, the tensor kinds on which the free-running tolerance refuses each).  The three the free-running comparison was
# measured to let through come first: carry_unrounded passes it whole at every shape; dr_without_bias (wrong by 50 - 90 % of the
# signal's rms) passes it whole at (5, 25, 64, 512) and on dG everywhere (0.8e-2 ... 1.3e-2 against 1.5e-2; only dh_init of the
# bottom layers gives it away at the smaller shapes); truncate passes on both gradients and is refused on out / reserve of the
# bottom layer by a factor 1.4 ... 3.  The operand-forced bound refuses every one by >= 4 x.
_ALL = {"dr_without_bias": {"dh_init"}, "carry_unrounded": set(), "truncate": {"out", "res"}, "dz_zero": {"dG", "dh_init"},
        "dz_stale_h": {"dG", "dh_init"}, "ghn_saved_without_bias": {"res", "dh_init"}, "wrong_mask": {"dG", "dh_init"},
        "swap_z": {"out", "res", "dG", "dh_init"}}
MUTATION_CASES = [((3, 9, 17, 80, 0.3), _ALL), ((5, 12, 64, 128, 0.4), _ALL), ((5, 25, 64, 512, 0.4), {"dr_without_bias": set()})]
assert set(_ALL) == set(G.MUTATIONS)


@pytest.mark.parametrize("shape,refused", MUTATION_CASES)
def test_every_mutation_is_caught_and_the_free_running_tolerance_misses_some(shape, refused):
    L = shape[0]
    I, e32 = _case(*shape)
    ref = G.free_running(I["gi0"], I["whh"], I["bhh"], I["wih"], I["bih"], I["h0"], I["masks"], I["dY"], I["dhl"])
    assert not _refused_by_the_free_running_tolerance(L, G.standin(I), ref)
    today = {}
    for m in refused:
        s = G.standin(I, mutate=m)
        err = G.max_errors(s, G.operand_forced(I, s))
        over = max(err[k][l] / (G.M[k] * e32[k][l]) for k in G.KINDS for l in range(L))
        today[m] = _refused_by_the_free_running_tolerance(L, s, ref)
        print(f"[mutation] {shape} {m}: {over:.1f} x the operand-forced bound; the free-running tolerance refuses {sorted(today[m])}")
        assert over >= 4.0, f"{m}: only {over:.2f} x the bound"
    assert today == refused
