"""The oracles of oracle/gru_bf16.py in the exact-fp32 regime (round = identity) on the CPU: what tests/test_gpu_gru_fp32_oracle.py
rests on.  (That without rounding the free-running recurrences are the pinned b2t_oracle is tests/test_gru_bf16_oracle_host.py's
tie test.)

  * floor: at every shape of the GPU file the float32 stand-in against the operand-forced oracle (e32) is positive and, times the
    project's M, inside the caps; the stand-in at fp64 sits on the oracle;
  * mutations: every regime-independent defect is >= 4 x over the bound on some tensor; matrix operands that lose their low 13
    mantissa bits (tf32-like) are on every tensor kind, those that lose 10 on both gradients;
  * drop-7: operands that lose their low 7 bits pass the sweeps' self-comparison tolerance 3e-6 max(1, |.|max)
    (tests/test_gpu_parity.py test_persistent_sweep_odd_shapes_match_step_launch) on dG and dh_init -- recorded here, so that the gap
    stays documented -- while the operand-forced bound refuses them on dh_init.
Figures: NOTES.md, "The operand-forced oracle on the exact-fp32 sweeps"."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gru_bf16 as G

SHAPES = list(G.FP32_SWEEP_SHAPES)
_cache = {}


def _case(T, B, H):
    """Inputs, clean stand-in and floor of a shape: computed once, shared, never modified."""
    key = (T, B, H)
    if key not in _cache:
        I = G.random_inputs(1, T, B, H, G.fp32_sweep_seed(T, B, H))
        s = G.standin(I, round=G.identity)
        _cache[key] = (I, s, G.max_errors(s, G.operand_forced(I, s, round=G.identity)))
    return _cache[key]


def _over(I, e32, s):
    """err / (M e32) of a stand-in's tensors per kind (one layer)."""
    err = G.max_errors(s, G.operand_forced(I, s, round=G.identity))
    return {k: err[k][0] / (G.M[k] * e32[k][0]) for k in G.KINDS}


def test_the_fp32_regime_leaves_the_bf16_one_alone():
    """Default arguments are the bf16 regime, bit for bit; identity is another one."""
    I = G.random_inputs(2, 3, 5, 32, seed=1)
    a, b, c = G.standin(I), G.standin(I, round=G.bf16_rne), G.standin(I, round=G.identity)
    for k in G.KINDS:
        for l in range(2):
            assert np.array_equal(a[k][l], b[k][l])
    assert not np.array_equal(a["out"][0], c["out"][0])
    assert G.floor_e32(I) == G.floor_e32(I, round=G.bf16_rne)
    assert G.floor_e32(I, round=G.identity) == G.max_errors(c, G.operand_forced(I, c, round=G.identity)) != G.floor_e32(I)
    fa, fb = G.operand_forced(I, a), G.operand_forced(I, a, round=G.bf16_rne)
    assert all(np.array_equal(fa[k][l], fb[k][l]) for k in G.KINDS for l in range(2))
    assert set(G.MUTATIONS_FP32) == (set(G.MUTATIONS) - {"truncate", "carry_unrounded"}) | set(G.PRECISION_MUTATIONS)
    with pytest.raises(AssertionError):
        G.standin(I, mutate="drop7")          # a precision mutation of the fp32 regime only
    with pytest.raises(AssertionError):
        G.standin(I, mutate="truncate", round=G.identity)
    x = np.array([1.0 + 2.0 ** -23, 1.0 + 2.0 ** -10, -3.0 - 2.0 ** -15], dtype=np.float32)
    assert np.array_equal(G.drop_low_bits(13)(x), np.array([1.0, 1.0 + 2.0 ** -10, -3.0], dtype=np.float32))
    assert np.array_equal(G.drop_low_bits(7)(x), np.array([1.0, 1.0 + 2.0 ** -10, -3.0 - 2.0 ** -15], dtype=np.float32))


@pytest.mark.parametrize("T,B,H", SHAPES)
def test_float32_floor_is_positive_and_inside_the_caps(T, B, H):
    I, s, e32 = _case(T, B, H)
    cap = G.caps(G.operand_forced(I, s, round=G.identity))
    for k in G.KINDS:
        print(f"[fp32 floor] ({T},{B},{H}) {k}: e32 {e32[k][0]:.3e}  M e32 {G.M[k] * e32[k][0]:.3e}  cap {cap[k][0]:.3e}")
        assert 0 < e32[k][0] and G.M[k] * e32[k][0] <= cap[k][0], k
    # the stand-in at fp64 sits on the oracle: what e32 measures is float32 roundoff, not a difference between the two restatements
    s64 = G.standin(I, dtype=np.float64, round=G.identity)
    e64 = G.max_errors(s64, G.operand_forced(I, s64, round=G.identity))
    assert max(max(v) for v in e64.values()) <= 1e-13


INDEPENDENT = ("dr_without_bias", "dz_zero", "dz_stale_h", "ghn_saved_without_bias", "swap_z")


@pytest.mark.parametrize("T,B,H", SHAPES)
def test_every_mutation_is_caught(T, B, H):
    """With T = 1 there is no h_{t-2} (dz_stale_h changes nothing) and dG[0] has no matrix product behind it (its carry is dh_last, its
    gates are read back from the reserve): those two are asked of the shapes with T >= 2 only, everything else of every shape."""
    I, _, e32 = _case(T, B, H)
    for m in INDEPENDENT:
        over = _over(I, e32, G.standin(I, mutate=m, round=G.identity))
        print(f"[fp32 mutation] ({T},{B},{H}) {m}: " + "  ".join(f"{k} {over[k]:.3g}" for k in G.KINDS) + "  x the bound")
        if m != "dz_stale_h" or T >= 2:
            assert max(over.values()) >= 4.0, f"{m}: only {max(over.values()):.2f} x the bound"
    for m, kinds in (("drop13", G.KINDS), ("drop10", ("dG", "dh_init"))):
        over = _over(I, e32, G.standin(I, mutate=m, round=G.identity))
        print(f"[fp32 mutation] ({T},{B},{H}) {m}: " + "  ".join(f"{k} {over[k]:.3g}" for k in G.KINDS) + "  x the bound")
        for k in kinds:
            if k != "dG" or T >= 2:
                assert over[k] >= 4.0, f"{m} {k}: only {over[k]:.2f} x the bound"


def test_wrong_mask_is_caught_in_the_fp32_regime_too():
    """The one mutation that needs three layers and dropout: at the bf16 host file's shape."""
    L, T, B, H, p = 3, 9, 17, 80, 0.3
    I = G.random_inputs(L, T, B, H, seed=L * 1000 + H + B)
    I["masks"] = G.bernoulli_masks(L, T, B, H, p, seed=7 + L + T)
    e32 = G.floor_e32(I, round=G.identity)
    s = G.standin(I, mutate="wrong_mask", round=G.identity)
    err = G.max_errors(s, G.operand_forced(I, s, round=G.identity))
    over = max(err[k][l] / (G.M[k] * e32[k][l]) for k in G.KINDS for l in range(L))
    print(f"[fp32 mutation] ({L},{T},{B},{H},{p}) wrong_mask: {over:.3g} x the bound")
    assert over >= 4.0


@pytest.mark.parametrize("T,B,H", SHAPES)
def test_drop7_passes_the_self_comparison_tolerance_on_the_gradients(T, B, H):
    """Matrix operands without their low 7 mantissa bits against the clean stand-in at the sweeps' present tolerance
    3e-6 max(1, |ref|max), and against the operand-forced bound.  Measured (NOTES.md): 0.09 - 0.37 of the tolerance on dG and
    0.31 - 0.65 on dh_init -- accepted; 2.7 - 6.4 x the operand-forced bound on dG (T >= 2) and 3.5 - 17 x on dh_init."""
    I, clean, e32 = _case(T, B, H)
    s = G.standin(I, mutate="drop7", round=G.identity)
    over = _over(I, e32, s)
    frac = {k: float(np.abs(s[k][0].astype(np.float64) - clean[k][0]).max()) / (3e-6 * max(1.0, float(np.abs(clean[k][0]).max()))) for k in G.KINDS}
    for k in G.KINDS:
        print(f"[fp32 drop7] ({T},{B},{H}) {k}: {frac[k]:.2f} of the 3e-6 tolerance, {over[k]:.2f} x the operand-forced bound")
    assert frac["dG"] <= 1.0 and frac["dh_init"] <= 1.0, "the self-comparison tolerance now refuses drop-7: update NOTES.md and this test"
    assert max(over.values()) > 1.0       # ... and the operand-forced bound does not accept it
