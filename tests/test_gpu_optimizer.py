"""b2t_opt_prepare / b2t_grad_norm_clip_f32 / b2t_opt_advance / b2t_adamw_f32 (csrc/optimizer.hip) on the MI355X, each driven
directly through the C ABI over an arena built by hand: about a dozen segments of 1..5 chunks, padded to 1024 floats, of all
three groups, with frozen (seg_day -2), day-less (-1) and day tensors (0..4) of which a batch holds only some.

What can be exact is asserted as equality (the active flags, the step counters, the sum of squares of integer gradients, the
clipped gradient fp32(g coef), untouched tensors bit for bit).  AdamW itself is a chain of roundings and is compared step-locally
with the float64 restatement of tests/test_optimizer_ref_host.py in the units defined there; the bound is 3 x what
torch.optim.AdamW(foreach=False) in fp32 on the CPU shows against the same restatement on the same inputs, measured in the same
test (the measured ratios are in NOTES.md 2c).  Buffers as in tests/test_gpu_elementwise.py: fresh for every call,
exactly the documented size, canaries behind each, workspaces 0xFF."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_elementwise import Buf, lib_and_stream, ok
from test_optimizer_ref_host import (BATCHES, BETA1, BETA2, CHUNK, LR3, SEGMENTS, WD3, TorchAdamW, active_of, adamw_ref64,
                                     clip_ref64, err_units, hyper32, problem)

pytestmark = pytest.mark.gpu


class Arena:
    """The tables of a flat arena: segment s is chunks[s] chunks of 1024 floats; chunk2seg, seg_group, seg_day."""

    def __init__(self, segments):
        self.chunks = [c for c, _, _ in segments]
        self.seg_group = np.array([g for _, g, _ in segments], dtype=np.int32)
        self.seg_day = np.array([d for _, _, d in segments], dtype=np.int32)
        self.nseg, self.nchunks = len(segments), sum(self.chunks)
        self.chunk2seg = np.repeat(np.arange(self.nseg, dtype=np.int32), self.chunks)
        self.off = np.concatenate([[0], np.cumsum(self.chunks)]) * CHUNK
        self.n = self.nchunks * CHUNK

    def seg(self, a, s):
        return a[self.off[s]:self.off[s + 1]]

    def pack(self, parts):
        """Per-segment arrays (shorter than the padded segment: zeros behind) -> one arena."""
        a = np.zeros(self.n, dtype=np.float32)
        for s, x in enumerate(parts):
            a[self.off[s]:self.off[s] + len(x)] = x
        return a

    def mask(self, per_seg):
        """A per-segment flag spread over the arena's elements."""
        return np.repeat(np.asarray(per_seg), np.array(self.chunks) * CHUNK)


def sized(nchunks):
    """The dozen segments with the third one stretched so that the arena has nchunks chunks (nchunks 1: a single segment)."""
    if nchunks == 1:
        return Arena([(1, 2, -1)])
    segs = list(SEGMENTS)
    segs[2] = (nchunks - (sum(c for c, _, _ in segs) - segs[2][0]), segs[2][1], segs[2][2])
    return Arena(segs)


def int_grads(ar, active, seed):
    """Integer gradients in [-8, 8]; tensors without a gradient hold NaN, which must not reach the norm."""
    g = np.random.default_rng(seed).integers(-8, 9, ar.n).astype(np.float32)
    g[ar.mask(active) == 0] = np.nan
    return g


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- one fresh-buffered call per entry point -------------------------------------------------------------------------------
def opt_prepare(day_idx, seg_day):
    lib, st = lib_and_stream()
    bd, bs, ba = Buf(np.array(day_idx, dtype=np.int32)), Buf(np.asarray(seg_day, dtype=np.int32)), Buf(4 * len(seg_day), np.int32)
    ok(lib.b2t_opt_prepare(bd.ptr, len(day_idx), bs.ptr, len(seg_day), ba.ptr, st))
    return ba.get().copy()


def grad_norm_clip(ar, g, active, max_norm, seg_step=None, status0=0.0, err=None):
    """-> (out4, seg_step after the call or None).  err = (words, n_err, err_stride)."""
    lib, st = lib_and_stream()
    bg, bc, ba = Buf(g), Buf(ar.chunk2seg), Buf(np.asarray(active, dtype=np.int32))
    ws, bo = Buf(4 * ar.nchunks), Buf(np.array([-1.0, -1.0, -1.0, status0], dtype=np.float32))
    bs = Buf(np.asarray(seg_step, dtype=np.int32)) if seg_step is not None else None
    be = Buf(np.asarray(err[0], dtype=np.uint32)) if err is not None else None
    ok(lib.b2t_grad_norm_clip_f32(bg.ptr, bc.ptr, ba.ptr, ar.nchunks, max_norm, ws.ptr, bo.ptr, bs.ptr if bs else None, ar.nseg,
                                  be.ptr if be else None, err[1] if err else 0, err[2] if err else 0, st))
    ws.get()
    assert np.array_equal(bits(bg.get()), bits(g)), "the norm must not write the gradients"
    return bo.get().copy(), (bs.get().copy() if bs else None)


def opt_advance(active, seg_step, out4):
    lib, st = lib_and_stream()
    ba, bs, bo = Buf(np.asarray(active, dtype=np.int32)), Buf(np.asarray(seg_step, dtype=np.int32)), Buf(np.asarray(out4, dtype=np.float32))
    ok(lib.b2t_opt_advance(ba.ptr, bs.ptr, len(active), bo.ptr, st))
    return bs.get().copy()


def adamw(ar, p, g, m, v, active, seg_step, clip4, apply_clip, eps, lr3=LR3, wd3=WD3):
    lib, st = lib_and_stream()
    bufs = [Buf(a) for a in (p, g, m, v)]
    bc, ba, bgp, bs = Buf(ar.chunk2seg), Buf(np.asarray(active, dtype=np.int32)), Buf(ar.seg_group), Buf(np.asarray(seg_step, dtype=np.int32))
    b4 = Buf(np.asarray(clip4, dtype=np.float32)) if clip4 is not None else None
    ok(lib.b2t_adamw_f32(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, bc.ptr, ba.ptr, bgp.ptr, bs.ptr, ar.nchunks,
                         b4.ptr if b4 else None, apply_clip, (C.c_float * 3)(*lr3), (C.c_float * 3)(*wd3), BETA1, BETA2, eps, st))
    for b in (bc, ba, bgp, bs) + ((b4,) if b4 else ()):
        b.get()
    return [b.get().copy() for b in bufs]


# ---- 1. opt_prepare ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("day_idx", BATCHES + [[4], [2, 2, 2, 2], [7, 9]], ids=lambda d: "days_" + "_".join(map(str, d)))
def test_opt_prepare_is_the_definition(day_idx):
    """active = 0 for a frozen tensor, 1 for one without a day, and for a day's tensor whether the batch holds that day: batches
    with repeated days, of one day, of one sentence, and of days no tensor has."""
    ar = Arena(SEGMENTS)
    got = opt_prepare(day_idx, ar.seg_day)
    assert got.tolist() == active_of(ar.seg_day, day_idx).tolist()
    assert not got[ar.seg_day == -2].any() and got[ar.seg_day == -1].all()


# ---- 2. grad_norm_clip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_norm", [0.0, 10.0, 1.0e6])
@pytest.mark.parametrize("nchunks", [1, 3073, 5000])
def test_grad_norm_clip_integer_gradients(nchunks, max_norm):
    """Integer gradients: out4[0] is fp32(the exact integer sum of squares) whatever the order of the sums, norm and coefficient
    are within one fp32 ulp of the float64 evaluation; 1, 3073 and 5000 partials take the four-chain loop of the final kernel
    through no round, one round, and one round plus the tail; max_norm 0 (coef exactly 1), one that clips, one that does not.
    Tensors without a gradient hold NaN.  The step counters advance by exactly `active`; with seg_step NULL b2t_opt_advance
    does the same afterwards."""
    ar = sized(nchunks)
    assert ar.nchunks == nchunks
    active = active_of(ar.seg_day, [0, 2, 2])
    g = int_grads(ar, active, nchunks)
    step0 = np.arange(ar.nseg, dtype=np.int32) * 3 + 1
    out4, step1 = grad_norm_clip(ar, g, active, max_norm, seg_step=step0)
    exact = int((g[~np.isnan(g)].astype(np.int64) ** 2).sum())
    assert out4[0] == np.float32(exact) and out4[3] == 0.0
    norm, coef = clip_ref64(exact, max_norm)
    print("sumsq %d norm %.9g (ref %.9g) coef %.9g (ref %.9g)" % (exact, out4[1], norm, out4[2], coef))
    assert abs(float(out4[1]) - norm) <= np.spacing(np.float32(norm))
    assert abs(float(out4[2]) - coef) <= np.spacing(np.float32(coef))
    if max_norm == 0.0 or max_norm == 1.0e6:
        assert out4[2] == 1.0
    else:
        assert out4[2] < 1.0
    assert step1.tolist() == (step0 + active).tolist()
    out4n, none = grad_norm_clip(ar, g, active, max_norm, seg_step=None)
    assert none is None and np.array_equal(bits(out4n), bits(out4))
    assert opt_advance(active, step0, out4n).tolist() == (step0 + active).tolist()


# ---- 3. the status word ---------------------------------------------------------------------------------------------------------
ERR_N, ERR_STRIDE = 3, 5
ERR_CLEAR = np.zeros((ERR_N - 1) * ERR_STRIDE + 1, dtype=np.uint32)
ERR_LAST = ERR_CLEAR.copy()
ERR_LAST[-1] = 0x80000000
ERR_BETWEEN = np.full_like(ERR_CLEAR, 7)      # set words that are none of the three
ERR_BETWEEN[::ERR_STRIDE] = 0


@pytest.mark.parametrize("name,inf_grad,err,status0,want", [
    ("ok_words_between_set", False, ERR_BETWEEN, 0.0, 0.0),
    ("inf_gradient", True, ERR_CLEAR, 0.0, 2.0),
    ("inf_gradient_no_words", True, None, 0.0, 2.0),
    ("last_error_word", False, ERR_LAST, 0.0, 1.0),
    ("both", True, ERR_LAST, 0.0, 1.0),
    ("preset_1", False, ERR_CLEAR, 1.0, 1.0),
    ("preset_2", False, ERR_CLEAR, 2.0, 2.0),
    ("preset_2_and_error_word", False, ERR_LAST, 2.0, 2.0),
])
def test_status_word(name, inf_grad, err, status0, want):
    """status 2 for a non-finite norm, 1 for a set error word (three words five apart, only the last set; words between them are
    not read), 1 when both, a preset status stays.  A bad step is never applied: the counters are bit-unchanged, b2t_opt_advance
    changes nothing, b2t_adamw_f32 leaves p, g, m, v as they were; the good step beside them moves all of it."""
    ar = Arena(SEGMENTS)
    rng = np.random.default_rng(3)
    active = active_of(ar.seg_day, [1, 3])
    g = int_grads(ar, active, 17)
    if inf_grad:
        g[ar.off[9] + 1500] = np.inf
    step0 = np.arange(ar.nseg, dtype=np.int32) + 2
    out4, step1 = grad_norm_clip(ar, g, active, 10.0, seg_step=step0, status0=status0,
                                 err=None if err is None else (err, ERR_N, ERR_STRIDE))
    assert out4[3] == want
    p, m = rng.standard_normal(ar.n).astype(np.float32), rng.standard_normal(ar.n).astype(np.float32)
    v = (rng.standard_normal(ar.n) ** 2).astype(np.float32)
    after = adamw(ar, p, g, m, v, active, step1, out4, 1, hyper32(0.1))
    if want == 0.0:
        assert step1.tolist() == (step0 + active).tolist()
        assert opt_advance(active, step0, out4).tolist() == (step0 + active).tolist()
        moved = ar.mask(active) == 1
        assert all((bits(a)[moved] != bits(b)[moved]).mean() > 0.9 for a, b in zip(after, (p, g, m, v)))
    else:
        assert np.array_equal(step1, step0)
        assert np.array_equal(opt_advance(active, step0, out4), step0)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(after, (p, g, m, v)))


# ---- 4. adamw: what is exact -----------------------------------------------------------------------------------------------------
def test_adamw_one_step_exact_parts():
    """After the call g is exactly fp32(g coef); tensors without a gradient and frozen ones, filled with NaN, are bit-unchanged
    in all four arrays; apply_clip = 0 and clip4 = NULL use coef 1 (g stays, and both give the bits of an applied coefficient of
    exactly 1.0); the padding behind every tensor stays zero."""
    ar = Arena(SEGMENTS)
    sizes, p0, grads = problem()
    active = active_of(ar.seg_day, BATCHES[0])
    off = ar.mask(active) == 0
    p, g = ar.pack(p0), ar.pack(grads[0])
    m = ar.pack([0.1 * x for x in grads[1]])
    v = ar.pack([x * x for x in grads[2]])
    for a in (p, g, m, v):
        a[off] = np.nan
    out4, step1 = grad_norm_clip(ar, g, active, 200.0, seg_step=np.full(ar.nseg, 2, dtype=np.int32))
    assert 0.0 < out4[2] < 1.0 and out4[3] == 0.0
    res = {}
    for key, clip4, apply_clip in (("clip", out4, 1), ("noapply", out4, 0), ("null", None, 1)):
        res[key] = adamw(ar, p, g, m, v, active, step1, clip4, apply_clip, hyper32(0.1))
        for a, b in zip(res[key], (p, g, m, v)):
            assert np.array_equal(bits(a)[off], bits(b)[off]), key
    assert np.array_equal(bits(res["clip"][1])[~off], bits(g[~off] * np.float32(out4[2])))
    assert np.array_equal(bits(res["noapply"][1]), bits(g)) and np.array_equal(bits(res["null"][1]), bits(g))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(res["noapply"], res["null"]))
    assert not np.array_equal(bits(res["clip"][0]), bits(res["null"][0]))
    pad = np.ones(ar.n, dtype=bool)
    for s, n in enumerate(sizes):
        pad[ar.off[s]:ar.off[s] + n] = False
    pad &= ~off
    assert pad.sum() > 1000 and all(not a[pad].any() for a in res["clip"])
    # coef 1 by either route is the coefficient 1.0 that max_norm 0 writes, applied: the path the next test measures
    one4, _ = grad_norm_clip(ar, g, active, 0.0)
    assert one4[2] == 1.0
    res["one"] = adamw(ar, p, g, m, v, active, step1, one4, 1, hyper32(0.1))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(res["one"], res["null"]))


# ---- 5. adamw: six steps, step-local, against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.1, 1e-8])
def test_adamw_six_steps_against_fp64(eps):
    """Six steps of prepare -> norm + clip -> AdamW with days absent from some batches, three groups of different lr and wd (bias
    wd 0), gradients over 1e-3 .. 10: every step's p, exp_avg, exp_avg_sq against the float64 restatement started from the
    kernel's own state before that step, largest error in u (|p| + |update|), u (|beta1 m| + |(1 - beta1) g|), u v_new, at most
    3 x the same figure of torch.optim.AdamW(foreach=False) in fp32 on the CPU on the same inputs; eps 0.1 (shipped) and 1e-8
    (where exp_avg_sq decides the step).  The per-tensor step counts equal torch's state['step'] after every step."""
    ar = Arena(SEGMENTS)
    sizes, p0, grads = problem()
    eps = hyper32(eps)
    tw = TorchAdamW(p0, ar.seg_group, LR3, WD3, eps)
    p, m, v = ar.pack(p0), np.zeros(ar.n, dtype=np.float32), np.zeros(ar.n, dtype=np.float32)
    seg_step = np.zeros(ar.nseg, dtype=np.int32)
    worst, worst_t = np.zeros(3), np.zeros(3)
    for it, (day_idx, gs) in enumerate(zip(BATCHES, grads)):
        active = opt_prepare(day_idx, ar.seg_day)
        assert active.tolist() == active_of(ar.seg_day, day_idx).tolist()
        g = ar.pack(gs)
        g[ar.mask(active) == 0] = np.nan
        out4, seg_step = grad_norm_clip(ar, g, active, 200.0, seg_step=seg_step)
        assert 0.0 < out4[2] < 1.0 and out4[3] == 0.0
        p1, g1, m1, v1 = adamw(ar, p, g, m, v, active, seg_step, out4, 1, eps)
        tgrads = []
        for s, n in enumerate(sizes):
            if not active[s]:
                tgrads.append(None)
                assert all(np.array_equal(bits(ar.seg(a, s)), bits(ar.seg(b, s))) for a, b in zip((p1, m1, v1), (p, m, v)))
                continue
            gc = gs[s] * np.float32(out4[2])
            assert np.array_equal(ar.seg(g1, s)[:n], gc)
            tgrads.append(gc)
            grp = ar.seg_group[s]
            ref, units = adamw_ref64(ar.seg(p, s)[:n], gc, ar.seg(m, s)[:n], ar.seg(v, s)[:n], int(seg_step[s]), LR3[grp], WD3[grp], eps)
            worst = np.maximum(worst, err_units([ar.seg(a, s)[:n] for a in (p1, m1, v1)], ref, units))
        worst_t = np.maximum(worst_t, tw.step(tgrads))
        assert seg_step.tolist() == tw.steps(), (it, seg_step, tw.steps())
        p, m, v = p1, m1, v1
    assert len(set(seg_step.tolist())) >= 4 and seg_step.max() == 6 and seg_step[ar.seg_day == -2].max() == 0
    ratio = worst / worst_t
    print("AdamW eps %g: kernel p %.2f exp_avg %.2f exp_avg_sq %.2f u | torch %.2f %.2f %.2f u | ratios %.2f %.2f %.2f"
          % ((eps,) + tuple(worst) + tuple(worst_t) + tuple(ratio)))
    assert np.isfinite(worst).all() and (worst_t > 0).all()
    assert (worst <= 3.0 * worst_t).all(), (worst, worst_t, ratio)
