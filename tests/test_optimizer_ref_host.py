"""The float64 restatement of clip_grad_norm_ + AdamW that the optimizer's GPU tests (tests/test_gpu_optimizer.py) compare
b2t_grad_norm_clip_f32 / b2t_adamw_f32 with, the three error measures, and torch.optim.AdamW run on the same inputs -- in one
importable place, checked here on the CPU.

AdamW is a chain of roundings, so it is compared STEP-LOCALLY: the restatement starts from the fp32 state (p, exp_avg,
exp_avg_sq) an implementation itself had before the step, takes beta, lr, wd and eps as doubles and the gradient as
fp32(g * coef), and the implementation's state after the step is measured against it in units of what fp32 can resolve there
(u = 2^-24):

    parameter    u * (|p| + |update|)
    exp_avg      u * (|beta1 m| + |(1 - beta1) g|)
    exp_avg_sq   u * v_new

The largest such error of torch.optim.AdamW(foreach=False) in fp32 on the CPU is what the reference's own roundings do; the
GPU test bounds the kernel by 3 x that figure, measured on the same inputs in the same test.  lr, wd and eps cross the C ABI as
floats, so the doubles that name the same inputs are the fp32 values themselves (hyper32)."""
import math

import numpy as np
import pytest
import torch

U = 2.0 ** -24
CHUNK = 1024
BETA1, BETA2 = 0.9, 0.999
GROUP_BIAS, GROUP_DAY, GROUP_OTHER = 0, 1, 2

# (chunks, group, seg_day): seg_day -2 = frozen, -1 = no day, d >= 0 = a day layer's tensor of day d
SEGMENTS = [(1, GROUP_BIAS, -1), (2, GROUP_OTHER, -1), (5, GROUP_OTHER, -1), (1, GROUP_DAY, 0), (1, GROUP_DAY, 1),
            (2, GROUP_DAY, 2), (1, GROUP_DAY, 3), (3, GROUP_DAY, 4), (1, GROUP_BIAS, -2), (4, GROUP_OTHER, -1),
            (1, GROUP_DAY, 0), (2, GROUP_BIAS, -1)]
# the day index of every sentence of the six steps' batches: days 0..4, of which each batch holds only some
BATCHES = [[0, 0, 2, 4, 2], [1], [3, 3, 3], [4, 0, 4, 1], [2, 2, 0], [1, 4, 3, 0, 2, 1]]


def hyper32(x):
    """The double that equals the fp32 value the C ABI receives."""
    return float(np.float32(x))


LR3 = [hyper32(0.005), hyper32(0.0025), hyper32(0.01)]     # bias, day, other
WD3 = [0.0, hyper32(0.001), hyper32(0.01)]                  # bias weight decay 0


def active_of(seg_day, day_idx):
    """The definition b2t_opt_prepare implements: frozen 0, no day 1, a day's tensor 1 iff that day is in the batch."""
    days = set(int(d) for d in day_idx)
    return np.array([0 if d == -2 else 1 if d == -1 else int(d in days) for d in seg_day], dtype=np.int32)


def seg_sizes():
    """Elements of every segment: the last chunk of most is partly padding (the arena pads each tensor to 1024 floats)."""
    return [c * CHUNK - (0 if i == 0 else (37 * i * i) % 1000) for i, (c, _, _) in enumerate(SEGMENTS)]


def problem(seed=11):
    """Initial parameters and six steps of gradients (magnitudes log-uniform over 1e-3 .. 10, both signs, none zero) per segment.

    |p| starts in [0.25, 1]: the parameter's unit u (|p| + |update|) does not see a cancellation between beta1 m and
    (1 - beta1) g, after which the rounding of exp_avg (some u of |beta1 m| + |(1 - beta1) g|, times lr / denom) is many u of
    the small update left over.  With |p| at least 25 x lr, and six updates of at most a few lr each, |p| resolves it for
    every element; with parameters around zero, one element in 10^4 carries torch's own figure from 2.5 to 10 u."""
    rng = np.random.default_rng(seed)
    sizes = seg_sizes()
    p0 = [(rng.choice([-1.0, 1.0], n) * rng.uniform(0.25, 1.0, n)).astype(np.float32) for n in sizes]
    grads = [[(rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-3.0, 1.0, n)).astype(np.float32) for n in sizes]
             for _ in BATCHES]
    return sizes, p0, grads


def clip_ref64(sumsq, max_norm):
    """(norm, coef) of clip_grad_norm_ evaluated in float64 from the exact sum of squares; max_norm <= 0: coef 1."""
    norm = math.sqrt(float(sumsq))
    coef = min(1.0, hyper32(max_norm) / (norm + 1e-6)) if max_norm > 0 else 1.0
    return norm, coef


def adamw_ref64(p, g, m, v, k, lr, wd, eps, beta1=BETA1, beta2=BETA2):
    """One AdamW step in float64 from the fp32 state (p, m, v) before it; g = the clipped fp32 gradient, k = the 1-based step
    count (scalar or per element).  Returns the new (p, m, v) and the three units the errors are measured in."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    k = np.asarray(k, dtype=np.float64)
    bm, gm = beta1 * m, (1.0 - beta1) * g
    m_new = bm + gm
    v_new = beta2 * v + (1.0 - beta2) * g * g
    update = lr / (1.0 - beta1 ** k) * m_new / (np.sqrt(v_new) / np.sqrt(1.0 - beta2 ** k) + eps)
    p_new = p * (1.0 - lr * wd) - update
    units = (U * (np.abs(p) + np.abs(update)), U * (np.abs(bm) + np.abs(gm)), U * v_new)
    return (p_new, m_new, v_new), units


def err_units(got, ref, units):
    """Largest error of each of (p, exp_avg, exp_avg_sq) in its unit."""
    out = []
    for a, r, un in zip(got, ref, units):
        assert (un > 0).all(), "a unit of zero: the inputs must keep every quantity away from 0"
        out.append(float((np.abs(np.asarray(a, dtype=np.float64) - r) / un).max()))
    return np.array(out)


class TorchAdamW:
    """torch.optim.AdamW(foreach=False) in fp32 on the CPU over the segments, one param group per (lr, wd); step() applies the
    given clipped gradients (None: the tensor has no gradient this step, as for a day absent from the batch) and returns the
    step-local figures of the tensors that moved."""

    def __init__(self, p0, groups, lr3, wd3, eps):
        self.params = [torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=np.float32))) for p in p0]
        self.groups, self.lr3, self.wd3, self.eps = list(groups), list(lr3), list(wd3), eps
        self.opt = torch.optim.AdamW(
            [dict(params=[q for q, g in zip(self.params, groups) if g == gi], lr=lr3[gi], weight_decay=wd3[gi]) for gi in range(3)],
            betas=(BETA1, BETA2), eps=eps, foreach=False)

    def steps(self):
        return [int(self.opt.state[q]["step"]) if q in self.opt.state and "step" in self.opt.state[q] else 0 for q in self.params]

    def moments(self, i):
        st = self.opt.state.get(self.params[i], {})
        z = np.zeros(self.params[i].shape, dtype=np.float32)
        return (st["exp_avg"].numpy().copy() if "exp_avg" in st else z, st["exp_avg_sq"].numpy().copy() if "exp_avg_sq" in st else z)

    def step(self, grads):
        before = [(q.detach().numpy().copy(),) + self.moments(i) for i, q in enumerate(self.params)]
        k0 = self.steps()
        for q, g in zip(self.params, grads):
            q.grad = None if g is None else torch.from_numpy(np.array(g, dtype=np.float32))
        self.opt.step()
        worst = np.zeros(3)
        for i, (q, g) in enumerate(zip(self.params, grads)):
            if g is None:
                assert np.array_equal(q.detach().numpy(), before[i][0]) and self.steps()[i] == k0[i]
                continue
            gi = self.groups[i]
            ref, units = adamw_ref64(before[i][0], g, before[i][1], before[i][2], k0[i] + 1, self.lr3[gi], self.wd3[gi], self.eps)
            worst = np.maximum(worst, err_units((q.detach().numpy(),) + self.moments(i), ref, units))
        return worst


@pytest.mark.parametrize("eps", [0.1, 1e-8])
def test_torch_adamw_within_a_few_u_of_the_restatement(eps):
    """Three param groups with different lr / wd, six steps with days absent from some batches: torch's own fp32 roundings stay
    below 8 u of the float64 restatement in every unit, and its per-tensor step counts are the number of batches that held the
    tensor's day."""
    sizes, p0, grads = problem()
    seg_day = [d for _, _, d in SEGMENTS]
    tw = TorchAdamW(p0, [g for _, g, _ in SEGMENTS], LR3, WD3, hyper32(eps))
    worst, count = np.zeros(3), np.zeros(len(SEGMENTS), dtype=np.int64)
    for day_idx, gs in zip(BATCHES, grads):
        act = active_of(seg_day, day_idx)
        coef = np.float32(clip_ref64(sum(float(np.sum(g.astype(np.float64) ** 2)) for g, a in zip(gs, act) if a), 200.0)[1])
        assert coef < 1
        worst = np.maximum(worst, tw.step([g * coef if a else None for g, a in zip(gs, act)]))
        count += act
    print("torch.optim.AdamW, eps %g: p %.2f u, exp_avg %.2f u, exp_avg_sq %.2f u" % ((eps,) + tuple(worst)))
    assert np.isfinite(worst).all() and (worst > 0).all() and (worst < 8).all(), worst
    assert tw.steps() == count.tolist() and len(set(count.tolist())) >= 4


def test_restatement_is_adamw():
    """The restatement against the textbook update written out per element in Python floats, and the step count per element."""
    rng = np.random.default_rng(5)
    p, g, m = (rng.standard_normal(7).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal(7) ** 2).astype(np.float32)
    k = np.array([1, 2, 3, 4, 5, 6, 40])
    (pn, mn, vn), units = adamw_ref64(p, g, m, v, k, 0.005, 0.01, 0.1)
    for i in range(7):
        mi = 0.9 * float(m[i]) + 0.1 * float(g[i])
        vi = 0.999 * float(v[i]) + 0.001 * float(g[i]) ** 2
        up = 0.005 * (mi / (1 - 0.9 ** int(k[i]))) / (math.sqrt(vi / (1 - 0.999 ** int(k[i]))) + 0.1)
        assert abs(mn[i] - mi) <= 1e-15 * abs(mi) and abs(vn[i] - vi) <= 1e-15 * vi
        assert abs(pn[i] - (float(p[i]) * (1 - 0.005 * 0.01) - up)) <= 1e-14 * (abs(float(p[i])) + abs(up))
        assert abs(units[0][i] - U * (abs(float(p[i])) + abs(up))) <= 1e-14 * units[0][i]


def test_clip_and_active_definitions():
    assert clip_ref64(9.0, 0.0) == (3.0, 1.0) and clip_ref64(9.0, 6.0) == (3.0, 1.0)
    assert clip_ref64(16.0, 2.0)[1] == 2.0 / (4.0 + 1e-6)
    assert active_of([-2, -1, 0, 3, 4], [3, 3, 0]).tolist() == [0, 1, 1, 1, 0]
    assert active_of([-2, -1, 0, 3], [7]).tolist() == [0, 1, 0, 0]
