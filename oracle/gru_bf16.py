"""CPU restatements of the bf16-mode GRU sweeps (the layer wavefront csrc/gru_wave.hip / gru_wave_ks.h and the bf16 persistent
sweep csrc/gru_persistent.hip with GRU_BF16): every matrix-core operand rounded to bf16 (RNE), fp32 everywhere else.

THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE (see oracle/b2t_oracle.py).  Three restatements of the same recurrences:

  free_running     fp64, operands rounded where the recurrence itself produces them.  A rounding that flips between a kernel's
                   fp32 and this fp64 moves an operand by 2^-9 and everything downstream with it: comparisons against it are
                   loose by construction (about 1e-3).
  operand_forced   fp64, every matrix operand the bf16 rounding of the tensor the KERNEL wrote (out / outd / dG); the elementwise
                   inputs of a step (h_{t-1}, the saved gates) the kernel's too.  No flips: what is left between a correct kernel
                   and this oracle is fp32 roundoff (1e-7 on the states and gates, 1e-8 on the gradients), independent of T.
                   Every step is checked against the true cell function of the inputs the kernel really had; a kernel that passes
                   every step is right by induction, and a stale hand-off shows because the saved gates then belong to another h
                   than the one in `out`.
  standin          the recurrences in float32 (numpy) with bf16 operands, in the kernels' tensor layout: stands in for a kernel on
                   the CPU, measures the fp32 floor e32 of the operand-forced comparison, and carries the deliberate defects
                   (`mutate`) that show what a bound lets through.

Layout (all time-major): gi0 [T,B,3H] (layer 0's input projection, b_ih[0] included); whh[l] [3H,H]; bhh[l] [3H]; wih[l] [3H,H]
and bih[l] [3H] for l >= 1 (index 0 is None); h0[l] [B,H]; masks None or L - 1 arrays [T,B,H] of keep / (1 - p) factors on out[l];
dY [T,B,H] (gradient wrt the top layer's outputs); dhl None or [L,B,H].  Gate order r, z, n; reserve = (r, z, n, gh_n) [T,B,4H];
dG = (dr_pre, dz_pre, dn_pre r, dn_pre) [T,B,4H] as gru_gate_bwd of csrc/gru_cell.h writes it.

The operand rounding is a parameter (`round`, bf16_rne by default).  round = identity gives the same three restatements of the
EXACT-FP32 sweeps (csrc/gru.hip step-launch, csrc/gru_persistent.hip without GRU_BF16, and the fused forward): only the operand
rounding differs between the regimes, M and the caps are the same.  tests/test_gru_fp32_oracle_host.py, tests/test_gpu_gru_fp32_oracle.py.
"""
from __future__ import annotations

import numpy as np

KINDS = ("out", "res", "dG", "dh_init")

# The kernels pass when max |kernel - operand_forced(kernel's tensors)| <= M[kind] * e32[kind][layer], e32 the same figure of the
# float32 stand-in at the same inputs (restatement against restatement).  M = 4 x the largest ratio measured on the MI355X over
# every case of tests/test_gpu_wave.py and test_persistent_sweep_bf16_operands (out / reserve 2.18, dG 1.50, dh_init 1.37), rounded
# up to a power of two: the table is in NOTES.md, "The operand-forced bf16 GRU oracle".  `out` and `reserve` share one constant.
M = {"out": 16.0, "res": 16.0, "dG": 8.0, "dh_init": 8.0}
# ... and M * e32 may never exceed these (asserted before every comparison, so that the bound cannot quietly become loose):
CAP_ABS = 1e-4          # out, reserve: 30 x below the free-running comparison's tightest tolerance
CAP_RMS = 1e-3          # dG, dh_init: times the rms of the oracle's tensor


# (T, B, H) of the exact-fp32 sweeps' tests, one layer per launch (host and GPU file share them): the smallest shapes that reach
# every template instance of csrc/gru_persistent.hip's launchers (NCH / NCB = K chunks per wave, forward / backward) and every edge.
FP32_SWEEP_SHAPES = ((3, 1, 16),       # one row, one workgroup column
                     (1, 17, 80),      # T = 1: no hand-off, the backward carry is dh_last alone
                     (2, 5, 48),       # H % 32 != 0: a cache line holds rows of two steps
                     (4, 17, 128),     # NCH 2 / NCB 6 at their upper edge
                     (5, 33, 160),     # NCH 4 / NCB 12, three row groups ...
                     (4, 16, 256),     # ... and exactly one, at the upper edge
                     (9, 33, 272),     # NCH 8 / NCB 24 just past 256
                     (6, 64, 512),     # four full row groups; the XCD-local hand-off and the 32-unit workgroups are eligible
                     (4, 70, 768),     # NCH 12 / NCB 36; B > 64: the XCD-local hand-off is refused
                     (3, 17, 1024))    # NCH 16 / NCB 48
fp32_sweep_seed = lambda T, B, H: B * 1000 + H


def identity(x):
    return np.asarray(x, dtype=np.float64)


def bf16_rne(x):
    """fp32 -> nearest-even bf16 -> fp32 (what v_cvt_pk_bf16_f32 does to the operands)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
    return ((u + r) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (a defect: the `truncate` mutation)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32)


def drop_low_bits(k):
    """fp32 with its low k mantissa bits cleared (a defect of the exact-fp32 regime: the `drop7` / `drop10` / `drop13` mutations;
    k = 13 leaves tf32's 10 mantissa bits)."""
    keep = np.uint32((0xFFFFFFFF << k) & 0xFFFFFFFF)
    return lambda x: (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & keep).view(np.float32)


def random_inputs(L, T, B, H, seed, with_dhl=True):
    """The operands of tests/test_gpu_wave.py's launches (torch generator, this order of draws), as float32 numpy arrays."""
    import torch
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).numpy()
    gi0 = rnd(T, B, 3 * H, sc=0.5)
    whh = [rnd(3 * H, H, sc=1.0 / H ** 0.5) for _ in range(L)]
    wih = [None] + [rnd(3 * H, H, sc=1.0 / H ** 0.5) for _ in range(L - 1)]
    bhh = [rnd(3 * H, sc=0.1) for _ in range(L)]
    bih = [None] + [rnd(3 * H, sc=0.1) for _ in range(L - 1)]
    h0 = [rnd(B, H, sc=0.3) for _ in range(L)]
    dY = rnd(T, B, H, sc=0.05)
    dhl = rnd(L, B, H, sc=0.05) if with_dhl else None
    return dict(gi0=gi0, whh=whh, bhh=bhh, wih=wih, bih=bih, h0=h0, masks=None, dY=dY, dhl=dhl)


def bernoulli_masks(L, T, B, H, p, seed):
    """Keep / (1 - p) factors for out[0 .. L-2] where no GPU is there to draw the Philox ones."""
    rng = np.random.default_rng(seed)
    return [(rng.random((T, B, H)) >= p).astype(np.float64) / (1.0 - p) for _ in range(L - 1)] if p > 0 and L > 1 else None


def free_running(gi0, whh, bhh, wih, bih, h0, masks, dY, dhl, round=bf16_rne):
    """fp64 recurrences with `round`-ed matrix operands.  Returns outs, outd, reserves, dG, dh_init."""
    rq = lambda x: round(x).astype(np.float64)
    L = len(whh)
    T, B, _ = gi0.shape
    H = whh[0].shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    outs, outd, res = [], [], []
    x = None
    for l in range(L):
        wq = rq(whh[l])
        gi = gi0.astype(np.float64) if l == 0 else rq(x.reshape(T * B, H)).reshape(T, B, H) @ rq(wih[l]).T + bih[l]
        h = h0[l].astype(np.float64)
        o, rs = [], []
        for t in range(T):
            gh = rq(h) @ wq.T + bhh[l]
            r = sig(gi[t][:, :H] + gh[:, :H]); z = sig(gi[t][:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gi[t][:, 2 * H:] + r * gh[:, 2 * H:])
            hp = h
            h = (1 - z) * n + z * hp
            o.append(h); rs.append((r, z, n, gh[:, 2 * H:], hp))
        o = np.stack(o)
        outs.append(o); res.append(rs)
        x = o * masks[l] if (masks and l < L - 1) else o
        outd.append(x)
    dG, dh_init = [None] * L, [None] * L
    dy = dY.astype(np.float64)
    for l in range(L - 1, -1, -1):
        wq = rq(whh[l])
        carry = dhl[l].astype(np.float64) if dhl is not None else np.zeros((B, H))
        g = np.zeros((T, B, 4 * H))
        for t in range(T - 1, -1, -1):
            r, z, n, ghn, hp = res[l][t]
            d = dy[t] + carry
            dn = d * (1 - z); dz = d * (hp - n)
            dn_pre = dn * (1 - n * n); dz_pre = dz * z * (1 - z); dr_pre = dn_pre * ghn * r * (1 - r)
            g[t] = np.concatenate([dr_pre, dz_pre, dn_pre * r, dn_pre], axis=1)
            carry = d * z + rq(g[t][:, :3 * H]) @ wq
        dG[l], dh_init[l] = g, carry
        if l > 0:
            dgi = np.concatenate([g[:, :, :2 * H], g[:, :, 3 * H:]], axis=2).reshape(T * B, 3 * H)
            dy = (rq(dgi) @ rq(wih[l])).reshape(T, B, H)
            if masks:
                dy = dy * masks[l - 1]
    return outs, outd, res, dG, dh_init


def stack_reserve(rs):
    """free_running's per-step tuples of one layer -> the kernels' reserve [T,B,4H]."""
    return np.stack([np.concatenate(s[:4], axis=1) for s in rs])


def _h_prev(h0_l, out_l):
    return np.concatenate([np.asarray(h0_l, dtype=np.float64)[None], np.asarray(out_l[:-1], dtype=np.float64)])


def operand_forced(inputs, kernel, round=bf16_rne):
    """The fp64 oracle driven by the tensors a kernel (or the stand-in) wrote: kernel = dict(out, outd, res, dG, dh_init), lists
    per layer of float32 arrays (outd is read only where inputs['masks'] is set; dh_init is not read at all).  `round`: what the
    kernel does to its matrix operands -- bf16_rne (written bf16() below) for the bf16 sweeps, identity for the exact-fp32 ones.

    Forward, layer l, step t (step-local): hp = kernel's out[l][t-1] (h0[l] at t = 0); gh = bf16(hp) W_hh^T + b_hh; gi = gi0 for
    layer 0, else bf16(kernel's outd[l-1][t]) W_ih^T + b_ih (out[l-1] without dropout); r, z, n, h in fp64 -> `out`, `res`.
    Backward, layer l from the top: the carry runs in fp64, its matrix product is bf16(kernel's dG[l][t][:, :3H]) bf16(W_hh); the
    saved gates and hp are the kernel's; the layer below gets dy = bf16(kernel's dG[l] columns (dr, dz, dn)) bf16(W_ih[l]) times
    masks[l-1] -> `dG`, `dh_init`.  Returns dict(out, res, dG, dh_init), lists per layer of fp64 arrays."""
    I = inputs
    q = lambda x: round(x).astype(np.float64)
    L = len(I["whh"])
    T, B, _ = I["gi0"].shape
    H = I["whh"][0].shape[1]
    masks = I["masks"]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    o_out, o_res = [], []
    for l in range(L):
        hp = _h_prev(I["h0"][l], kernel["out"][l])
        gh = (q(hp.reshape(T * B, H)) @ q(I["whh"][l]).T + I["bhh"][l]).reshape(T, B, 3 * H)
        if l == 0:
            gi = I["gi0"].astype(np.float64)
        else:
            x = kernel["outd"][l - 1] if masks else kernel["out"][l - 1]
            gi = (q(np.asarray(x).reshape(T * B, H)) @ q(I["wih"][l]).T + I["bih"][l]).reshape(T, B, 3 * H)
        r = sig(gi[..., :H] + gh[..., :H]); z = sig(gi[..., H:2 * H] + gh[..., H:2 * H])
        ghn = gh[..., 2 * H:]
        n = np.tanh(gi[..., 2 * H:] + r * ghn)
        o_out.append((1 - z) * n + z * hp)
        o_res.append(np.concatenate([r, z, n, ghn], axis=2))
        del gh, gi
    o_dG, o_dh = [None] * L, [None] * L
    dy = I["dY"].astype(np.float64)
    for l in range(L - 1, -1, -1):
        R = np.asarray(kernel["res"][l], dtype=np.float64)
        r, z, n, ghn = R[..., :H], R[..., H:2 * H], R[..., 2 * H:3 * H], R[..., 3 * H:]
        hp = _h_prev(I["h0"][l], kernel["out"][l])
        kdG = np.asarray(kernel["dG"][l])
        prod = (q(kdG[..., :3 * H].reshape(T * B, 3 * H)) @ q(I["whh"][l])).reshape(T, B, H)
        carry = I["dhl"][l].astype(np.float64) if I["dhl"] is not None else np.zeros((B, H))
        g = np.empty((T, B, 4 * H))
        for t in range(T - 1, -1, -1):
            d = dy[t] + carry
            dn_pre = d * (1 - z[t]) * (1 - n[t] * n[t])
            g[t, :, :H] = dn_pre * ghn[t] * r[t] * (1 - r[t])
            g[t, :, H:2 * H] = d * (hp[t] - n[t]) * z[t] * (1 - z[t])
            g[t, :, 2 * H:3 * H] = dn_pre * r[t]
            g[t, :, 3 * H:] = dn_pre
            carry = d * z[t] + prod[t]
        o_dG[l], o_dh[l] = g, carry
        if l > 0:
            dgi = np.concatenate([kdG[..., :2 * H], kdG[..., 3 * H:]], axis=2).reshape(T * B, 3 * H)
            dy = (q(dgi) @ q(I["wih"][l])).reshape(T, B, H)
            if masks:
                dy = dy * masks[l - 1]
        del R, prod, kdG
    return dict(out=o_out, res=o_res, dG=o_dG, dh_init=o_dh)


MUTATIONS = ("dr_without_bias",        # dr_pre built from gh_n without its bias
             "carry_unrounded",        # the dG operand of the carry product not rounded to bf16
             "truncate",               # matrix operands truncated to bf16 instead of RNE
             "dz_zero",                # dz_pre = 0
             "dz_stale_h",             # dz from h_{t-2} instead of h_{t-1}
             "ghn_saved_without_bias",  # gh_n saved in reserve without its bias
             "wrong_mask",             # the layer below's dy times another layer's mask (needs L >= 3 and dropout)
             "swap_z")                 # z and 1 - z swapped in h


# The exact-fp32 regime (round = identity): `truncate` and `carry_unrounded` change nothing there and are left out; what takes their
# place are matrix operands that silently lose their low mantissa bits (a reduced-precision matrix-core path taken by mistake).
PRECISION_MUTATIONS = {"drop7": 7, "drop10": 10, "drop13": 13}
MUTATIONS_FP32 = tuple(m for m in MUTATIONS if m not in ("truncate", "carry_unrounded")) + tuple(PRECISION_MUTATIONS)


def standin(inputs, dtype=np.float32, mutate=None, round=bf16_rne):
    """The recurrences in `dtype` with `round`-ed operands (bf16 by default, identity: the exact-fp32 sweeps), in the kernels'
    layout: dict(out, outd, res [T,B,4H], dG [T,B,4H], dh_init), lists per layer.  Like the kernels, the backward pass reads what
    the forward pass stored.  `mutate`: one of MUTATIONS, or of MUTATIONS_FP32 with round = identity."""
    assert mutate is None or mutate in (MUTATIONS_FP32 if round is identity else MUTATIONS), mutate
    I = inputs
    rnd = bf16_trunc if mutate == "truncate" else drop_low_bits(PRECISION_MUTATIONS[mutate]) if mutate in PRECISION_MUTATIONS else round
    q = lambda x: rnd(x).astype(dtype)
    c = lambda x: np.asarray(x, dtype=dtype)
    L = len(I["whh"])
    T, B, _ = I["gi0"].shape
    H = I["whh"][0].shape[1]
    masks = [c(m) for m in I["masks"]] if I["masks"] else None
    one = np.dtype(dtype).type(1)
    sig = lambda v: one / (one + np.exp(-v))
    out, outd, res = [], [], []
    x = None
    for l in range(L):
        wq, bh = q(I["whh"][l]), c(I["bhh"][l])
        gi = c(I["gi0"]) if l == 0 else (q(x.reshape(T * B, H)) @ q(I["wih"][l]).T + c(I["bih"][l])).reshape(T, B, 3 * H)
        h = c(I["h0"][l])
        o = np.empty((T, B, H), dtype=dtype); rs = np.empty((T, B, 4 * H), dtype=dtype)
        for t in range(T):
            gh = q(h) @ wq.T + bh
            r = sig(gi[t][:, :H] + gh[:, :H]); z = sig(gi[t][:, H:2 * H] + gh[:, H:2 * H])
            ghn = gh[:, 2 * H:]
            n = np.tanh(gi[t][:, 2 * H:] + r * ghn)
            h = (z * n + (one - z) * h) if mutate == "swap_z" else ((one - z) * n + z * h)
            o[t] = h
            rs[t] = np.concatenate([r, z, n, ghn - bh[2 * H:] if mutate == "ghn_saved_without_bias" else ghn], axis=1)
        out.append(o); res.append(rs)
        x = o * masks[l] if (masks and l < L - 1) else o
        outd.append(x)
    dG, dh_init = [None] * L, [None] * L
    dy = c(I["dY"])
    for l in range(L - 1, -1, -1):
        wq, bh = q(I["whh"][l]), c(I["bhh"][l])
        carry = c(I["dhl"][l]) if I["dhl"] is not None else np.zeros((B, H), dtype=dtype)
        g = np.empty((T, B, 4 * H), dtype=dtype)
        h0 = c(I["h0"][l])
        for t in range(T - 1, -1, -1):
            rs = res[l][t]
            r, z, n, ghn = rs[:, :H], rs[:, H:2 * H], rs[:, 2 * H:3 * H], rs[:, 3 * H:]
            hp = out[l][t - 1] if t > 0 else h0
            d = dy[t] + carry
            dn = d * (one - z)
            dz = d * (((out[l][t - 2] if t > 1 else h0) if mutate == "dz_stale_h" else hp) - n)
            dn_pre = dn * (one - n * n)
            dz_pre = np.zeros_like(dz) if mutate == "dz_zero" else dz * z * (one - z)
            dr_pre = dn_pre * (ghn - bh[2 * H:] if mutate == "dr_without_bias" else ghn) * r * (one - r)
            g[t] = np.concatenate([dr_pre, dz_pre, dn_pre * r, dn_pre], axis=1)
            carry = d * z + (g[t][:, :3 * H] if mutate == "carry_unrounded" else q(g[t][:, :3 * H])) @ wq
        dG[l], dh_init[l] = g, carry
        if l > 0:
            dgi = np.concatenate([g[:, :, :2 * H], g[:, :, 3 * H:]], axis=2).reshape(T * B, 3 * H)
            dy = (q(dgi) @ q(I["wih"][l])).reshape(T, B, H)
            if masks:
                assert mutate != "wrong_mask" or L >= 3
                dy = dy * masks[l % (L - 1) if mutate == "wrong_mask" else l - 1]
    return dict(out=out, outd=outd, res=res, dG=dG, dh_init=dh_init)


def max_errors(kernel, forced):
    """max |kernel - forced| per tensor kind and layer."""
    return {k: [float(np.abs(np.asarray(kernel[k][l], dtype=np.float64) - forced[k][l]).max()) for l in range(len(forced[k]))] for k in KINDS}


def floor_e32(inputs, round=bf16_rne):
    """e32: the float32 stand-in against the oracle driven by the stand-in's own tensors, per kind and layer."""
    s = standin(inputs, round=round)
    return max_errors(s, operand_forced(inputs, s, round=round))


def caps(forced):
    """What M * e32 may not exceed, per kind and layer: CAP_ABS on out / reserve, CAP_RMS x rms(oracle tensor) on the gradients."""
    rms = lambda a: float(np.sqrt(np.mean(np.square(a))))
    L = len(forced["out"])
    return {"out": [CAP_ABS] * L, "res": [CAP_ABS] * L,
            "dG": [CAP_RMS * rms(forced["dG"][l]) for l in range(L)], "dh_init": [CAP_RMS * rms(forced["dh_init"][l]) for l in range(L)]}


def check_kernel(inputs, kernel, label, round=bf16_rne, e32=None):
    """The operand-forced comparison of a kernel's tensors: prints err, e32 and err / e32 per kind and layer, then asserts the caps
    on M * e32 and err <= M * e32.  Returns the table's rows.  `round`: the kernel's operand rounding (identity: the exact-fp32
    sweeps; the same M); `e32`: floor_e32(inputs, round) where the caller already has it (several kernels on one set of inputs)."""
    forced = operand_forced(inputs, kernel, round=round)
    err, e32, cap = max_errors(kernel, forced), floor_e32(inputs, round=round) if e32 is None else e32, caps(forced)
    rows = [(k, l, err[k][l], e32[k][l], cap[k][l]) for k in KINDS for l in range(len(forced[k]))]
    tag = "fp32 oracle" if round is identity else "bf16 oracle"
    for k, l, e, f, c_ in rows:
        print(f"[{tag}] {label} {k}[{l}]: err {e:.3e}  e32 {f:.3e}  ratio {e / f if f > 0 else float('inf'):.2f}  bound {M[k] * f:.3e}  cap {c_:.3e}")
    for k, l, e, f, c_ in rows:
        assert f > 0, f"{label} {k}[{l}]: the stand-in's floor is zero"
        assert M[k] * f <= c_, f"{label} {k}[{l}]: bound {M[k] * f:.3e} above its cap {c_:.3e}"
    for k, l, e, f, c_ in rows:
        assert e <= M[k] * f, f"{label} {k}[{l}]: {e:.3e} from the operand-forced oracle, bound {M[k]:g} x {f:.3e}"
    return rows
