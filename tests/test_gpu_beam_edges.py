"""The three CTC prefix beam searchers (csrc/beam.hip: LM-free, token n-gram, lexicon + word n-gram) through the C ABI on
what tests/test_gpu_decoder.py never feeds them: per-utterance frame counts (lens), ragged streaming, blank != 0, the
class-count edges (C = 2, C = first_beam, 63, 64), every ranking path, frames with fewer finite classes than the first
beam, and both overflow causes (max_nodes, max_len) with recovery by b2t_beam_reset.

Every device buffer has a canary region behind it and is pre-filled with a poison pattern, so a write out of bounds, an
unwritten output and a write beyond hyp_len all show.

STRICT COMPARISON.  The oracle (oracle/b2t_oracle.py, instrument=True) reports for an input the smallest gap between the
last kept and the first dropped candidate of any frame (margin) and its own fp32-vs-double error (e_ref).  An input is
admissible if the fp32 and the double run keep the same prefixes in every frame and margin > 8 * e_ref (the kernel is
allowed 4 x the fp32 oracle's own error, and two such errors can meet at the boundary).  On an admissible input the
kernel's list must be the oracle's: same prefixes, same count, same lengths, the oracle's order wherever adjacent oracle
scores differ by more than 8 * e_ref, scores within 2e-4 * max(1, |ref|).  The seeds below were chosen on the CPU (the
most admissible of seeds 0-11 of each case: largest margin / e_ref; the rule is written out above SEEDS, the figures
measured for each seed at the end of the file); admissibility is asserted, never skipped.

EXACT VITERBI DATA.  On dyadic inputs (log-probs that are multiples of 1/8) Viterbi scores are exact in fp32 and in
double, exact ties are frequent, and vscore / times of EVERY hypothesis must equal the oracle's exactly, in all modes."""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import b2t_oracle as O

POISON, CANARY, GUARD = 0x5A, 0xA5, 4096
POISON_I32 = 0x5A5A5A5A
MODES = ("free", "lm", "lex")
MODE_C = {"free": 41, "lm": 41, "lex": 14}
FUSION = {"lm": (0.7, 0.3), "lex": (0.6, 0.5)}            # alpha, beta
WORDS41 = [None] + [f"p{i}" for i in range(1, 41)]
LENS = [48, 1, 17, 0, 33, 60]                              # the ragged batch (T = 48: the 60 is clamped)
RANK_PATHS = [(23, 16), (24, 16), (63, 16), (64, 7), (127, 16), (128, 16), (100, 1)]    # (second_beam, first_beam)
Out = namedtuple("Out", "hyps hl sc vs tm lms")


# ---- language models (the sizes tests/test_gpu_decoder.py uses) -------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _token_lm():
    import ngram_lm
    text = ngram_lm.synthetic_arpa(WORDS41, 3, 400, seed=3)
    return ngram_lm.NGramLM.from_arpa(text, WORDS41), O.parse_arpa(text)


@functools.lru_cache(maxsize=None)
def _lexicon_lm():
    import ngram_lm
    prons = ngram_lm.synthetic_lexicon(60, 14, seed=60)
    lex = ngram_lm.Lexicon(prons, 14)
    text = ngram_lm.synthetic_word_arpa(lex.words, 3, 180, seed=3)
    return prons, lex, ngram_lm.SparseNGramLM.from_arpa(text, lex.words), O.parse_arpa(text)


def oracle(mode, logp, first, second, blank=0):
    """The instrumented oracle of a mode (</s> is added in both fused modes, as the kernel is asked to)."""
    if mode == "free":
        return O.prefix_beam_search(logp, first, second, blank, instrument=True)[1]
    alpha, beta = FUSION[mode]
    if mode == "lm":
        _, (order, table) = _token_lm()
        return O.prefix_beam_search_lm(logp, order, table, WORDS41, alpha, beta, first, second, blank, add_eos=True,
                                       instrument=True)[1]
    prons, _, _, (order, table) = _lexicon_lm()
    return O.prefix_beam_search_lexicon(logp, prons, order, table, alpha, beta, first, second, blank, 1, add_eos=True,
                                        instrument=True)[1]


# ---- inputs -----------------------------------------------------------------------------------------------------------
def random_logp(mode, seed, T, C=None, scale=2.5, blank=0):
    """Tie-free rows: N(0, 1) logits x scale, +1 on blank (the lexicon mode: x 1.5 at the most, +0.7 on SIL, as in
    test_gpu_decoder.py)."""
    C = C or MODE_C[mode]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, C)).astype(np.float32) * (min(scale, 1.5) if mode == "lex" else scale)
    x[:, 1 if mode == "lex" else blank] += 0.7 if mode == "lex" else 1.0
    return O.log_softmax(x)


def dyadic_logp(mode, seed, T, blank=0):
    """-(integers 1..40) / 8, blank raised by 1.0, not normalised: Viterbi sums are exact, ties are frequent."""
    rng = np.random.default_rng(1000 + seed)
    x = -rng.integers(1, 41, size=(T, MODE_C[mode])).astype(np.float32) / 8
    x[:, blank] += 1.0
    return x


def masked_logp(mode, seed, T, blank=0, dyadic=True):
    """Dyadic (or random) rows; frames 2, 5, 8, ... keep 3 finite classes (alternately with and without blank), the rest
    is -inf."""
    x = dyadic_logp(mode, seed, T, blank) if dyadic else random_logp(mode, seed, T, blank=blank).copy()
    rng = np.random.default_rng(2000 + seed)
    others = [c for c in range(x.shape[1]) if c != blank]
    for t in range(2, T, 3):
        keep = [int(c) for c in rng.choice(others, 3, replace=False)]
        if (t // 3) % 2 == 0:
            keep[0] = blank
        drop = np.ones(x.shape[1], dtype=bool)
        drop[keep] = False
        x[t, drop] = -np.inf
    return x


def edge_logp(seed, T, C):
    """Random rows over C classes with the two highest class ids of a 64-lane wave (62, 63, where they exist; else C - 1)
    boosted on alternate odd frames, so they are in the best hypothesis."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, C)).astype(np.float32) * 2.5
    x[:, 0] += 1.0
    x[1::4, C - 1] += 8.0
    x[3::4, min(62, C - 1)] += 8.0
    return O.log_softmax(x)


def alternating_logp(seed, T, C=41, a=3, b=5):
    """Token a on even frames, b on odd ones, far above the rest: the best hypothesis has T tokens."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, C)).astype(np.float32)
    x[0::2, a] += 12.0
    x[1::2, b] += 12.0
    return O.log_softmax(x)


# ---- the cases whose seeds are committed --------------------------------------------------------------------------------
CASES = {}
for _m in MODES:
    for _second, _first in RANK_PATHS:
        CASES[f"rank-{_m}-{_second}-{_first}"] = dict(mode=_m, gen="random", T=24, first=_first, second=_second,
                                                      scale=1.5 if _second >= 63 else 2.5, n=2)
    for _j, _len in enumerate(LENS):
        if _len:
            CASES[f"ragged-{_m}-{_j}"] = dict(mode=_m, gen="random", T=48, use=min(_len, 48), first=10, second=10, n=1)
# Dyadic rows tie exactly, and in the LM-free search a tie across the pruning boundary of ANY frame makes margin = 0: of
# seeds 0-119 at T = 12, 24 and 48 with beams (10, 10) none is admissible.  So the LM-free dyadic cases are sized so that
# nothing is ever dropped (1 + 3 + 9 + 27 + 81 = 121 and 2^7 - 1 = 127 prefixes fit a beam of 128: margin = +inf); the
# fused modes, whose LM terms break the ties, run at beams (10, 10) (lexicon: 3 of seeds 0-11 admissible at T = 48,
# 35 of 0-119 at T = 24, from which the seeds are taken).
CASES["dyadic-free-3x4"] = dict(mode="free", gen="dyadic", T=4, first=3, second=128, n=3)
CASES["dyadic-free-2x6"] = dict(mode="free", gen="dyadic", T=6, first=2, second=128, n=3)
CASES["dyadic-lm"] = dict(mode="lm", gen="dyadic", T=48, first=10, second=10, n=3)
CASES["dyadic-lex"] = dict(mode="lex", gen="dyadic", T=24, first=10, second=10, n=3, pool=120)
# Masked frames, dyadic as well: LM 12 of 12 seeds admissible at T = 24; lexicon 3 of 0-119 and LM-free with blank 7 1 of
# 0-119 at T = 12 (none at 24 or 48); LM-free with blank 0: none of 0-119 at any of the three lengths, so that one runs on
# tie-free random rows with the same masks ("masked-random"), where Viterbi data is compared to the usual tolerance.
CASES["masked-lm"] = dict(mode="lm", gen="masked", T=24, first=10, second=10, n=2)
CASES["masked-lex"] = dict(mode="lex", gen="masked", T=12, first=10, second=10, n=2, pool=120)
CASES["masked-free-blank7"] = dict(mode="free", gen="masked", T=12, first=10, second=10, blank=7, n=1, pool=120)
CASES["masked-random-free"] = dict(mode="free", gen="masked-random", T=24, first=10, second=10, n=2)
CASES["masked-random-free-blank7"] = dict(mode="free", gen="masked-random", T=24, first=10, second=10, blank=7, n=2)
CASES["blank-40"] = dict(mode="free", gen="random", T=32, first=10, second=10, blank=40, n=2)
CASES["blank-7"] = dict(mode="free", gen="random", T=32, first=10, second=10, blank=7, n=2)
# C = 2 with a beam of 3: the live prefixes ((), (1), (1, 1) from frame 2 on) fill it exactly; a wider beam keeps prefixes of
# probability zero, which all tie at the log-zero sentinel (margin 0 for every seed)
for _C, _first, _second in ((2, 10, 3), (16, 16, 10), (63, 10, 10), (64, 10, 10)):
    CASES[f"classes-{_C}"] = dict(mode="free", gen="edge", T=24, C=_C, first=_first, second=_second, n=2)


def case_logp(name, seed):
    c = CASES[name]
    if c["gen"] == "random":
        return random_logp(c["mode"], seed, c["T"], scale=c.get("scale", 2.5), blank=c.get("blank", 0))
    if c["gen"] == "dyadic":
        return dyadic_logp(c["mode"], seed, c["T"], c.get("blank", 0))
    if c["gen"] in ("masked", "masked-random"):
        return masked_logp(c["mode"], seed, c["T"], c.get("blank", 0), dyadic=c["gen"] == "masked")
    return edge_logp(seed, c["T"], c["C"])


def case_oracle(name, seed):
    c = CASES[name]
    lp = case_logp(name, seed)
    return oracle(c["mode"], lp[:c.get("use", c["T"])], c["first"], c["second"], c.get("blank", 0))


def admissible(info):
    return info["same_kept"] and info["margin"] > 8 * info["e_ref"]


# Chosen on the CPU from seeds 0-11 of each case (0-119 where the case says pool=120): the admissible seeds ranked by
# margin / e_ref, largest first.  Two refinements, both from the precision of the formats rather than from any kernel
# result: a seed with e_ref == 0 has no ratio and is passed over (its kept scores are single paths, whose sums the oracle
# keeps in double), unless nothing is ever dropped (margin = +inf); and seeds whose final list has two adjacent scores
# between 8 * e_ref and 1e-4 apart come last -- e_ref measures the rounding of the log-adds only, while the kernel's plain
# sums are fp32 as well (half an ulp of a score near -40 is 1.9e-6, per frame), so such a pair can legitimately swap.
# dyadic-free-*: every seed is admissible alike (margin = +inf); 446, 487 and 379 are the first of seeds 0-3999 on which the
# times depend on the ORDER in which a prefix's repeat (case 1) and its parent's extension (cases 2 / 3) reach v_ns -- beam
# order in the oracle: the earlier one sets cur_token_prob, after which a better repeat raises v_ns but keeps the times.
SEEDS = {
    "rank-free-23-16": [6, 2],
    "rank-free-24-16": [9, 7],
    "rank-free-63-16": [2, 1],
    "rank-free-64-7": [7, 8],
    "rank-free-127-16": [3, 4],
    "rank-free-128-16": [4, 9],
    "rank-free-100-1": [0, 1],
    "ragged-free-0": [10],
    "ragged-free-1": [0],
    "ragged-free-2": [6],
    "ragged-free-4": [6],
    "ragged-free-5": [10],
    "rank-lm-23-16": [8, 6],
    "rank-lm-24-16": [8, 2],
    "rank-lm-63-16": [3, 1],
    "rank-lm-64-7": [5, 0],
    "rank-lm-127-16": [3, 4],
    "rank-lm-128-16": [3, 11],
    "rank-lm-100-1": [0, 1],
    "ragged-lm-0": [11],
    "ragged-lm-1": [0],
    "ragged-lm-2": [5],
    "ragged-lm-4": [7],
    "ragged-lm-5": [11],
    "rank-lex-23-16": [1, 8],
    "rank-lex-24-16": [4, 3],
    "rank-lex-63-16": [7, 0],
    "rank-lex-64-7": [8, 1],
    "rank-lex-127-16": [6, 5],
    "rank-lex-128-16": [6, 5],
    "rank-lex-100-1": [0, 1],
    "ragged-lex-0": [2],
    "ragged-lex-1": [0],
    "ragged-lex-2": [3],
    "ragged-lex-4": [2],
    "ragged-lex-5": [2],
    "dyadic-free-3x4": [0, 446, 487],
    "dyadic-free-2x6": [0, 1, 379],
    "dyadic-lm": [4, 1, 7],
    "dyadic-lex": [41, 94, 4],
    "masked-lm": [11, 2],
    "masked-lex": [31, 73],
    "masked-free-blank7": [77],
    "masked-random-free": [2, 11],
    "masked-random-free-blank7": [2, 6],
    "blank-40": [8, 7],
    "blank-7": [8, 10],
    "classes-2": [4, 1],
    "classes-16": [3, 8],
    "classes-63": [3, 2],
    "classes-64": [9, 6],
}


# ---- the kernel behind guarded, poisoned buffers -----------------------------------------------------------------------
class _Guarded:
    def __init__(self, nbytes, dev):
        self.n = int(nbytes)
        self.raw = torch.empty((self.n + GUARD,), dtype=torch.uint8, device=dev)
        self.raw[:self.n] = POISON
        self.raw[self.n:] = CANARY

    def view(self, dtype, shape):
        return self.raw[:self.n].view(dtype).view(shape)

    def intact(self):
        return bool((self.raw[self.n:] == CANARY).all().item())


class Beam:
    """One state block and one set of output buffers for U utterances of a mode; search() may be called chunk by chunk."""

    def __init__(self, mode, U, first, second, L, NN, blank=0, block_NN=None):
        import b2t_native as N
        self.N, self.lib = N, N.load()
        self.dev = torch.device("cuda:0")
        self.mode, self.U, self.first, self.second, self.L, self.NN, self.blank = mode, U, first, second, L, NN, blank
        self.g = {"state": _Guarded(self.lib.b2t_beam_state_bytes(L, block_NN or NN) * U, self.dev)}
        for k, n in (("hyps", U * second * L), ("hl", U * second), ("sc", U * second), ("vs", U * second),
                     ("tm", U * second * L), ("lms", U * second)):
            self.g[k] = _Guarded(4 * n, self.dev)
        self.hyps = self.g["hyps"].view(torch.int32, (U, second, L))
        self.tm = self.g["tm"].view(torch.int32, (U, second, L))
        self.hl = self.g["hl"].view(torch.int32, (U, second))
        self.sc, self.vs, self.lms = (self.g[k].view(torch.float32, (U, second)) for k in ("sc", "vs", "lms"))
        self.reset()

    def reset(self, NN=None):
        import b2t_ops as ops
        self.NN = NN or self.NN
        assert self.lib.b2t_beam_state_bytes(self.L, self.NN) * self.U <= self.g["state"].n
        self.N.check(self.lib.b2t_beam_reset(ops._p(self.g["state"].raw), self.U, self.L, self.NN, ops._stream()), "reset")

    def search(self, logp, lens=None):
        import b2t_ops as ops
        N, lib = self.N, self.lib
        lp = torch.from_numpy(np.ascontiguousarray(logp, dtype=np.float32)).to(self.dev)
        U, T, Cc = lp.shape
        assert U == self.U
        ln = None if lens is None else torch.tensor([int(v) for v in lens], dtype=torch.int32, device=self.dev)
        head = (ops._p(lp), None if ln is None else ops._p(ln), U, T, Cc, self.first, self.second, self.blank,
                ops._p(self.g["state"].raw), self.L, self.NN, ops._p(self.hyps), ops._p(self.hl), ops._p(self.sc),
                ops._p(self.vs), ops._p(self.tm))
        if self.mode == "free":
            N.check(lib.b2t_prefix_beam_search_f32(*head, ops._stream()), "search")
        elif self.mode == "lm":
            lm, _ = _token_lm()
            d = lm.to_device(self.dev)
            alpha, beta = FUSION["lm"]
            N.check(lib.b2t_prefix_beam_search_lm_f32(
                *head, ops._p(d["child"]), ops._p(d["logp"]), ops._p(d["bow"]), ops._p(d["suffix"]), ops._p(d["nstate"]),
                lm.V, lm.start_state, lm.eos, float(alpha), float(beta), float(lm.unk_logp), ops._p(self.lms),
                ops._stream()), "search_lm")
        else:
            _, lex, lm, _ = _lexicon_lm()
            dl, dm = lex.to_device(self.dev), lm.to_device(self.dev)
            alpha, beta = FUSION["lex"]
            d = N.LexLmDesc(dl["child"].data_ptr(), dl["wbeg"].data_ptr(), dl["wend"].data_ptr(), dl["wlist"].data_ptr(),
                            dm["cb"].data_ptr(), dm["ce"].data_ptr(), dm["ctok"].data_ptr(), dm["cnode"].data_ptr(),
                            dm["logp"].data_ptr(), dm["bow"].data_ptr(), dm["suffix"].data_ptr(), dm["nstate"].data_ptr(),
                            lm.start_state, lm.eos, 1, float(alpha), float(beta), float(lm.unk_logp))
            N.check(lib.b2t_prefix_beam_search_lex_f32(*head, C.byref(d), ops._p(self.lms), ops._stream()), "search_lex")
        torch.cuda.synchronize()
        return self

    def overflowed(self):
        import b2t_ops as ops
        flag = C.c_int(0)
        self.N.check(self.lib.b2t_beam_overflowed(ops._p(self.g["state"].raw), self.U, self.L, self.NN, C.byref(flag),
                                                  ops._stream()), "ovf")
        return flag.value

    def repoison(self):
        for k, g in self.g.items():
            if k != "state":
                g.raw[:g.n] = POISON

    def canaries(self):
        return [k for k, g in self.g.items() if not g.intact()]

    def read(self):
        assert self.canaries() == [], "bytes behind a buffer were written"
        lms = self.lms.cpu().numpy() if self.mode != "free" else np.zeros((self.U, self.second), dtype=np.float32)
        return Out(self.hyps.cpu().numpy(), self.hl.cpu().numpy(), self.sc.cpu().numpy(), self.vs.cpu().numpy(),
                   self.tm.cpu().numpy(), lms)


def run(mode, logp, first, second, lens=None, blank=0, chunks=None, L=None, NN=None, want_flag=0):
    """One search over logp [U][T][C] (optionally in chunks with per-chunk lens); the overflow flag must be want_flag."""
    U, T, _ = logp.shape
    b = Beam(mode, U, first, second, L or T + 1, NN or T * second + 2, blank)
    if chunks is None:
        b.search(logp, lens)
    else:
        for a, e in chunks:
            b.search(logp[:, a:e], None if lens is None else np.clip(np.asarray(lens) - a, 0, e - a))
    assert b.overflowed() == want_flag
    return b.read()


def prefixes(out, u):
    n = int((out.hl[u] >= 0).sum())
    return [tuple(int(v) for v in out.hyps[u, i, :out.hl[u, i]]) for i in range(n)]


def assert_same_bytes(a, b, ua=None, ub=None, what=""):
    """Every output of utterance ua of a equals that of ub of b, bit for bit (poison beyond hyp_len included)."""
    for name, x, y in zip(Out._fields, a, b):
        x = x if ua is None else x[ua]
        y = y if ub is None else y[ub]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {name} differs"


def check_vs_oracle(tag, mode, out, u, info, exact_viterbi=False):
    """The strict comparison (module docstring).  Returns the largest |kernel score - oracle score| of the list."""
    e, fm = info["e_ref"], info["frame_margin"]
    tf = int(np.argmin(fm)) if fm else -1
    ctx = f"{tag} u={u}: margin {info['margin']:.4g} (frame {tf}), margin in double {info['margin64']:.4g}, e_ref {e:.3g}"
    assert admissible(info), f"{ctx}: the committed input is not admissible (same kept sets: {info['same_kept']})"
    beam, keys = info["beam"], info["keys"]
    got = prefixes(out, u)
    n = len(got)
    ref = {r[0]: r for r in beam}
    k_sc = {p: (float(out.sc[u, i]), float(out.lms[u, i])) for i, p in enumerate(got)}
    extra = [(p, k_sc[p]) for p in got if p not in ref]
    lost = [(r[0], r[1], r[4]) for r in beam if r[0] not in k_sc]
    assert not extra and not lost and n == len(beam) == len(set(got)), \
        f"{ctx}: kernel-only (prefix, (score, lm)) {extra}; oracle-only (prefix, score, lm) {lost}; counts {n} / {len(beam)}"
    assert (out.hl[u, n:] == -1).all()
    start = 0
    for i in range(1, n + 1):            # the oracle's order, up to runs of scores closer than 8 * e_ref
        if i == n or keys[i - 1] - keys[i] > 8 * e:
            assert set(got[start:i]) == {r[0] for r in beam[start:i]}, \
                f"{ctx}: places {start}..{i - 1}: kernel {[(p, k_sc[p]) for p in got[start:i]]}, oracle {beam[start:i]} keys {keys[start:i]}"
            start = i
    worst = 0.0
    for i, p in enumerate(got):
        _, sc, vit, times, lm = ref[p]
        hl = int(out.hl[u, i])
        assert hl == len(p)
        d = abs(float(out.sc[u, i]) - sc)
        worst = max(worst, d)
        assert d < 2e-4 * max(1.0, abs(sc)), f"{ctx}: score of {p}: kernel {out.sc[u, i]!r}, oracle {sc!r}"
        if mode != "free":
            if math.isinf(lm):
                assert out.lms[u, i] == lm, f"{ctx}: lm score of {p}: kernel {out.lms[u, i]!r}, oracle {lm!r}"
            else:
                assert abs(float(out.lms[u, i]) - lm) < 2e-4 * max(1.0, abs(lm)), \
                    f"{ctx}: lm score of {p}: kernel {out.lms[u, i]!r}, oracle {lm!r}"
        if exact_viterbi:
            assert float(np.float32(vit)) == vit, "the oracle's Viterbi score is not exact in fp32: not a dyadic input"
            assert float(out.vs[u, i]) == vit, f"{ctx}: vscore of {p} (place {i}): kernel {out.vs[u, i]!r}, oracle {vit!r}"
            # (a prefix of probability zero that fills up a short list has no Viterbi path: the reference's times() is then
            # not a vector of hyp_len frames, and b2t.h leaves the row unspecified)
            assert vit <= -O.FLT_MAX or [int(v) for v in out.tm[u, i, :hl]] == times, \
                f"{ctx}: times of {p} (place {i}): kernel {out.tm[u, i, :hl].tolist()}, oracle {times}"
        else:
            assert abs(float(out.vs[u, i]) - vit) < 2e-4 * max(1.0, abs(vit)), f"{ctx}: vscore of {p}"
        assert (out.hyps[u, i, hl:] == POISON_I32).all() and (out.tm[u, i, hl:] == POISON_I32).all(), \
            f"{ctx}: place {i}: written beyond hyp_len"
    assert (out.hyps[u, n:] == POISON_I32).all() and (out.tm[u, n:] == POISON_I32).all(), f"{ctx}: rows beyond the list written"
    print(f"{ctx}, max |score - oracle| {worst:.3g}, list of {n}")
    return worst


def case_batch(name):
    return np.stack([case_logp(name, s) for s in SEEDS[name]])


def check_case(name, exact_viterbi=False):
    """Run a committed case as one batch and compare every utterance strictly with the oracle."""
    c = CASES[name]
    assert len(SEEDS[name]) == c["n"]
    logp = case_batch(name)
    out = run(c["mode"], logp, c["first"], c["second"], blank=c.get("blank", 0))
    for u, seed in enumerate(SEEDS[name]):
        check_vs_oracle(f"{name} seed {seed}", c["mode"], out, u, case_oracle(name, seed), exact_viterbi)
    return logp, out


# ---- ranking paths (256 / 512 / 1024 threads, 1 / 2 / 4 parts, odd candidate counts, rank_by_counting<9>) ------------
@pytest.mark.parametrize("second,first", RANK_PATHS)
@pytest.mark.parametrize("mode", MODES)
def test_ranking_paths_strict(mode, second, first):
    check_case(f"rank-{mode}-{second}-{first}")


# ---- exact Viterbi scores and times of every hypothesis ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["dyadic-free-3x4", "dyadic-free-2x6", "dyadic-lm", "dyadic-lex"])
def test_dyadic_viterbi_exact(name):
    check_case(name, exact_viterbi=True)


# ---- frames with fewer finite classes than first_beam ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["masked-free-blank7", "masked-lm", "masked-lex", "masked-random-free",
                                  "masked-random-free-blank7"])
def test_masked_frames(name):
    """The first beam takes K DISTINCT classes, the -inf ones in index order: no class twice, so blank's Viterbi data is
    not overwritten with -inf and no (parent, token) pair reaches the trie twice in a frame."""
    _, out = check_case(name, exact_viterbi=CASES[name]["gen"] == "masked")
    for u in range(len(SEEDS[name])):
        got = prefixes(out, u)
        assert len(set(got)) == len(got)          # a trie node is a prefix: none appears twice


# ---- per-utterance frame counts ----------------------------------------------------------------------------------------
def _ragged(mode):
    seeds = {j: SEEDS[f"ragged-{mode}-{j}"][0] for j, n in enumerate(LENS) if n}
    logp = np.stack([random_logp(mode, seeds.get(j, 99), 48) for j in range(len(LENS))])
    return seeds, logp


def _assert_initial_beam(out, u, mode):
    assert out.hl[u].tolist() == [0] + [-1] * (out.hl.shape[1] - 1)
    assert out.sc[u, 0] == 0.0 and out.vs[u, 0] == 0.0
    assert (out.hyps[u] == POISON_I32).all() and (out.tm[u] == POISON_I32).all()
    if mode != "free":                    # the empty sentence: alpha * ln p(</s> | <s>)
        assert abs(float(out.lms[u, 0]) - oracle(mode, np.zeros((0, MODE_C[mode]), np.float32), 10, 10)["beam"][0][4]) < 2e-4


@pytest.mark.parametrize("mode", MODES)
def test_ragged_lens(mode):
    seeds, logp = _ragged(mode)
    out = run(mode, logp, 10, 10, lens=LENS)
    for u, n in enumerate(LENS):
        if n == 0:
            _assert_initial_beam(out, u, mode)
            continue
        n = min(n, 48)
        solo = run(mode, logp[u:u + 1, :n], 10, 10, L=49, NN=48 * 10 + 2)         # no lens, T = the utterance's frames
        assert_same_bytes(out, solo, u, 0, f"utterance {u} ({n} frames) vs its own call")
        check_vs_oracle(f"ragged-{mode}-{u} seed {seeds[u]}", mode, out, u, case_oracle(f"ragged-{mode}-{u}", seeds[u]))


@pytest.mark.parametrize("mode", MODES)
def test_zero_frames_leave_the_state_usable(mode):
    """lens[u] == 0 consumes nothing: a later call decodes that utterance as if the empty call had not been, and leaves
    the utterances it gives no frames as they were."""
    seeds, logp = _ragged(mode)
    b = Beam(mode, len(LENS), 10, 10, 49, 482)
    first = b.search(logp, LENS).read()
    later = [0, 0, 0, 17, 0, 0]
    b.repoison()
    second = b.search(logp[::-1].copy(), later).read()                           # utterance 3 now gets utterance 2's rows
    assert b.overflowed() == 0
    for u in range(len(LENS)):
        if later[u] == 0:
            assert_same_bytes(first, second, u, u, f"utterance {u} got no frames")
    solo = run(mode, logp[2:3, :17], 10, 10, L=49, NN=482)
    assert_same_bytes(second, solo, 3, 0, "utterance 3 after an empty call")


@pytest.mark.parametrize("mode", MODES)
def test_ragged_streaming_equals_one_shot(mode):
    _, logp = _ragged(mode)
    whole = run(mode, logp, 10, 10, lens=LENS)
    b = Beam(mode, len(LENS), 10, 10, 49, 482)
    prev = None
    for a, e in [(0, 1), (1, 9), (9, 32), (32, 48)]:
        b.repoison()                  # every call writes the whole list anew; what an earlier, longer row left is not its business
        cur = b.search(logp[:, a:e], np.clip(np.asarray(LENS) - a, 0, e - a)).read()
        for u, n in enumerate(LENS):
            if prev is not None and n <= a:                                      # ended in an earlier chunk
                assert_same_bytes(prev, cur, u, u, f"utterance {u} ({n} frames) after chunk [{a}, {e})")
        prev = cur
    assert b.overflowed() == 0
    assert_same_bytes(whole, prev, what="chunked vs one call")


# ---- blank != 0 (LM-free) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blank", [40, 7])
def test_blank_elsewhere(blank):
    name = f"blank-{blank}"
    logp, out = check_case(name)
    # the same input with the blank column moved to 0 and the classes below it shifted up by one
    perm = [blank] + [c for c in range(41) if c != blank]                         # new column j holds old class perm[j]
    moved = run("free", np.ascontiguousarray(logp[:, :, perm]), 10, 10, blank=0)
    back = np.asarray(perm, dtype=np.int32)
    valid = np.arange(moved.hyps.shape[2])[None, None, :] < moved.hl[:, :, None]
    relabelled = np.where(valid, back[np.where(valid, moved.hyps, 0)], moved.hyps)
    assert_same_bytes(out, moved._replace(hyps=relabelled), what=f"blank {blank} vs blank moved to 0")


# ---- class-count edges (LM-free) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [2, 16, 63, 64])
def test_class_count_edges(Cc):
    """C = 2 (first_beam 10 is clamped to 2), C = first_beam = 16, C = 63 (one padding lane), C = 64 (none; bit 63 of the
    child mask).  The highest class ids are boosted into the best hypothesis."""
    name = f"classes-{Cc}"
    _, out = check_case(name)
    for u in range(len(SEEDS[name])):
        best = prefixes(out, u)[0]
        assert Cc - 1 in best and min(62, Cc - 1) in best


# ---- overflow: max_nodes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_overflow_max_nodes_and_recovery(mode):
    """A trie of 40 nodes cannot hold 48 frames of a beam of 10: the flag is raised, nothing is written out of bounds, an
    utterance of the batch that stays within 40 nodes is unaffected, and after b2t_beam_reset the same block (laid out
    anew for enough nodes) decodes like a block that never overflowed."""
    T, second = 48, 10
    logp = np.stack([random_logp(mode, 5, T), random_logp(mode, 6, T)])
    full = T * second + 2
    b = Beam(mode, 2, 10, second, T + 1, 40, block_NN=full)
    b.search(logp, [T, 3])                                   # utterance 1: 3 frames, <= 31 nodes
    assert b.overflowed() == 1
    over = b.read()                                          # (asserts the canaries)
    solo = run(mode, logp[1:2, :3], 10, second, L=T + 1, NN=40)
    assert_same_bytes(over, solo, 1, 0, "the utterance that did not overflow")
    tight = Beam(mode, 1, 10, second, T + 1, 40)             # the canary directly behind a 40-node block
    tight.search(logp[:1])
    assert tight.overflowed() == 1 and tight.canaries() == []
    b.reset(NN=full)
    assert b.overflowed() == 0
    b.repoison()
    again = b.search(logp).read()
    assert b.overflowed() == 0
    assert_same_bytes(again, run(mode, logp, 10, second), what="after reset vs a block that never overflowed")


# ---- overflow: max_len ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_overflow_max_len_sets_the_flag(mode):
    """Surviving prefixes longer than max_len = 8: flagged; hyps / times rows are clipped at 8 columns and nothing behind
    the buffers is touched."""
    logp = random_logp(mode, 7, 40)[None]
    b = Beam(mode, 1, 10, 10, 8, 40 * 10 + 2)
    b.search(logp)
    assert b.canaries() == []
    assert int(b.hl.max().item()) > 8, "the input does not exceed max_len: the case tests nothing"
    assert b.overflowed() == 1
    b.reset()
    assert b.overflowed() == 0


@pytest.mark.parametrize("mode", ["free", "lm"])
def test_max_len_exact_fit(mode):
    """12 alternating tokens in max_len = 8: flag.  9 tokens in 9 frames with max_len = 9 fit exactly: no flag, and the best
    hypothesis is all of them."""
    b = Beam(mode, 1, 10, 10, 8, 122)
    b.search(alternating_logp(1, 12)[None])
    assert b.overflowed() == 1 and b.canaries() == []
    assert int(b.hl[0, 0].item()) == 12                                          # the length is reported, the row is clipped
    out = run(mode, alternating_logp(1, 9)[None], 10, 10, L=9, NN=92, want_flag=0)
    assert prefixes(out, 0)[0] == (3, 5, 3, 5, 3, 5, 3, 5, 3)
    assert out.tm[0, 0].tolist() == list(range(9))


# ---- the product asks -----------------------------------------------------------------------------------------------------
def test_decoder_raises_on_overflow_and_recovers():
    import lm_decoder
    opts = lm_decoder.DecodeOptions(7000, 200, 17., 8., 0.325, 1.0, 0., 100)
    dec = lm_decoder.BrainSpeechDecoder(lm_decoder.DecodeResource("", "", "", "", ""), opts, max_len=8)
    with pytest.raises(RuntimeError, match="max_len"):
        lm_decoder.DecodeNumpyLogProbs(dec, alternating_logp(1, 12))
    assert dec.result() == []
    dec.Reset()
    short = alternating_logp(2, 6)
    lm_decoder.DecodeNumpyLogProbs(dec, short)
    ref = O.prefix_beam_search(short, 10, 10)
    best = dec.result()[0]
    assert tuple(int(t) for t in best.tokens) == tuple(ref[0][0]) == (3, 5, 3, 5, 3, 5)
    assert [int(t) for t in best.times] == ref[0][3]
    assert abs(best.ac_score - ref[0][1]) < 2e-4 * max(1.0, abs(ref[0][1]))


# Measured on an MI355X for the committed seeds -- case: seed (margin, e_ref, max |kernel score - oracle score|) ...
#   rank-free-23-16: 6 (0.005198, 9.98e-07, 2.62e-06); 2 (0.001094, 2.19e-07, 2.08e-06)
#   rank-free-24-16: 9 (0.001138, 2.15e-07, 4.54e-06); 7 (0.001858, 5.69e-07, 4.68e-06)
#   rank-free-63-16: 2 (0.0004368, 5.32e-07, 5.19e-06); 1 (8.07e-05, 1.96e-07, 4.56e-06)
#   rank-free-64-7: 7 (0.001019, 1.23e-06, 4.47e-06); 8 (0.0003233, 7.16e-07, 2.56e-06)
#   rank-free-127-16: 3 (0.000133, 1.35e-06, 3.1e-06); 4 (4.494e-05, 3.51e-06, 5.36e-06)
#   rank-free-128-16: 4 (0.0003271, 3.51e-06, 5.36e-06); 9 (0.000155, 1.37e-06, 4.05e-06)
#   rank-free-100-1: 0 (inf, 0, 2.68e-06); 1 (inf, 0, 2.12e-06)
#   ragged-free-0: 10 (0.002612, 2.66e-07, 4.74e-06)
#   ragged-free-1: 0 (inf, 0, 0)
#   ragged-free-2: 6 (0.01755, 2.5e-07, 1.91e-06)
#   ragged-free-4: 6 (0.005132, 2.5e-07, 1.74e-06)
#   ragged-free-5: 10 (0.002612, 2.66e-07, 4.74e-06)
#   rank-lm-23-16: 8 (0.004328, 1.39e-06, 4.53e-06); 6 (0.004993, 3.24e-06, 3.31e-06)
#   rank-lm-24-16: 8 (0.004955, 1.39e-06, 4.53e-06); 2 (0.005272, 2.27e-06, 3.81e-06)
#   rank-lm-63-16: 3 (0.004873, 6.03e-06, 1.53e-05); 1 (0.001228, 3.53e-06, 9.78e-06)
#   rank-lm-64-7: 5 (0.003216, 2.57e-06, 6.74e-06); 0 (0.0006294, 1.4e-06, 5.9e-06)
#   rank-lm-127-16: 3 (0.0006905, 4.91e-06, 1.53e-05); 4 (0.0009975, 7.73e-06, 1.2e-05)
#   rank-lm-128-16: 3 (0.0009918, 6.54e-06, 1.53e-05); 11 (0.0007935, 6.9e-06, 1.53e-05)
#   rank-lm-100-1: 0 (inf, 0, 2.68e-06); 1 (inf, 0, 2.12e-06)
#   ragged-lm-0: 11 (0.005627, 2.08e-06, 8.11e-06)
#   ragged-lm-1: 0 (inf, 0, 0)
#   ragged-lm-2: 5 (0.02561, 1.22e-06, 3.67e-06)
#   ragged-lm-4: 7 (0.00856, 8.72e-07, 4.41e-06)
#   ragged-lm-5: 11 (0.005627, 2.08e-06, 8.11e-06)
#   rank-lex-23-16: 1 (0.01281, 5.88e-06, 7.63e-06); 8 (0.005135, 2.73e-06, 5.72e-06)
#   rank-lex-24-16: 4 (0.009085, 5.81e-06, 8.7e-06); 3 (0.01396, 9.8e-06, 1.14e-05)
#   rank-lex-63-16: 7 (0.002403, 5.33e-06, 7.63e-06); 0 (0.001694, 6.26e-06, 7.63e-06)
#   rank-lex-64-7: 8 (0.00251, 3.25e-06, 5.72e-06); 1 (0.001259, 3.6e-06, 1e-05)
#   rank-lex-127-16: 6 (0.000927, 5.36e-06, 7.63e-06); 5 (0.0008297, 4.87e-06, 7.63e-06)
#   rank-lex-128-16: 6 (0.001152, 5.36e-06, 7.63e-06); 5 (0.0006981, 4.92e-06, 7.63e-06)
#   rank-lex-100-1: 0 (inf, 0, 0); 1 (inf, 0, 0)
#   ragged-lex-0: 2 (0.02055, 9.18e-06, 2.29e-05)
#   ragged-lex-1: 0 (inf, 0, 0)
#   ragged-lex-2: 3 (0.03472, 1.75e-06, 4.41e-06)
#   ragged-lex-4: 2 (0.02119, 4.09e-06, 4.41e-06)
#   ragged-lex-5: 2 (0.02055, 9.18e-06, 2.29e-05)
#   dyadic-free-3x4: 0 (inf, 0, 0); 446 (inf, 1.9e-09, 1.12e-08); 487 (inf, 4.37e-09, 5.96e-08)
#   dyadic-free-2x6: 0 (inf, 0, 0); 1 (inf, 0, 0); 379 (inf, 1.9e-09, 0)
#   dyadic-lm: 4 (0.00794, 4.75e-07, 9.54e-07); 1 (0.005705, 5.46e-07, 0); 7 (0.004295, 5.82e-07, 9.54e-07)
#   dyadic-lex: 41 (0.06916, 1.46e-06, 9.54e-07); 94 (0.04264, 1.52e-06, 0); 4 (0.03636, 1.39e-06, 9.54e-07)
#   masked-lm: 11 (0.02322, 5.36e-07, 1.19e-06); 2 (0.01417, 5.67e-07, 0)
#   masked-lex: 31 (0.03233, 3.91e-07, 4.77e-07); 73 (0.02149, 3.89e-07, 9.54e-07)
#   masked-free-blank7: 77 (0.02359, 2.02e-08, 1.04e-07)
#   masked-random-free: 2 (0.00413, 8.03e-08, 3.68e-06); 11 (0.001755, 2.13e-07, 5.76e-06)
#   masked-random-free-blank7: 2 (0.00413, 2.58e-08, 6.77e-06); 6 (0.001768, 1.71e-08, 3.81e-06)
#   blank-40: 8 (0.001503, 3.28e-09, 9.35e-07); 7 (0.01222, 1.74e-07, 3.32e-06)
#   blank-7: 8 (0.00961, 1.44e-07, 2.16e-06); 10 (0.003081, 1.38e-07, 1.94e-06)
#   classes-2: 4 (0.9101, 2.51e-07, 2.38e-07); 1 (0.5326, 1.97e-07, 1.19e-07)
#   classes-16: 3 (0.0761, 3.54e-07, 4.25e-07); 8 (0.01417, 2.21e-07, 8.24e-07)
#   classes-63: 3 (0.00747, 4.09e-07, 1.67e-06); 2 (0.002083, 1.64e-07, 2.62e-06)
#   classes-64: 9 (0.01834, 4.38e-08, 2.33e-06); 6 (0.02462, 8.69e-08, 7.87e-07)
