"""The instrumented return of the oracle's three prefix beam searches (oracle/b2t_oracle.py: margin, e_ref, same_kept, beam),
which tests/test_gpu_beam_edges.py uses to decide where a strict comparison with the kernel is fair.  CPU only."""
import math

import numpy as np

from oracle import b2t_oracle as O

KNOWN = np.array([[0.25, 0.40, 0.35], [0.40, 0.35, 0.25], [0.10, 0.50, 0.40]], dtype=np.float32)


def test_known_answer_under_both_roundings():
    """ctc_prefix_beam_search_test.cc:18-59 comes out of the fp32-rounded search and of the one with log-adds in double."""
    res, info = O.prefix_beam_search(np.log(KNOWN), 3, 3, instrument=True)
    assert res == O.prefix_beam_search(np.log(KNOWN), 3, 3)          # the default return is the fp32-rounded list
    assert info["same_kept"]
    assert [r[0] for r in res] == [(2, 1), (1, 2), (1,)]
    np.testing.assert_allclose([math.exp(r[1]) for r in res], [0.2185, 0.1550, 0.1525], rtol=1e-5)
    np.testing.assert_allclose([math.exp(r[2]) for r in res], [0.07, 0.064, 0.07], rtol=1e-5)
    assert [r[3] for r in res] == [[0, 2], [0, 2], [2]]
    # the double run on its own: same list, and its scores differ from the rounded ones by e_ref at the most
    x, y = -1.25, -0.75
    assert O.log_add(x, y) == float(np.float32(O.log_add(x, y, rnd=False)))
    assert O.log_add(x, y, rnd=False) == math.log(math.exp(x - y) + 1.0) + y
    assert 0.0 < info["e_ref"] < 4 * 2.0 ** -24 * 3            # a few fp32 roundings of numbers in (-4, 0)
    assert info["beam"] == [r + (0.0,) for r in res]


def test_margin_by_hand():
    """Two frames, three classes, second beam 2.  Frame 0 keeps () 0.5 and (1) 0.4 and drops (2) 0.1: gap ln 4.  Frame 1
    (0.3, 0.3, 0.4): (1) = 0.4*0.3 + 0.4*0.3 + 0.5*0.3 = 0.39, (2) = 0.5*0.4 = 0.20 are kept, (1, 2) = 0.4*0.4 = 0.16 is
    the first dropped (then () = 0.15): gap ln(0.20 / 0.16) = ln 1.25, the minimum."""
    p = np.array([[0.5, 0.4, 0.1], [0.3, 0.3, 0.4]], dtype=np.float32)
    res, info = O.prefix_beam_search(np.log(p), 3, 2, instrument=True)
    assert [r[0] for r in res] == [(1,), (2,)]
    np.testing.assert_allclose([math.exp(r[1]) for r in res], [0.39, 0.20], rtol=1e-6)
    assert abs(info["frame_margin"][0] - math.log(4.0)) < 1e-6
    assert abs(info["frame_margin"][1] - math.log(1.25)) < 1e-6
    assert info["margin"] == info["frame_margin"][1]
    assert info["same_kept"] and info["e_ref"] < 1e-6
    # nothing dropped: +inf
    assert O.prefix_beam_search(np.log(p), 3, 16, instrument=True)[1]["margin"] == math.inf


def test_no_frames_is_the_initial_beam():
    empty = np.zeros((0, 3), dtype=np.float32)
    res, info = O.prefix_beam_search(empty, 3, 3, instrument=True)
    assert res == [((), 0.0, 0.0, [])] and info["margin"] == math.inf and info["e_ref"] == 0.0 and info["same_kept"]
    words = [None, "a", "b"]
    table = {("a",): (-0.3, 0.0), ("b",): (-0.4, 0.0), ("</s>",): (-1.0, 0.0), ("<s>",): (-99.0, -0.2)}
    assert O.prefix_beam_search_lm(empty, 1, table, words, 0.5, 0.1, 3, 3) == [((), 0.0, 0.0, 0.0)]
    lex = O.prefix_beam_search_lexicon(empty, {"a": [(2,)]}, 1, table, 0.5, 0.1, 3, 3, add_eos=False)
    assert lex == [((), (), 0.0, 0.0, 0.0)]


def test_fused_searches_instrumented_agree_with_default():
    """instrument=True changes nothing in the list; the fused searches now carry Viterbi data, which has no LM term: with
    alpha = beta = 0 and a beam nothing falls out of, it is the LM-free search's."""
    rng = np.random.default_rng(0)
    logp = O.log_softmax(rng.standard_normal((6, 4)).astype(np.float32) * 2)
    words = [None, "a", "b", "c"]
    table = {("a",): (-0.3, -0.1), ("b",): (-0.4, -0.2), ("c",): (-0.9, 0.0), ("a", "b"): (-0.2, 0.0), ("</s>",): (-1.0, 0.0),
             ("<s>",): (-99.0, -0.2)}
    a = O.prefix_beam_search_lm(logp, 2, table, words, 0.7, 0.3, 4, 5)
    b, info = O.prefix_beam_search_lm(logp, 2, table, words, 0.7, 0.3, 4, 5, instrument=True)
    assert a == b and len(info["beam"]) == len(b) and len(info["frame_margin"]) == 6
    assert sorted(r[0] for r in info["beam"]) == sorted(r[0] for r in b)
    free = {r[0]: r for r in O.prefix_beam_search(logp, 4, 4096)}
    _, i0 = O.prefix_beam_search_lm(logp, 2, table, words, 0.0, 0.0, 4, 4096, instrument=True)
    assert len(i0["beam"]) == len(free)
    for p, sc, v, tm, lm in i0["beam"]:
        assert (sc, v, tm) == free[p][1:] and lm == 0.0
