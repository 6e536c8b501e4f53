"""b2t_clm_score_f16 (csrc/causal_lm.hip) against an fp64 restatement of its numerics contract, on both GEMM tile paths.

The reference (_ref_logp) is an n-layer pre-LN OPT in float64 on the GPU that rounds to fp16 exactly where the file header's
contract does and nowhere else: the LayerNorm outputs, q after its bias and the head_dim^-0.5 scaling (rounded once), k and v,
the attention output, fc1 after its ReLU.  The embedding sum, residual stream, LayerNorm statistics, softmax, log-softmax and
the sums stay fp64.  The attention's probabilities P are rounded to fp16 as the kernel's online softmax rounds them, per 32-key
block relative to the running maximum (the kernel's P.V operand); left unrounded, that one rounding moved the attention output
by an ulp in about half of its elements and the log-probs by up to 4.8e-3.

B2T_CLM_GEMM_256 selects the GEMM tiles (0 = 128 x 128 always, unset = the default rule, 2 = 256 x 256 always); the two
kernels must agree bit for bit.  Every call here gets a fresh workspace filled with 0xFF (NaN in fp16 and fp32), so a tile,
column group or row the kernels never write shows up as NaN instead of as the previous call's identical value."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import llm_rescore as R
from test_gpu_llm_rescore import _random_opt

pytestmark = pytest.mark.gpu

V_OPT = 50272
WIDTHS = {"1.3b": (2048, 32, 8192), "2.7b": (2560, 32, 10240), "6.7b": (4096, 32, 16384)}
ENV = "B2T_CLM_GEMM_256"


def _tile(M, N, mode=None):
    """The tile edge launch_gemm picks for an M x N GEMM (its rule mirrored; test_clm_host.py pins the C++ side)."""
    if mode == "2":
        return 256
    if mode == "0":
        return 128
    return 256 if (-(-M // 256)) * (-(-N // 256)) >= 256 else 128


@contextlib.contextmanager
def _tiles(mode):
    old = os.environ.get(ENV)
    if mode is None:
        os.environ.pop(ENV, None)
    else:
        os.environ[ENV] = mode
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old


_MODELS = {}


def _model(d, heads, ffn, vocab, max_pos=2048, n_layers=2, seed=0):
    """(OptScorer, state dict, dims), cached: the OPT-width models take seconds to build."""
    key = (d, heads, ffn, vocab, max_pos, n_layers, seed)
    if key not in _MODELS:
        if len(_MODELS) >= 3:
            _MODELS.pop(next(iter(_MODELS)))
        st, dims = _random_opt(d, heads, ffn, vocab, max_pos, seed=seed + d + vocab, n_layers=n_layers)
        _MODELS[key] = (R.OptScorer(dims, R.device_layout(st, dims), "cuda"), st, dims)
    return _MODELS[key]


def _logp(sc, seqs, mode=None):
    """Per-sequence token log-probs of the kernel, on a fresh poisoned workspace, under B2T_CLM_GEMM_256 = mode."""
    import torch
    import b2t_native as N
    M = sum(len(s) for s in seqs)
    need = N.load().b2t_clm_ws_bytes(C.byref(sc.desc), M, len(seqs))
    sc._ws = None
    torch.cuda.empty_cache()
    sc._ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    with _tiles(mode):
        out = sc.token_logprobs(seqs)
    sc._ws = None
    return out


def _ref_logp(st, dims, seqs):
    """fp64 forward rounded to fp16 where the contract rounds; per sequence the log-probs (0 at the first token)."""
    import torch
    F = torch.nn.functional
    W = lambda k: st[k].double()
    r16 = lambda t: t.half().double()
    d, H, nl, V = dims["d_model"], dims["n_heads"], dims["n_layers"], dims["vocab"]
    hd = d // H
    lens = [len(s) for s in seqs]
    B = len(seqs)
    dev = st["decoder.embed_tokens.weight"].device
    ids = torch.as_tensor(np.concatenate([np.asarray(s, np.int64) for s in seqs]), device=dev)
    pos = torch.as_tensor(np.concatenate([np.arange(n) for n in lens]), device=dev)
    off = np.concatenate([[0], np.cumsum(lens)])
    # padded attention batches of whole sequences, each batch's score tensor <= 2^27 fp64 elements (1 GB)
    groups, cur = [], []
    for i in range(B):
        if cur and (len(cur) + 1) * H * max(lens[j] for j in cur + [i]) ** 2 > 1 << 27:
            groups.append(cur); cur = []
        cur.append(i)
    groups.append(cur)
    x = W("decoder.embed_tokens.weight")[ids] + W("decoder.embed_positions.weight")[pos + 2]
    ln = lambda t, p: F.layer_norm(t, (d,), W(p + ".weight"), W(p + ".bias"), 1e-5)
    lin = lambda t, p: t @ W(p + ".weight").T + W(p + ".bias")
    for l in range(nl):
        p = f"decoder.layers.{l}."
        h = r16(ln(x, p + "self_attn_layer_norm"))
        q = r16(lin(h, p + "self_attn.q_proj") * hd ** -0.5)
        k = r16(lin(h, p + "self_attn.k_proj"))
        v = r16(lin(h, p + "self_attn.v_proj"))
        o = torch.empty_like(q)
        for g in groups:
            Lg = max(lens[j] for j in g)
            idx = torch.as_tensor(np.stack([off[j] + np.minimum(np.arange(Lg), lens[j] - 1) for j in g]), device=dev)
            L = torch.as_tensor([lens[j] for j in g], device=dev)
            sh = lambda t: t[idx].view(len(g), Lg, H, hd).transpose(1, 2)          # [b, H, Lg, hd]
            s = sh(q) @ sh(k).transpose(2, 3)
            kk = torch.arange(Lg, device=dev)
            mask = (kk[None, :] > kk[:, None])[None] | (kk[None, None, :] >= L[:, None, None])   # [b, Lg(query), Lg(key)]
            s = s.masked_fill(mask[:, None], float("-inf"))
            # the kernel's online softmax over 32-key blocks: P of block b is exp(s - m_b) rounded to fp16, m_b the running
            # max through block b, then rescaled by exp(m_b - m_final); the normaliser sums the unrounded P
            nb = -(-Lg // 32)
            sb = F.pad(s, (0, nb * 32 - Lg), value=float("-inf")).view(len(g), H, Lg, nb, 32)
            mb = sb.amax(-1).cummax(-1).values                      # finite: key 0 is valid for every query row
            pb = torch.exp(sb - mb[..., None])
            resc = torch.exp(mb - mb[..., -1:])[..., None]
            l = (pb * resc).sum((-1, -2))
            p16 = (r16(pb) * resc).view(len(g), H, Lg, nb * 32)[..., :Lg]
            og = ((p16 @ sh(v)) / l[..., None]).transpose(1, 2).reshape(len(g), Lg, d)
            for a, j in enumerate(g):
                o[off[j]:off[j + 1]] = og[a, :lens[j]]
        x = x + lin(r16(o), p + "self_attn.out_proj")
        h = r16(ln(x, p + "final_layer_norm"))
        x = x + lin(r16(torch.relu(lin(h, p + "fc1"))), p + "fc2")
    src = torch.as_tensor(np.concatenate([np.arange(off[j], off[j + 1] - 1) for j in range(B)]).astype(np.int64), device=dev)
    out = [np.zeros(n) for n in lens]
    if src.numel() == 0:
        return out
    tgt = ids[src + 1]
    h = r16(F.layer_norm(x[src], (d,), W("decoder.final_layer_norm.weight"), W("decoder.final_layer_norm.bias"), 1e-5))
    E = st["decoder.embed_tokens.weight"]
    chunk = max(64, (1 << 27) // h.shape[0])   # fp64 logits of one vocabulary chunk <= 1 GB
    lse = torch.stack([torch.logsumexp(h @ E[c:c + chunk].double().T, -1) for c in range(0, V, chunk)], -1).logsumexp(-1)
    lp = ((h * E[tgt].double()).sum(-1) - lse).cpu().numpy()
    r = 0
    for j in range(B):
        out[j][1:] = lp[r:r + lens[j] - 1]
        r += lens[j] - 1
    return out


def _err(got, ref):
    g, r = np.concatenate(got), np.concatenate(ref)
    assert g.shape == r.shape and np.isfinite(g).all(), "non-finite log-probs"
    return float(np.abs(g - r).max()), float(np.abs(r).max())


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a) == len(b)


def _prod_list(V, seed=0, cands=100):
    """tools/bench_llm_rescore.py's list generator: cands candidates of 10-40 tokens, BOS first."""
    rng = np.random.default_rng(seed)
    return [[2] + list(rng.integers(4, V, int(n) - 1)) for n in rng.integers(10, 41, cands)]


def _random_seqs(lens, V, seed):
    rng = np.random.default_rng(seed)
    return [[2] + list(rng.integers(0, V, n - 1)) for n in lens]


# Bound on max |dlogp| against the fp64 reference: measured on an MI355X at 1.2e-3 .. 3.8e-3 over every shape below (median
# |dlogp| about 6e-4), 2.6x headroom.  With the contract's roundings and P's emulated, what remains is rounding flips: the
# kernel's fp32 and the reference's fp64 land on different sides of an fp16 rounding boundary (1.3 % of the attention
# outputs), and one ulp there moves the 2-layer log-probs by up to a few 1e-3.  Every log-prob here is checked, targets
# down to -20.  The planted bugs this file was checked against moved them by 0.13 (q scaling one column too far) and 2.05
# (q scaled before its bias), or gave NaN from the poisoned workspace.
BOUND = 1e-2

TOTALS = {1: [1], 255: [120, 90, 45], 256: [128, 100, 28], 257: [1, 200, 56], 2500: None}
SHAPES = {"d576": (576, 9, 1344, 65), "d320": (320, 4, 1216, 1000), "d384": (384, 3, 1600, 40),
          "1.3b": WIDTHS["1.3b"] + (V_OPT,), "2.7b": WIDTHS["2.7b"] + (V_OPT,), "6.7b": WIDTHS["6.7b"] + (V_OPT,)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_tile_paths_bit_identical_and_within_fp64_bound(shape):
    """128- and 256-tiles give the same bits at token totals 1, 255, 256, 257 and ~2500; both within the fp64 bound.
    d 576 = 9 x 64 puts q's last columns and k's first in one 128 / 256 column tile (qcols = 576); 3d = 1728, 1344, 960 and
    4800 are padded weights of ragged N; vocab 65, 40 leave a 1- and a 40-column last group (40: the only one).
    Measured max |dlogp| (255 / 256 / 257 / ~2530 tokens): d576 3.2e-3 2.6e-3 2.6e-3 3.7e-3; d320 3.0e-3 2.9e-3 2.1e-3
    3.3e-3; d384 3.0e-3 2.8e-3 2.6e-3 3.1e-3; 1.3b 3.8e-3 2.4e-3 2.8e-3 3.3e-3; 2.7b 2.9e-3 2.6e-3 3.5e-3 3.0e-3;
    6.7b 2.8e-3 2.8e-3 2.6e-3 3.8e-3."""
    d, H, F, V = SHAPES[shape]
    sc, st, dims = _model(d, H, F, V)
    for total, lens in TOTALS.items():
        seqs = _prod_list(V, seed=total) if lens is None else _random_seqs(lens, V, seed=total)
        assert lens is not None or 2300 <= sum(map(len, seqs)) <= 2700
        a = _logp(sc, seqs, "0")
        b = _logp(sc, seqs, "2")
        assert _same(a, b), (shape, total)
        err, mx = _err(a, _ref_logp(st, dims, seqs))
        print(f"CLM tiles {shape} tokens {sum(map(len, seqs))}: max |dlogp| {err:.3e} (max |logp| {mx:.2f})")
        assert err <= BOUND, (shape, total, err)


@pytest.mark.parametrize("width", ["6.7b", "2.7b", "1.3b"])
def test_production_list_default_rule(width):
    """The bench's list (100 candidates of 10-40 tokens, ~2500 tokens) on the default rule against the fp64 reference; the
    rule must have put the GEMMs on the tiles listed (256 for QKV, fc1 and the head where they fill the chip).
    Measured max |dlogp| at 2531 tokens: 6.7b 3.7e-3, 2.7b 3.2e-3, 1.3b 3.6e-3."""
    d, H, F = WIDTHS[width]
    sc, st, dims = _model(d, H, F, V_OPT)
    seqs = _prod_list(V_OPT)
    M = sum(map(len, seqs))
    Mh = M - len(seqs)
    tiles = {"qkv": _tile(M, 3 * d), "out": _tile(M, d), "fc1": _tile(M, F), "fc2": _tile(M, d), "head": _tile(Mh, V_OPT)}
    want = {"6.7b": dict(qkv=256, out=128, fc1=256, fc2=128, head=256),
            "2.7b": dict(qkv=256, out=128, fc1=256, fc2=128, head=256),
            "1.3b": dict(qkv=128, out=128, fc1=256, fc2=128, head=256)}[width]
    assert tiles == want, (M, tiles)
    got = _logp(sc, seqs)
    err, mx = _err(got, _ref_logp(st, dims, seqs))
    print(f"CLM production {width} tokens {M}: max |dlogp| {err:.3e} (max |logp| {mx:.2f})")
    assert err <= BOUND
    assert _same(got, _logp(sc, seqs, "0"))


def test_head_edges():
    """Targets at the edges of the 64-column groups and of the vocabulary (V = 50272: the last group has 32 columns), and
    small vocabularies where the last group carries a large share of the mass (40: one partial group; 64: one full group;
    65 and 257: a 1-column last group).  Both tile paths, bit-identical.  Measured max |dlogp|: vocab 50272 1.2e-3,
    40 2.1e-3, 64 2.5e-3, 65 2.5e-3, 257 3.0e-3."""
    edge = [0, 63, 64, 127, 128, 255, 256, V_OPT - 65, V_OPT - 64, V_OPT - 33, V_OPT - 32, V_OPT - 1]
    sc, st, dims = _model(256, 4, 512, V_OPT)
    seqs = [[2] + edge, [2] + edge[::-1], [V_OPT - 1] + edge[1::2] + edge[0::2]]
    cases = [(sc, st, dims, seqs)]
    for V in (40, 64, 65, 257):
        s2, t2, d2 = _model(256, 4, 512, V)
        every = list(range(V))
        rng = np.random.default_rng(V)
        cases.append((s2, t2, d2, [[2] + every, [V - 1] + every[::-1], [2] + list(rng.integers(V - 2, V, 40))]))
    for sc, st, dims, seqs in cases:
        a, b = _logp(sc, seqs, "0"), _logp(sc, seqs, "2")
        assert _same(a, b), dims["vocab"]
        err, mx = _err(a, _ref_logp(st, dims, seqs))
        print(f"CLM head edges vocab {dims['vocab']}: max |dlogp| {err:.3e} (max |logp| {mx:.2f})")
        assert err <= BOUND, (dims["vocab"], err)


@pytest.mark.parametrize("hd", [64, 80, 128])
def test_attention_edges(hd):
    """Lengths 1, 31-33, 63-65, 127-129 (32-row block edges) and one of exactly max_pos (the position table's last row) in
    one pack, last; at head dim 128 also one 2048-token sequence.  Measured max |dlogp|: head dim 64
    3.0e-3, 80 3.0e-3, 128 2.7e-3; 2048 tokens 2.8e-3."""
    d = {64: 128, 80: 320, 128: 256}[hd]
    max_pos = 150
    sc, st, dims = _model(d, d // hd, 2 * d, 1000, max_pos=max_pos)
    seqs = _random_seqs([1, 31, 32, 33, 63, 64, 65, 127, 128, 129, max_pos], 1000, seed=hd)
    cases = [(sc, st, dims, seqs)]
    if hd == 128:
        s2, t2, d2 = _model(d, d // hd, 2 * d, 1000, max_pos=2048)
        cases.append((s2, t2, d2, _random_seqs([2048], 1000, seed=7)))
    for sc, st, dims, seqs in cases:
        got = _logp(sc, seqs)
        err, mx = _err(got, _ref_logp(st, dims, seqs))
        print(f"CLM attention hd {hd} max_pos {dims['max_pos']} longest {max(map(len, seqs))}: max |dlogp| {err:.3e} "
              f"(max |logp| {mx:.2f})")
        assert err <= BOUND, (hd, err)


def test_invariance_across_the_tile_switch():
    """At OPT-6.7b width a probe alone (every GEMM on 128-tiles) is bit-identical to the same probe at positions 0, middle
    and last of a production list (QKV, fc1 and the head on 256-tiles) and to the probe alone with 256-tiles forced."""
    d, H, F = WIDTHS["6.7b"]
    sc, _, _ = _model(d, H, F, V_OPT)
    probe = _random_seqs([37], V_OPT, seed=11)[0]
    others = _prod_list(V_OPT, seed=5)
    alone = _logp(sc, [probe])[0]
    assert _tile(len(probe), 3 * d) == 128 and np.isfinite(alone).all()
    assert _logp(sc, [probe], "2")[0].tobytes() == alone.tobytes()
    for pos in (0, 50, 100):
        batch = others[:pos] + [probe] + others[pos:]
        M = sum(map(len, batch))
        assert _tile(M, 3 * d) == 256 and _tile(M, F) == 256 and _tile(M - len(batch), V_OPT) == 256
        assert _logp(sc, batch)[pos].tobytes() == alone.tobytes(), pos


@pytest.mark.parametrize("mode", ["0", "2"])
def test_poisoned_workspace(mode):
    """The ABI driven directly: a workspace of exactly b2t_clm_ws_bytes bytes filled with 0xFF gives the same bits as a
    zeroed one, with no NaN; the canaries behind the workspace, scores_out and tok_logp_out are untouched; the scores without
    tok_logp_out equal those with it."""
    import torch
    import b2t_native as N
    lib = N.load()
    sc, _, _ = _model(576, 9, 1344, 65)
    seqs = _random_seqs([33, 1, 70, 5, 129, 41], 65, seed=3)   # 279 tokens; the last sequence ends inside a 32-key block
    ids = np.ascontiguousarray(np.concatenate(seqs), np.int32)
    off = np.zeros(len(seqs) + 1, np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    M, S, CAN = int(off[-1]), len(seqs), 4096
    need = lib.b2t_clm_ws_bytes(C.byref(sc.desc), M, S)
    assert need > 0
    canary = torch.randint(0, 256, (CAN,), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(fill, with_tok):
        ws = torch.empty(need + CAN, dtype=torch.uint8, device="cuda")
        ws[:need] = fill
        ws[need:] = canary
        scores = torch.full((S + 64,), 12345.0, device="cuda")
        tok = torch.full((M + 64,), 12345.0, device="cuda")
        with _tiles(mode):
            rc = lib.b2t_clm_score_f16(C.byref(sc.desc), ids.ctypes.data, off.ctypes.data, S, scores.data_ptr(),
                                       tok.data_ptr() if with_tok else None, ws.data_ptr(), need, stream)
        assert rc == 0, N.last_error()
        torch.cuda.synchronize()
        assert torch.equal(ws[need:], canary)
        assert (scores[S:] == 12345.0).all() and (tok[M:] == 12345.0).all()
        if not with_tok:
            assert (tok == 12345.0).all()
        return scores[:S].cpu().numpy(), tok[:M].cpu().numpy()

    s_p, t_p = run(0xFF, True)
    s_z, t_z = run(0, True)
    s_n, _ = run(0xFF, False)
    assert np.isfinite(s_p).all() and np.isfinite(t_p).all()
    assert s_p.tobytes() == s_z.tobytes() and t_p.tobytes() == t_z.tobytes()
    assert s_n.tobytes() == s_p.tobytes()
    assert (t_p[off[:-1]] == 0).all()
