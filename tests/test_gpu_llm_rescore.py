"""b2t_clm_score_f16 (csrc/causal_lm.hip) on the MI355X: the tiny OPT of tests/golden/llm_rescore.npz against HF fp32, batch
invariance, one full-width layer + the 50272 head against a torch fp32 restatement, input errors, and the service end to end."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import llm_rescore as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
pytestmark = pytest.mark.gpu


def _tiny():
    import torch
    z = np.load(os.path.join(GOLD, "llm_rescore.npz"))
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        gold = json.load(f)
    cfg = gold["config"]
    state = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w/")}
    dims = R.opt_dims(cfg)
    return R.OptScorer(dims, R.device_layout(state, dims), "cuda"), z, gold


def _seqs(ids, off):
    return [ids[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_tiny_opt_matches_hf_fp32():
    sc, z, gold = _tiny()
    seqs = _seqs(z["ids"], z["seq_off"])
    tok = np.concatenate(sc.token_logprobs(seqs))
    # fp16 operands (the contract) against an fp32 forward: the error of a log-prob grows with its logit's magnitude (fp16's
    # relative precision 2^-11 on the head's operands), so the bound is 2e-3 plus 1e-3 of |logp| (measured on an MI355X:
    # max |dlogp| 7.9e-3 with log-probs down to -12, max |dscore| 2.4e-2 on scores down to -881)
    sco = sc.score(seqs, 0.0)
    err_tok = np.abs(tok - z["tok_logp"]).max()
    err_sc = np.abs(sco - z["scores"]).max()
    print(f"tiny OPT vs HF fp32: max |dlogp| {err_tok:.2e}, max |dscore| {err_sc:.2e}")
    assert np.all(np.abs(tok - z["tok_logp"]) <= 2e-3 + 1e-3 * np.abs(z["tok_logp"]))
    assert np.all(np.abs(sco - z["scores"]) <= 1e-2 + 1e-4 * np.abs(z["scores"]))
    # the reference's choice among the recorded n-best lists, with the HIP scorer in place of HF
    tk = R.WordTokenizer(**gold["tokenizer"])
    for c in gold["decode"]:
        r = R.gpt2_lm_decode(sc, tk, "cuda", c["nbest"], 0.35, length_penalty=c["length_penalty"], alpha=c["alpha"],
                             returnConfidence=c["confidence"], current_context_str=c["context"])
        assert r[0] == c["best"]


def test_batch_invariance():
    sc, z, _ = _tiny()
    rng = np.random.default_rng(3)
    probe = [2] + list(rng.integers(0, 272, 36))
    others = [[2] + list(rng.integers(0, 272, int(n))) for n in rng.integers(0, 100, 99)]
    alone = sc.score([probe])[0]
    for pos in (0, 37, 99):
        batch = others[:pos] + [probe] + others[pos:]
        s = sc.score(batch)
        assert s[pos].tobytes() == alone.tobytes(), pos
    a, b = sc.score(others), sc.score(others)
    assert a.tobytes() == b.tobytes()


def _random_opt(d, heads, ffn, vocab, max_pos, seed, n_layers=1):
    """A random pre-LN OPT state dict (fp16, on the GPU) and its dims.  The scales give log-prob spreads of about 2."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s, std: (torch.randn(*s, generator=g, device="cuda") * std).half()
    st = {"decoder.embed_tokens.weight": rn(vocab, d, std=2.0 / d ** 0.5), "decoder.embed_positions.weight": rn(max_pos + 2, d, std=0.5),
          "decoder.final_layer_norm.weight": (1 + rn(d, std=0.2).float()).half(), "decoder.final_layer_norm.bias": rn(d, std=0.1)}
    for l in range(n_layers):
        p = f"decoder.layers.{l}."
        for n, (o, i) in {"self_attn.q_proj": (d, d), "self_attn.k_proj": (d, d), "self_attn.v_proj": (d, d),
                          "self_attn.out_proj": (d, d), "fc1": (ffn, d), "fc2": (d, ffn)}.items():
            st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
            st[p + n + ".bias"] = rn(o, std=0.1)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            st[p + n + ".weight"] = (1 + rn(d, std=0.2).float()).half()
            st[p + n + ".bias"] = rn(d, std=0.1)
    return st, dict(n_layers=n_layers, d_model=d, n_heads=heads, ffn_dim=ffn, vocab=vocab, max_pos=max_pos)


def _torch_fp32_logp(st, dims, seq):
    import torch
    F = torch.nn.functional
    W = {k: v.float() for k, v in st.items()}
    d, H = dims["d_model"], dims["n_heads"]
    hd = d // H
    ids = torch.as_tensor(np.asarray(seq, np.int64), device="cuda")
    n = len(seq)
    x = W["decoder.embed_tokens.weight"][ids] + W["decoder.embed_positions.weight"][torch.arange(n, device="cuda") + 2]
    p = "decoder.layers.0."
    h = F.layer_norm(x, (d,), W[p + "self_attn_layer_norm.weight"], W[p + "self_attn_layer_norm.bias"], 1e-5)
    q = F.linear(h, W[p + "self_attn.q_proj.weight"], W[p + "self_attn.q_proj.bias"]) * hd ** -0.5
    k = F.linear(h, W[p + "self_attn.k_proj.weight"], W[p + "self_attn.k_proj.bias"])
    v = F.linear(h, W[p + "self_attn.v_proj.weight"], W[p + "self_attn.v_proj.bias"])
    sh = lambda t: t.view(n, H, hd).transpose(0, 1)
    a = torch.softmax((sh(q) @ sh(k).transpose(1, 2)).masked_fill(torch.ones(n, n, device="cuda").triu(1).bool(), float("-inf")), -1)
    o = (a @ sh(v)).transpose(0, 1).reshape(n, d)
    x = x + F.linear(o, W[p + "self_attn.out_proj.weight"], W[p + "self_attn.out_proj.bias"])
    h = F.layer_norm(x, (d,), W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], 1e-5)
    x = x + F.linear(F.relu(F.linear(h, W[p + "fc1.weight"], W[p + "fc1.bias"])), W[p + "fc2.weight"], W[p + "fc2.bias"])
    h = F.layer_norm(x, (d,), W["decoder.final_layer_norm.weight"], W["decoder.final_layer_norm.bias"], 1e-5)
    lp = torch.log_softmax(h @ W["decoder.embed_tokens.weight"].T, -1)
    out = np.zeros(n)
    if n > 1:
        out[1:] = lp[torch.arange(n - 1, device="cuda"), ids[1:]].double().cpu().numpy()
    return out


@pytest.mark.parametrize("d,heads,ffn", [(4096, 32, 16384), (1024, 16, 4096), (2560, 32, 10240)])
def test_full_width_layer_against_torch_fp32(d, heads, ffn):
    st, dims = _random_opt(d, heads, ffn, 50272, 2048, seed=d)
    sc = R.OptScorer(dims, R.device_layout(st, dims), "cuda")
    rng = np.random.default_rng(d)
    seqs = [[2] + list(rng.integers(0, 50272, n - 1)) for n in (1, 2, 17, 300)]
    got = sc.token_logprobs(seqs)
    ref = [_torch_fp32_logp(st, dims, s) for s in seqs]
    allr = np.concatenate([r[1:] for r in ref])
    spread = allr.std()
    err = max(np.abs(g - r).max() for g, r in zip(got, ref))
    print(f"d {d} head dim {d // heads}: max |dlogp| {err:.3e}, std of reference log-probs {spread:.3f}")
    assert spread > 0.3 and err <= 0.01 * spread
    lp = 0.25
    s = sc.score(seqs, lp)
    assert s[0] == np.float32(-1 * lp)   # a 1-token sequence scores -n * length_penalty
    np.testing.assert_allclose(s, [r.sum() - len(r) * lp for r in ref], rtol=0, atol=0.01 * spread * 300)


def test_bad_input_returns_errors():
    import torch
    import b2t_native as N
    sc, _, _ = _tiny()
    with pytest.raises(RuntimeError, match="outside"):
        sc.score([[2, 5, 272]])
    with pytest.raises(RuntimeError, match="max_pos"):
        sc.score([[2] * 129])
    lib = N.load()
    desc = N.ClmDesc.from_buffer_copy(sc.desc)
    desc.n_heads = 4   # head dim 32
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    out = torch.empty(1, dtype=torch.float32, device="cuda")
    ids = np.array([2, 3], np.int32); off = np.array([0, 2], np.int32)
    rc = lib.b2t_clm_score_f16(C.byref(desc), ids.ctypes.data, off.ctypes.data, 1, out.data_ptr(), None, ws.data_ptr(),
                               ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and "head dim" in N.last_error()
    assert sc.score([[2, 5, 7]]).shape == (1,)   # the device is still usable


def test_service_end_to_end_with_hip_decoder():
    import evaluate_model_helpers as H
    import lm_decoder, ngram_lm
    from remote_lm import LocalLMService
    sc, _, gold = _tiny()
    Cc = 41
    prons = ngram_lm.synthetic_lexicon(200, Cc, seed=5)
    lex = ngram_lm.Lexicon(prons, Cc)
    wlm = ngram_lm.SparseNGramLM.from_arpa(ngram_lm.synthetic_word_arpa(lex.words, 2, 400, seed=2), lex.words)
    res = lm_decoder.DecodeResource("", "", "", "", "")
    res.set_lexicon_lm(lex, wlm, sil=1)
    opts = lm_decoder.DecodeOptions(7000, 200, 17.0, 8.0, 0.35, 0.95, 0.0, 10)
    opts.lm_alpha, opts.lm_beta = 0.8, 0.0
    dec = lm_decoder.BrainSpeechDecoder(res, opts, max_len=128)
    tok = R.WordTokenizer(**gold["tokenizer"])
    r = LocalLMService(dec, acoustic_scale=0.35, blank_penalty=9.0, nbest=10, llm=(sc, tok), do_opt=1, alpha=0.5,
                       top_candidates_to_augment=5)
    rs = np.random.RandomState(0)
    words = [lex.words[i] for i in rs.randint(0, 200, size=4)]
    frames = []
    for w in words:
        for c in list(prons[w][0]) + [1]:
            frames += [c, 0]
    lg = np.full((len(frames), Cc), -1.0, dtype=np.float32)
    for t, c in enumerate(frames):
        lg[t, c] = 2.0
    seen = H.get_current_redis_time_ms(r)
    H.reset_remote_language_model(r, seen)
    H.send_logits_to_remote_lm(r, 'remote_lm_input', 'remote_lm_output_partial', seen, lg)
    _, out = H.finalize_remote_lm(r, 'remote_lm_output_final', seen)
    nb = [[d.sentence, d.ac_score, d.lm_score] for d in dec.result()[:10]]
    nb = R.augment_nbest(nb, top_candidates_to_augment=5, acoustic_scale=0.35)
    best, lines = R.gpt2_lm_decode(sc, tok, "cuda", nb, 0.35, length_penalty=0.0, alpha=0.5, current_context_str="")
    llm = out['candidate_llm_scores']
    assert 1 <= len(llm) <= len(nb) and all(v != 0.0 for v in llm)
    assert r.streams['remote_lm_output_final'][-1][1][b'lm_response_final'].decode() == best
