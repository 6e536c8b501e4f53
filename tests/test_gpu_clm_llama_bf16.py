"""b2t_clm_llama_score_bf16 / b2t_clm_llama_score_tree_bf16 (csrc/causal_lm_llama_bf16.hip) on the MI355X, driven through the
C ABI: against the float64 restatement of the contract with bf16 roundings (ref_logp_llama_fmt of
tests/test_clm_llama_bf16_host.py, on the GPU here), tree against flat and both forced tile modes byte for byte, the range that
fp16 lacks, one full width, the bit identities of the fp16 path, and the Python surface up to the service.

Every call (_call) gets a fresh workspace of exactly the size the library asks for (b2t_clm_llama_ws_bytes /
b2t_clm_llama_tree_ws_bytes: the elements are 2 bytes in either format), filled with 0xFF (NaN in bf16, fp16 and fp32), with
canaries behind it and behind both outputs.

The contract bound is the project's own form: e_bf16 = max |bf16-rounded restatement - unrounded restatement| is what the
contract's roundings alone do to the log-probs of that case, and the kernels must be within 3 x e_bf16 of the rounded
restatement (the margin covers accumulation order and the fast exponentials).  e_bf16 <= 0.1 is asserted first, so the bound
is never looser than 0.3 on log-probs of magnitude up to 15.  The measured figures are in NOTES.md ("LLM")."""
import numpy as np
import pytest

import llm_rescore as R
from test_clm_llama_bf16_host import E_BF16_MAX, LENS, bf16_model, ref_logp_llama_fmt, scaled_state
from test_clm_llama_host import TINY, hf_inv_freq, ref_dims, state_of, tiny_seqs
from test_gpu_clm_llama import WIDTHS, _call, _prod_list, _same

pytestmark = pytest.mark.gpu


def _flat_and_tree(sc, seqs, mode=None):
    """Both calls; asserts tree == flat byte for byte in scores and log-probs, returns the flat results."""
    fs, ft = _call(sc, seqs, False, mode)
    ts, tt = _call(sc, seqs, True, mode)
    assert fs.tobytes() == ts.tobytes() and _same(ft, tt), "tree != flat"
    assert all(t[0] == 0 for t in ft)
    return fs, ft


def _scorer(st, cfg, dtype="bfloat16"):
    import torch
    dims = R.llama_dims(cfg)
    wdt = R.clm_dtype(dtype)
    sc = R.LlamaScorer(dims, R.llama_device_layout(st, dims, R.rope_inv_freq(cfg), dtype=wdt), "cuda", dtype=dtype)
    assert sc.dtype is wdt and sc.w["embed_tokens"].dtype == wdt and sc.w["rope_cos"].dtype == torch.float32
    return sc


_TINY = {}


def _tiny(name, **over):
    """(bf16 LlamaScorer, CPU state dict, GPU state dict, config, reference dims, inv_freq) of a tiny model with bf16-valued
    weights, cached."""
    key = (name, tuple(sorted(over.items())))
    if key not in _TINY:
        model, cfg = bf16_model(name, **over)
        st = state_of(model, TINY[name]["tie_word_embeddings"])
        _TINY[key] = (_scorer(st, cfg), st, {k: v.cuda() for k, v in st.items()}, cfg, ref_dims(cfg), hf_inv_freq(model))
    return _TINY[key]


def _contract(tag, got, st, rd, inv, seqs):
    """Asserts got against the bf16-rounded restatement within 3 x e_bf16, e_bf16 <= 0.1; prints the figures first."""
    ref = np.concatenate(ref_logp_llama_fmt(st, rd, inv, seqs, "bfloat16"))
    exact = np.concatenate(ref_logp_llama_fmt(st, rd, inv, seqs, None))
    g = np.concatenate(got)
    assert g.shape == ref.shape
    e = float(np.abs(ref - exact).max())
    err = float(np.abs(g - ref).max())
    print(f"CLM llama bf16 contract {tag}: tokens {len(g)} max |dlogp| {err:.3e}  e_bf16 {e:.3e}  ratio {err / e:.3f}  "
          f"(max |logp| {np.abs(ref).max():.2f})")
    assert 0 < e <= E_BF16_MAX, (tag, e)
    assert err <= 3 * e, (tag, err, e)


def _contract_seqs(V):
    seqs = tiny_seqs(V, seed=3, lens=LENS)
    return seqs + [seqs[5][:20] + [7, 8, 9], seqs[5][:20] + [7, 8, 10], list(seqs[9])]    # shared prefixes and a duplicate


# ---- against the contract -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TINY))
def test_tiny_models_against_the_bf16_contract(name):
    """Flat and tree (bit-identical) against the bf16-rounded float64 restatement; B2T_CLM_GEMM_256 = 0 and 2 (how these
    shapes reach the 256-tile kernels) give the default's bytes.  Group sizes 2, 4, 1 and 8, head dims 64 and 128, biases,
    tied and untied heads, llama3 frequency scaling.

    Measured on an MI355X: see NOTES.md ("LLM")."""
    sc, _, st, _, rd, inv = _tiny(name)
    seqs = _contract_seqs(rd["vocab"])
    fs, got = _flat_and_tree(sc, seqs)
    _contract(f"tiny {name}", got, st, rd, inv, seqs)
    for mode in ("0", "2"):
        s, t = _call(sc, seqs, False, mode)
        assert s.tobytes() == fs.tobytes() and _same(t, got), mode
        assert _same(_call(sc, seqs, True, mode)[1], got), mode


def test_bf16_has_the_range_fp16_lacks():
    """Tiny llama with up_proj * 2^14 and down_proj * 2^-14, the same function: the bf16 scorer returns the unscaled model's
    bytes, all finite; the fp16 scorer of the same (fp16-finite) weights overflows at silu(gate) * up."""
    import torch
    _, st, _, cfg, rd, _ = _tiny("llama")
    big = scaled_state(st, rd["n_layers"])
    assert all(torch.isfinite(v.half()).all() for v in big.values())
    seqs = tiny_seqs(rd["vocab"], seed=3, lens=LENS)
    s0, t0 = _call(_tiny("llama")[0], seqs)
    s1, t1 = _call(_scorer(big, cfg), seqs)
    assert s1.tobytes() == s0.tobytes() and _same(t1, t0)
    assert np.isfinite(np.concatenate(t1)).all() and np.isfinite(s1).all()
    s16, t16 = _call(_scorer(big, cfg, "float16"), seqs, finite=False)
    t16 = np.concatenate(t16)
    print(f"CLM llama fp16 on the scaled model: {int(np.isfinite(t16).sum())} of {len(t16)} log-probs finite, "
          f"{int(np.isfinite(s16).sum())} of {len(s16)} scores")
    assert not np.isfinite(t16).all() and not np.isfinite(s16).all()
    # the unscaled model is fine in fp16: it is the scaling that fp16 cannot hold
    assert np.isfinite(np.concatenate(_call(_scorer(st, cfg, "float16"), seqs)[1])).all()


def test_full_width_layer_against_the_bf16_contract():
    """One layer plus the head at the Llama-3.2-1B width (d 2048, 32 / 8 heads, F 8192, 128256 tied columns): the contract,
    tree = flat, and both forced tile modes."""
    import torch
    d, Hq, Hkv, Fd, V, bias, tied, theta = WIDTHS["llama3.2-1b"]
    hd = d // Hq
    g = torch.Generator(device="cuda").manual_seed(d + V)
    rn = lambda *s, std: (torch.randn(*s, generator=g, device="cuda") * std).bfloat16()
    st = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "model.norm.weight": (1 + rn(d, std=0.2).float()).bfloat16()}
    p = "model.layers.0."
    for n, (o, i) in {"self_attn.q_proj": (Hq * hd, d), "self_attn.k_proj": (Hkv * hd, d), "self_attn.v_proj": (Hkv * hd, d),
                      "self_attn.o_proj": (d, d), "mlp.gate_proj": (Fd, d), "mlp.up_proj": (Fd, d),
                      "mlp.down_proj": (d, Fd)}.items():
        st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
    for n in ("input_layernorm", "post_attention_layernorm"):
        st[p + n + ".weight"] = (1 + rn(d, std=0.2).float()).bfloat16()
    cfg = dict(model_type="llama", hidden_size=d, num_attention_heads=Hq, num_key_value_heads=Hkv, intermediate_size=Fd,
               vocab_size=V, num_hidden_layers=1, max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=theta,
               tie_word_embeddings=tied)
    assert tied and not bias
    sc = _scorer(st, cfg)
    rng = np.random.default_rng(d)
    seqs = [[2] + list(rng.integers(0, V, n - 1)) for n in (1, 2, 17, 33, 300)]
    seqs += [seqs[4][:120] + list(rng.integers(0, V, 30)), seqs[4][:120] + list(rng.integers(0, V, 5))]
    fs, got = _flat_and_tree(sc, seqs)
    _contract("llama3.2-1b", got, st, ref_dims(cfg), R.rope_inv_freq(cfg), seqs)
    for mode in ("0", "2"):
        s, t = _flat_and_tree(sc, seqs, mode)
        assert s.tobytes() == fs.tobytes() and _same(t, got), mode


# ---- bit identity ---------------------------------------------------------------------------------------------------------
def test_score_alone_equals_score_in_a_batch():
    sc, _, _, _, rd, _ = _tiny("llama")
    V = rd["vocab"]
    probe = _prod_list(V, seed=11, cands=1)[0] + [9, 9, 9]
    others = _prod_list(V, seed=5, cands=99)
    s0, t0 = _call(sc, [probe], False)
    for pos in (0, 50, 99):
        batch = others[:pos] + [probe] + others[pos:]
        for tree in (False, True):
            s, t = _call(sc, batch, tree)
            assert s[pos].tobytes() == s0[0].tobytes() and t[pos].tobytes() == t0[0].tobytes(), (pos, tree)
    assert _call(sc, [probe], False, with_tok=False)[0].tobytes() == s0.tobytes()
    assert _call(sc, [probe], False, fill=0)[0].tobytes() == s0.tobytes()


@pytest.mark.parametrize("name", ["llama", "qwen2"])
def test_tree_equals_flat_at_the_block_edges(name):
    """The first owned position of the later candidates at the 32-row block edges (head dims 64 and 128), then duplicates, a
    forest and one-token sequences."""
    sc, _, _, _, rd, _ = _tiny(name)
    V = rd["vocab"]
    rng = np.random.default_rng(5)
    r = lambda n: list(rng.integers(4, V, n))
    for own in (31, 32, 33, 63, 64, 65):
        ctx = [2] + r(own - 1)
        seqs = [ctx + r(int(n)) for n in rng.integers(1, 40, 12)]
        assert all(s[:own] == ctx for s in seqs)
        _flat_and_tree(sc, seqs)
    a, b = [2] + r(20), [2] + r(7)
    _flat_and_tree(sc, [a, b, a, a, b])
    _flat_and_tree(sc, [[2] + r(5), [3] + r(5), [2, 5, 7], [3, 5]])
    _flat_and_tree(sc, [[2], [2], [3], [2], [4]])


def test_sequence_of_exactly_max_pos():
    """A 512-token sequence at max_pos = 512 (the rotary table's last row, llama3 scaling far beyond its original 64),
    beside short ones, against the restatement; one token more is refused under the bf16 entry point's name."""
    sc, _, st, _, rd, inv = _tiny("llama3")
    assert sc.desc.max_pos == 512
    seqs = tiny_seqs(rd["vocab"], seed=6, lens=(512, 5, 33))
    _, got = _flat_and_tree(sc, seqs)
    _contract("max_pos 512 llama3", got, st, rd, inv, seqs)
    with pytest.raises(RuntimeError, match="b2t_clm_llama_score_bf16.*max_pos"):
        sc.score([[2] * 513])
    with pytest.raises(RuntimeError, match="b2t_clm_llama_score_tree_bf16.*outside"):
        sc.score([[2, 5, rd["vocab"]]], share_prefixes=True)
    assert sc.score([[2, 5, 7]]).shape == (1,)   # the device is still usable


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_python_surface_and_the_service(tmp_path):
    """A bf16 checkpoint on disk: build_scorer(dtype="auto") gives a bf16 LlamaScorer whose score / token_logprobs are the
    direct ABI call's with share_prefixes on and off; dtype=None on the same directory gives the fp16 scorer; LocalLMService
    runs end to end with the bf16 scorer."""
    import torch
    model, cfg = bf16_model("qwen2")
    st = {k: v.clone() for k, v in state_of(model, True).items()}
    model.to(torch.bfloat16).save_pretrained(str(tmp_path))
    sc = R.build_scorer(str(tmp_path), dtype="auto")
    assert isinstance(sc, R.LlamaScorer) and sc.dtype is torch.bfloat16 and sc.device.type == "cuda"
    direct = _scorer(st, cfg)
    for k, v in direct.w.items():
        assert torch.equal(sc.w[k].view(torch.uint8), v.view(torch.uint8)), k      # the checkpoint's values, kept exactly
    V = cfg["vocab_size"]
    seqs = tiny_seqs(V, seed=8, lens=(1, 9, 40))
    s, t = _call(direct, seqs, False)
    for tree in (False, True):
        assert _same(sc.token_logprobs(seqs, share_prefixes=tree), t)
        assert sc.last_stats == {"tokens": 50, "nodes": 48 if tree else 50}
        assert sc.score(seqs, 0.25, share_prefixes=tree).tobytes() == (s - np.array([1, 9, 40]) * 0.25).astype(np.float32).tobytes()
    sc.share_prefixes = True
    assert _same(sc.token_logprobs(seqs), t)
    s16 = R.build_scorer(str(tmp_path), dtype=None)
    assert s16.dtype is torch.float16 and s16.w["embed_tokens"].dtype == torch.float16
    t16 = s16.token_logprobs(seqs)
    assert _same(t16, _call(_scorer(st, cfg, "float16"), seqs)[1]) and not _same(t16, t)

    import evaluate_model_helpers as H
    import lm_decoder, ngram_lm
    from remote_lm import LocalLMService
    sc.share_prefixes = False
    Cc = 41
    prons = ngram_lm.synthetic_lexicon(200, Cc, seed=5)
    lex = ngram_lm.Lexicon(prons, Cc)
    wlm = ngram_lm.SparseNGramLM.from_arpa(ngram_lm.synthetic_word_arpa(lex.words, 2, 400, seed=2), lex.words)
    res = lm_decoder.DecodeResource("", "", "", "", "")
    res.set_lexicon_lm(lex, wlm, sil=1)
    opts = lm_decoder.DecodeOptions(7000, 200, 17.0, 8.0, 0.35, 0.95, 0.0, 10)
    opts.lm_alpha, opts.lm_beta = 0.8, 0.0
    dec = lm_decoder.BrainSpeechDecoder(res, opts, max_len=128)
    tok = R.WordTokenizer(vocab_size=V, bos_id=2, pad_id=1)
    r = LocalLMService(dec, acoustic_scale=0.35, blank_penalty=9.0, nbest=10, llm=(sc, tok), do_opt=1, alpha=0.5,
                       top_candidates_to_augment=5)
    rs = np.random.RandomState(0)
    words = [lex.words[i] for i in rs.randint(0, 200, size=4)]
    frames = []
    for w in words:
        for c in list(prons[w][0]) + [1]:
            frames += [c, 0]
    lg = np.full((len(frames), Cc), -1.0, dtype=np.float32)
    for i, c in enumerate(frames):
        lg[i, c] = 2.0
    seen = H.get_current_redis_time_ms(r)
    H.reset_remote_language_model(r, seen)
    H.send_logits_to_remote_lm(r, 'remote_lm_input', 'remote_lm_output_partial', seen, lg)
    _, out = H.finalize_remote_lm(r, 'remote_lm_output_final', seen)
    nb = [[d.sentence, d.ac_score, d.lm_score] for d in dec.result()[:10]]
    nb = R.augment_nbest(nb, top_candidates_to_augment=5, acoustic_scale=0.35)
    best, _ = R.gpt2_lm_decode(sc, tok, "cuda", nb, 0.35, length_penalty=0.0, alpha=0.5, current_context_str="")
    llm = out['candidate_llm_scores']
    assert 1 <= len(llm) <= len(nb) and all(v != 0.0 for v in llm)
    assert r.streams['remote_lm_output_final'][-1][1][b'lm_response_final'].decode() == best
