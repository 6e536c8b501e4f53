"""llm_rescore's host side against the reference's own outputs (tests/golden/llm_rescore.json, make_llm_golden.py):
get_string_differences, augment_nbest, gpt2_lm_decode with a scorer that replays the reference's recorded LLM scores; the
checkpoint loader in its four on-disk forms and its refusals; remote_lm.LocalLMService's finalize with do_opt / augmentation."""
import json
import os

import numpy as np
import pytest

import llm_rescore as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "llm_rescore.json")) as f:
        return json.load(f)


class _Replay:
    """Scorer stub: returns the reference's recorded scores, one list per call (fp32, as the reference's numpy scores)."""

    def __init__(self, calls):
        self.calls = [np.array(c, dtype=np.float32) for c in calls]
        self.seen = []

    def score(self, ids, length_penalty):
        self.seen.append([list(map(int, s)) for s in ids])
        return self.calls.pop(0)


def test_string_differences(gold):
    for c in gold["string_differences"]:
        cost, path, spans = R.get_string_differences(c["cue"], c["out"])
        assert (cost, path, [list(s) for s in spans]) == (c["cost"], c["path"], c["spans"])


def test_augment_nbest_matches_reference(gold):
    for c in gold["augment"]:
        res = R.augment_nbest([list(e) for e in c["nbest"]], top_candidates_to_augment=c["top"],
                              acoustic_scale=c["acoustic_scale"], score_penalty_percent=c["penalty"])
        assert [[e[0], float(e[1]), float(e[2])] for e in res] == c["result"]


def test_gpt2_lm_decode_matches_reference(gold):
    tok = R.WordTokenizer(**gold["tokenizer"])
    for c in gold["decode"]:
        model = _Replay(c["llm_calls"])
        r = R.gpt2_lm_decode(model, tok, "cpu", c["nbest"], 0.35, length_penalty=c["length_penalty"], alpha=c["alpha"],
                             returnConfidence=c["confidence"], current_context_str=c["context"])
        assert r[0] == c["best"] and r[1] == c["nbest_out"]
        if c["confidence"]:
            assert float(r[2]) == c["conf_value"]
        # the scorer saw the reference's token sequences: BOS + one id per word of the normalised, context-prefixed hypothesis
        assert all(s[0] == 2 for s in model.seen[0])


# ---- loader ------------------------------------------------------------------------------------------------------------
def _tiny_opt(**over):
    transformers = pytest.importorskip("transformers")
    import torch
    cfg = dict(vocab_size=100, hidden_size=64, num_hidden_layers=2, ffn_dim=128, num_attention_heads=1, max_position_embeddings=32,
               word_embed_proj_dim=64, do_layer_norm_before=True, activation_function="relu")
    cfg.update(over)
    torch.manual_seed(0)
    m = transformers.OPTForCausalLM(transformers.OPTConfig(**cfg))
    with torch.no_grad():
        for p in m.parameters():
            p.add_(0.05 * torch.randn_like(p))
    return m


def _save_forms(m, root):
    import torch
    forms = {}
    d = os.path.join(root, "bin"); m.save_pretrained(d, safe_serialization=False); forms["bin"] = d
    d = os.path.join(root, "st"); m.save_pretrained(d, safe_serialization=True); forms["safetensors"] = d
    d = os.path.join(root, "sharded"); m.save_pretrained(d, safe_serialization=True, max_shard_size="20KB"); forms["sharded"] = d
    d = os.path.join(root, "noprefix"); os.makedirs(d)
    m.config.to_json_file(os.path.join(d, "config.json"))
    sd = {k[len("model."):]: v.clone() for k, v in m.state_dict().items() if k.startswith("model.")}
    torch.save(sd, os.path.join(d, "pytorch_model.bin"))
    forms["noprefix"] = d
    return forms


def test_loader_forms_identical(tmp_path):
    import torch
    m = _tiny_opt()
    forms = _save_forms(m, str(tmp_path))
    assert any(f.endswith(".index.json") for f in os.listdir(forms["sharded"]))
    loaded = {k: R.load_opt_arrays(d) for k, d in forms.items()}
    dims0, a0 = loaded["bin"]
    assert dims0 == dict(n_layers=2, d_model=64, n_heads=1, ffn_dim=128, vocab=100, max_pos=32)
    for name, (dims, arrs) in loaded.items():
        assert dims == dims0 and sorted(arrs) == sorted(a0), name
        for k in a0:
            assert arrs[k].dtype == torch.float16 and torch.equal(arrs[k], a0[k]), (name, k)
    sd = {k: v.half() for k, v in m.state_dict().items()}
    assert a0["embed_tokens"].shape == (256, 64) and torch.equal(a0["embed_tokens"][:100], sd["model.decoder.embed_tokens.weight"])
    assert not a0["embed_tokens"][100:].any()
    q = sd["model.decoder.layers.1.self_attn.q_proj.weight"]; v = sd["model.decoder.layers.1.self_attn.v_proj.weight"]
    assert a0["layers.1.qkv_w"].shape == (256, 64)
    assert torch.equal(a0["layers.1.qkv_w"][:64], q) and torch.equal(a0["layers.1.qkv_w"][128:192], v)
    assert torch.equal(a0["layers.1.fc2_w"][:64], sd["model.decoder.layers.1.fc2.weight"])
    assert a0["embed_positions"].shape == (34, 64)


def test_loader_resolves_hub_cache_and_never_downloads(tmp_path):
    m = _tiny_opt()
    snap = tmp_path / "models--org--tiny" / "snapshots" / "abc123"
    m.save_pretrained(str(snap))
    (tmp_path / "models--org--tiny" / "refs").mkdir()
    (tmp_path / "models--org--tiny" / "refs" / "main").write_text("abc123")
    assert R.resolve_model_dir("org/tiny", str(tmp_path)) == str(snap)
    with pytest.raises(FileNotFoundError, match="never downloaded"):
        R.resolve_model_dir("org/absent", str(tmp_path))


@pytest.mark.parametrize("over,msg", [(dict(do_layer_norm_before=False), "post-LN"),
                                      (dict(word_embed_proj_dim=32), "word_embed_proj_dim"),
                                      (dict(activation_function="gelu"), "activation"),
                                      (dict(num_attention_heads=4), "head dim")])
def test_loader_refuses_unsupported(tmp_path, over, msg):
    m = _tiny_opt(**over)
    m.save_pretrained(str(tmp_path))
    with pytest.raises(ValueError, match=msg):
        R.load_opt_arrays(str(tmp_path))


# ---- the service ---------------------------------------------------------------------------------------------------------
class _Res:
    def __init__(self, s, a, l):
        self.sentence, self.ac_score, self.lm_score = s, a, l


class _Dec:
    def __init__(self, res):
        self._res, self.rescored = res, 0

    def Reset(self): pass

    def FinishDecoding(self): pass

    def Rescore(self): self.rescored += 1

    def result(self): return self._res


NB = [_Res("the cat sat", -10.0, -3.0), _Res("a bat sat", -11.0, -2.0), _Res("a cat", -9.0, -6.0), _Res("the hat sat", -30.0, -2.0)]


class _LenScorer:
    """Scores a sequence by -(sum of ids) / 100: deterministic, favours 'a cat'-like low ids."""

    def score(self, ids, lp):
        return np.array([-float(np.sum(s)) / 100.0 - len(s) * lp for s in ids], dtype=np.float32)


def _finalize(r):
    import evaluate_model_helpers as H
    t0 = H.get_current_redis_time_ms(r)
    H.reset_remote_language_model(r, t0)
    r.xadd("remote_lm_finalize", {"done": 0})
    return r.streams["remote_lm_output_final"][-1][1]


def test_service_defaults_unchanged():
    from remote_lm import LocalLMService
    r = LocalLMService(_Dec(NB), acoustic_scale=0.5, decode_fn=lambda *a: None)
    out = _finalize(r)
    expect = ";".join(";".join(map(str, [d.sentence, d.ac_score, d.lm_score, 0.0, 0.5 * d.ac_score + d.lm_score])) for d in NB)
    assert out == {b"lm_response_final": b"the cat sat", b"scoring": expect.encode(), b"context_str": b""}


def test_service_do_opt_wire_format():
    from remote_lm import LocalLMService
    tok = R.WordTokenizer(50)
    dec = _Dec(NB)
    r = LocalLMService(dec, acoustic_scale=0.5, alpha=0.5, decode_fn=lambda *a: None, llm=(_LenScorer(), tok))
    r.xadd("remote_lm_update_params", {"do_opt": 1, "rescore": 1, "top_candidates_to_augment": 4, "length_penalty": 0.0,
                                       "score_penalty_percent": 0.01})
    r.set("contextual_decoding_current_context", "so then")
    out = _finalize(r)
    assert dec.rescored == 1 and out[b"context_str"] == b"so then"
    nb = R.augment_nbest([[d.sentence, d.ac_score, d.lm_score] for d in NB], top_candidates_to_augment=4, acoustic_scale=0.5)
    assert len(nb) > len(NB)
    hyps = ["so then " + e[0] for e in nb]
    llm = _LenScorer().score([tok([h])["input_ids"][0] for h in hyps], 0.0)
    total = 0.5 * np.array([e[1] for e in nb]) + 0.5 * np.array([e[2] for e in nb]) + 0.5 * llm
    assert out[b"lm_response_final"].decode() == nb[int(np.argmax(total))][0]
    fields = out[b"scoring"].decode().split(";")
    assert len(fields) == 5 * len(nb)
    llm_col = [float(x) for x in fields[3::5]]
    assert all(v != 0.0 for v in llm_col) and np.allclose(llm_col, llm)
    assert [float(x) for x in fields[4::5]] == pytest.approx(list(total))
