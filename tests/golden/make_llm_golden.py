#!/usr/bin/env python3
"""Pins llm_rescore to the reference's LLM stage (language_model/language-model-standalone.py :127-411).

1. A seeded tiny OPTForCausalLM (transformers; vocab 272, d 128, 2 layers, 2 heads of 64 -- the smallest head dim the HIP
   kernels run --, ffn 256, max_pos 128), weights rounded to fp16-exact values, spread so that the log-probs are far from
   uniform.  Ragged id sequences with HF's fp32 per-token log-probs and scores.
2. The reference's own get_string_differences / augment_nbest / gpt2_lm_decode on recorded n-best lists, the module imported
   with its heavy imports (redis, lm_decoder) stubbed; gpt2_lm_decode rescoring with the tiny model and
   llm_rescore.WordTokenizer (its LLM scores recorded per call, for a stub scorer on machines without the reference).

Writes tests/golden/llm_rescore.npz (weights, ids, HF log-probs) and tests/golden/llm_rescore.json (n-best cases).  Run in
the build container (needs the reference checkout and transformers).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "nejm-brain-to-text_amd"))
REF = "/root/reference/language_model/language-model-standalone.py"

CFG = dict(vocab_size=272, hidden_size=128, num_hidden_layers=2, ffn_dim=256, num_attention_heads=2, max_position_embeddings=128,
           do_layer_norm_before=True, word_embed_proj_dim=128, activation_function="relu", dropout=0.0, attention_dropout=0.0,
           layerdrop=0.0, pad_token_id=1, bos_token_id=2, eos_token_id=2, init_std=0.02)
LENGTHS = [1, 2, 3, 5, 9, 17, 31, 33, 40, 64, 100, 128]


def tiny_model(seed=0):
    from transformers import OPTConfig, OPTForCausalLM
    torch.manual_seed(seed)
    m = OPTForCausalLM(OPTConfig(**CFG)).float().eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith("embed_tokens.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.15)
            elif name.endswith("embed_positions.weight"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
            elif "layer_norm" in name and name.endswith("weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * (1.5 / p.shape[1] ** 0.5))
            p.copy_(p.half().float())
    return m


def hf_logprobs(m, seqs):
    out = []
    with torch.no_grad():
        for s in seqs:
            lp = torch.log_softmax(m(input_ids=torch.tensor([s])).logits[0].double(), -1)
            tok = np.zeros(len(s), np.float64)
            for t in range(1, len(s)):
                tok[t] = lp[t - 1, s[t]].item()
            out.append(tok)
    return out


def load_reference():
    for name in ("redis", "lm_decoder"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("lm_standalone_ref", REF)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


NBEST_CASES = [
    # equal word counts, several substitutions
    [["the cat sat on the mat", -10.0, -3.0], ["the bat sat on the hat", -11.0, -2.5], ["a cat sat in the mat", -12.0, -4.0],
     ["the cat sat on a mat", -10.5, -3.2], ["the cat sat", -20.0, -1.0]],
    # unequal counts, duplicates, ties, punctuation and an empty hypothesis
    [["i want to go home .", -5.0, -2.0], ["i want to go home .", -5.0, -2.0], ["i want go home", -6.0, -1.0],
     ["", -1.0, -0.5], ["you want to go home ?", -5.5, -2.2], ["i went to go home ,", -5.0, -2.0], ["i want to > go home", -7.0, -3.0]],
    # ties in the total score, single words
    [["yes", -1.0, -1.0], ["no", -1.0, -1.0], ["maybe", -2.0, 0.5], ["yes no", -3.0, -3.0], ["no yes", -3.0, -3.0]],
    # one candidate
    [["hello there", -2.0, -1.5]],
]
STRING_PAIRS = [("the cat sat on the mat", "the bat sat on the hat"), ("a b c d", "a c d"), ("a c d", "a b c d"),
                ("x y z", "p q r"), ("", "a b"), ("a b", ""), ("one two two three", "one two three three")]


def main():
    ref = load_reference()
    import llm_rescore
    m = tiny_model()
    rng = np.random.default_rng(7)
    seqs = [[2] + list(rng.integers(0, CFG["vocab_size"], n - 1)) for n in LENGTHS]
    tok = hf_logprobs(m, seqs)
    arrays = {"w/" + k: v.detach().half().numpy() for k, v in m.state_dict().items() if k != "lm_head.weight"}
    arrays["ids"] = np.concatenate(seqs).astype(np.int32)
    arrays["seq_off"] = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int32)
    arrays["tok_logp"] = np.concatenate(tok).astype(np.float64)
    arrays["scores"] = np.array([t.sum() for t in tok])
    np.savez_compressed(os.path.join(HERE, "llm_rescore.npz"), **arrays)

    tokenizer = llm_rescore.WordTokenizer(CFG["vocab_size"])
    real = ref.rescore_with_gpt2
    calls = []

    def recording(model, tk, device, hyps, lp):
        s = real(model, tk, device, hyps, lp)
        calls.append([float(x) for x in s])
        return s
    ref.rescore_with_gpt2 = recording
    out = {"config": CFG, "tokenizer": {"vocab_size": CFG["vocab_size"], "bos_id": 2, "pad_id": 1},
           "string_differences": [], "augment": [], "decode": []}
    for a, b in STRING_PAIRS:
        c, p, spans = ref.get_string_differences(a, b)
        out["string_differences"].append({"cue": a, "out": b, "cost": c, "path": p, "spans": [list(x) for x in spans]})
    for ci, nb in enumerate(NBEST_CASES):
        for top, ac, pen in ((20, 0.3, 0.01), (2, 1.0, 0.05), (0, 0.3, 0.01)):
            res = ref.augment_nbest([list(e) for e in nb], top_candidates_to_augment=top, acoustic_scale=ac, score_penalty_percent=pen)
            out["augment"].append({"case": ci, "nbest": nb, "top": top, "acoustic_scale": ac, "penalty": pen,
                                   "result": [[e[0], float(e[1]), float(e[2])] for e in res]})
        for ctx, lp, alpha, conf in ((None, 0.0, 0.5, True), ("well then", 0.1, 0.55, True), ("   ", 0.0, 0.8, False)):
            aug = ref.augment_nbest([list(e) for e in nb], top_candidates_to_augment=20, acoustic_scale=0.35)
            nbest = [[e[0], float(e[1]), float(e[2])] for e in aug] if ci % 2 == 0 else [list(e) for e in nb]
            calls.clear()
            r = ref.gpt2_lm_decode(m, tokenizer, "cpu", nbest, 0.35, length_penalty=lp, alpha=alpha, returnConfidence=conf,
                                   current_context_str=ctx)
            out["decode"].append({"case": ci, "nbest": nbest, "context": ctx, "length_penalty": lp, "alpha": alpha,
                                  "confidence": conf, "llm_calls": list(calls), "best": r[0], "nbest_out": r[1],
                                  "conf_value": float(r[2]) if conf else None})
    with open(os.path.join(HERE, "llm_rescore.json"), "w") as f:
        json.dump(out, f, indent=1)
    lp_all = arrays["tok_logp"][arrays["tok_logp"] != 0]
    print("wrote llm_rescore.npz/.json; log-prob mean %.3f std %.3f (uniform %.3f)" % (lp_all.mean(), lp_all.std(), -np.log(272)))


if __name__ == "__main__":
    main()
