#!/usr/bin/env python3
"""OPT n-best rescoring throughput: b2t_clm_score_f16 against a plain-torch fp16 restatement of the same forward (F.linear on
hipBLASLt, SDPA) on the same weights.  OPT-6.7b shape (32 layers, d 4096, 32 x 128 heads, ffn 16384, vocab 50272) with random
fp16 weights (~13.3 GB); one "list" = 100 candidates of 10-40 tokens.  Prints one JSON line.

  python tools/bench_llm_rescore.py [--layers 32] [--lists 5] [--warmup 2]

The default list is 100 candidates of independent random ids: no two share a prefix beyond BOS, the one shape the service
never sees.  `--list nbest` draws what augment_nbest produces (a base sentence with single words exchanged), `--context N`
puts N shared tokens in front of every candidate (contextual decoding), and either of them, or `--tree`, switches to an A/B of
the flat call against the shared-prefix tree call (b2t_clm_score_tree_f16) in one process: the two alternate list by list
after a warm-up of both, --reps passes over the lists, and the line reports tokens, nodes and the median / min / max ms per
list of each, with the largest spread between the repeats of one list
(hip_ms_per_list = flat, hip_tree_ms_per_list = tree); the torch baseline is not run in that mode.

  python tools/bench_llm_rescore.py --list nbest --context 64 [--lists 7]

`--session` measures the context cache (b2t_clm_score_tree_cached_f16) in the closed loop it is for: a conversation of
--sentences calls, call k scoring a 100-candidate nbest list behind the context = the base sentences of the calls before it.
Per call the tree path, the cached path with B2T_CLM_TRUNK_ATTN=0 (stage A) and with 1 (stage A + B) run one after the other
in this process on the same cache state (the cache is cut back to what it held before the call in between); --reps passes
over the conversation after one untimed pass.  The line reports per call the context tokens, tree nodes, rows computed,
positions reused, the median ms of each path with the spread (max - min) over the repeats of that call, and whether all
scores were byte-identical.

  python tools/bench_llm_rescore.py --session [--sentences 12] [--reps 5]

`--arch llama` runs the Llama family's path (b2t_clm_llama_score_f16 / b2t_clm_llama_score_tree_f16 /
b2t_clm_llama_score_tree_cached_f16) at the Llama-3-8B shape (32 layers, d 4096, 32 query / 8 kv heads, ffn 14336, vocab
128256, untied head; random fp16 weights, ~16 GB twice) on the same lists under the same protocol: without --tree the HIP
path against HF's LlamaForCausalLM in fp16 on the same weights in this process (padded batch, SDPA), with --tree / --list
nbest / --context the flat call against the tree call, with --session the session comparison above.

  python tools/bench_llm_rescore.py --arch llama [--tree --context 64 | --session]

`--dtype bfloat16` (with --arch llama) runs the same in bfloat16: b2t_clm_llama_score_bf16 / b2t_clm_llama_score_tree_bf16 on
bf16 weights against HF's model in bf16.  The cached path has no bf16 form yet, so --session stays float16.

  python tools/bench_llm_rescore.py --arch llama --dtype bfloat16 [--tree --context 64]

`--arch qwen3` runs Qwen3's path (b2t_clm_qwen3_score_*: the Llama forward with the q / k RMSNorm in the QKV GEMM's epilogue)
under the protocol of --arch llama, against HF's Qwen3ForCausalLM, at the Qwen3-8B shape: 36 layers, d 4096, 32 query / 8 kv
heads of 128, ffn 12288, vocab 151936, untied head.  What the norm costs is this run beside --arch llama forced to the same
dimensions, the two alternating process by process:

  python tools/bench_llm_rescore.py --arch qwen3 --lists 7
  python tools/bench_llm_rescore.py --arch llama --layers 36 --ffn 12288 --vocab 151936 --lists 7

`--arch gpt2` runs GPT-2's path (b2t_clm_gpt2_score_f16 / _tree_f16 / _tree_cached_f16: the OPT forward with gelu_new in the fc1
GEMM's epilogue) under the protocol of --arch llama, against HF's GPT2LMHeadModel in fp16, at the GPT-2 XL shape: 48 layers,
d 1600, 25 heads of 64, ffn 6400, vocab 50257, 1024 positions, tied head.

  python tools/bench_llm_rescore.py --arch gpt2 [--tree --context 64 | --session]

`--arch olmo2` measures what OLMo-2's layer costs beside the Llama layer: an Olmo2Scorer (b2t_clm_olmo2_score_f16 / _tree_f16:
the whole-row q / k norm and the two post-norms as passes of their own over an fp32 region) and a LlamaScorer of the same
dimensions on the same random weights, in one process, alternating list by list, each on its flat and its tree path, --reps
passes over the lists after a warm-up of all four.  The OLMo-2-7B shape: 32 layers, d 4096, 32 query / 32 kv heads of 128, ffn
11008, vocab 100352, untied head.  The line reports per family and path the per-list medians with their spread, and the
ratio olmo2 / llama per list.  No HF model is built.

  python tools/bench_llm_rescore.py --arch olmo2 --lists 7 [--list nbest --context 64]

`--arch mixtral` measures what routing costs: a MixtralScorer (b2t_clm_mixtral_score_f16 / _tree_f16: router, plan, gather, two
grouped GEMMs over the rows sorted by expert, combine) at the Mixtral-8x7B shape with a few layers -- d 4096, 32 query / 8 kv
heads of 128, ffn 14336, 8 experts, top-2, vocab 32000 -- beside a dense LlamaScorer with d 4096 and ffn 28672 = top_k x 14336,
which has the same active FLOPs per row, under the protocol of --arch olmo2.  The line reports the per-list medians and the
ratio mixtral / llama per list; the sorted rows S = round_up(rows * top_k, 256) + 256 * n_experts against rows * top_k say how much
of the grouped GEMM is padding at that list length.

  python tools/bench_llm_rescore.py --arch mixtral --layers 4 --lists 7 [--cands 20] [--list nbest --context 64]

`--arch gemma2` measures Gemma-2's path (b2t_clm_gemma2_score_f16 / _tree_f16: attention at head dim 256 with the soft cap, at
one wave per SIMD; four norms per layer; GeGLU; the capped head) at the gemma-2-2b shape -- 26 layers, d 2304, 8 query / 4 kv
heads of 256, ffn 9216, vocab 256000, tied head -- beside a LlamaScorer of equal active FLOPs per row: the same d, ffn, vocab
and tied head with 18 query / 6 kv heads of 128, under the protocol of --arch olmo2.

  python tools/bench_llm_rescore.py --arch gemma2 --lists 5 --cands 5|20|100

`--arch gptoss` measures gpt-oss's path (b2t_clm_gptoss_score_bf16 / _tree_bf16: attention with sinks and a window of 128 on every
other layer, router, plan, gather, two grouped GEMMs with biases, combine) at the gpt-oss-20b shape -- d 2880, 64 query / 8 kv
heads of 64, F 2880, 32 experts top-4, vocab 201088, --layers of the 24 (default 4) -- on random bf16 weights, beside a dense
LlamaScorer of equal active matmul FLOPs per row (d 2880, 45 query / 9 kv heads of 64, ffn 12288: 4 x 2880 for the four experts
and 768 for the wider attention projections), under the protocol of --arch olmo2.  The sorted rows S against rows * top_k say how
much of the grouped GEMMs is padding.  `--experts mxfp4` makes the experts an MXFP4 checkpoint's and adds the scorer that keeps
them packed (b2t_clm_gptoss_mx_score_bf16 / _tree_bf16), alternating with the dense scorer of the same checkpoint.

  python tools/bench_llm_rescore.py --arch gptoss --lists 5 --cands 5|20|100 [--list nbest --context 64] [--experts mxfp4]

`--arch llama|qwen3 --weights fp8` measures what keeping the projections packed costs: one synthetic checkpoint in the fine-grained
FP8 spelling (weight_block_size [128, 128]; random non-NaN e4m3 codes, scales spread over three octaves) at the chosen shape,
through the dense scorer (the checkpoint expanded into --dtype) and through the Fp8LlamaScorer that unpacks in the tile GEMM
(linear_weights="fp8"), flat and tree of each alternating list by list under the protocol of --arch olmo2.  The line has both
scorers' times, their ratio per list, whether the packed scores were the dense scorer's bytes, and the bytes of the four
projections in either form (weight_bytes).  No HF model is built.

  python tools/bench_llm_rescore.py --arch llama|qwen3 --weights fp8 --layers 8 --lists 5 --cands 5|20|100 [--dtype bfloat16]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nejm-brain-to-text_amd"))


def random_list(rng, V, cands=100, context=()):
    """cands candidates of 10-40 independent random tokens, BOS first, behind the shared context tokens."""
    return [[2] + list(context) + list(rng.integers(4, V, int(n) - 1)) for n in rng.integers(10, 41, cands)]


def nbest_list(rng, V, cands=100, context=()):
    """An n-best list as augment_nbest leaves it: a base sentence of 10-40 random tokens (BOS first, the first candidate), and
    cands - 1 more made from it by replacing 1-3 positions with another id of that position's confusion set (2-4 ids, the
    base's among them).  Duplicates may occur, as they may not in the service; the scorer accepts them."""
    n = int(rng.integers(10, 41)) - 1
    conf = [rng.choice(np.arange(4, V), size=int(rng.integers(2, 5)), replace=False) for _ in range(n)]
    base = [int(c[0]) for c in conf]
    out = [[2] + list(context) + base]
    for _ in range(cands - 1):
        cand = list(base)
        for p in rng.choice(n, size=int(rng.integers(1, 4)), replace=False):
            cand[p] = int(rng.choice(conf[p][1:]))
        out.append([2] + list(context) + cand)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=("opt", "llama", "qwen3", "gpt2", "olmo2", "mixtral", "gemma2", "phi3", "gptoss"), default="opt",
                    help="opt: OPT-6.7b shape; llama: Llama-3-8B shape; qwen3: Qwen3-8B shape; gpt2: GPT-2 XL shape; "
                         "olmo2: OLMo-2-7B shape, beside the Llama forward of the same dimensions; mixtral: Mixtral-8x7B shape "
                         "with 4 layers, beside the dense Llama forward of the same active FLOPs; gemma2: gemma-2-2b shape, beside "
                         "a Llama forward of the same active FLOPs; phi3: Phi-3-mini shape (32 heads of 96), beside a Llama forward of "
                         "the same FLOPs (24 heads of 128)")
    ap.add_argument("--dtype", choices=("float16", "bfloat16"), default="float16",
                    help="--arch llama / qwen3: the compute dtype of the scorer and of the HF model beside it")
    ap.add_argument("--layers", type=int, default=None, help="default 32 (opt, llama), 36 (qwen3), 48 (gpt2)")
    ap.add_argument("--d", type=int, default=None, help="default 4096, 1600 (gpt2)")
    ap.add_argument("--heads", type=int, default=None, help="default 32, 25 (gpt2)")
    ap.add_argument("--kv-heads", type=int, default=None, help="--arch llama / qwen3 / olmo2: key / value heads; default 8, 32 (olmo2)")
    ap.add_argument("--ffn", type=int, default=None, help="default 16384 (opt), 14336 (llama), 12288 (qwen3), 6400 (gpt2), 11008 (olmo2)")
    ap.add_argument("--vocab", type=int, default=None, help="default 50272 (opt), 128256 (llama), 151936 (qwen3), 50257 (gpt2), 100352 (olmo2)")
    ap.add_argument("--experts", choices=("dense", "mxfp4"), default="dense",
                    help="--arch gptoss: mxfp4 makes the experts an MXFP4 checkpoint's and runs the scorer that keeps them packed "
                         "(expert_weights='mxfp4') beside the dense scorer of the same checkpoint")
    ap.add_argument("--weights", choices=("dense", "fp8"), default="dense",
                    help="--arch llama / qwen3: fp8 makes the checkpoint a fine-grained FP8 one and runs the scorer that keeps its "
                         "projections packed (linear_weights='fp8') beside the dense scorer of the same checkpoint")
    ap.add_argument("--cands", type=int, default=100)
    ap.add_argument("--lists", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--list", choices=("random", "nbest"), default="random", help="candidate generator (nbest: A/B with the tree path)")
    ap.add_argument("--context", type=int, default=0, help="shared tokens in front of every candidate (A/B with the tree path)")
    ap.add_argument("--tree", action="store_true", help="A/B flat against tree on the chosen list")
    ap.add_argument("--reps", type=int, default=3, help="A/B: timed passes over the lists")
    ap.add_argument("--session", action="store_true", help="tree against context cache over a growing conversation")
    ap.add_argument("--sentences", type=int, default=12, help="--session: calls of the conversation")
    a = ap.parse_args()
    a.layers = a.layers or {"qwen3": 36, "gpt2": 48, "mixtral": 4, "gemma2": 26, "gptoss": 4}.get(a.arch, 32)   # phi3: 32
    a.d = a.d or {"gpt2": 1600, "gemma2": 2304, "phi3": 3072, "gptoss": 2880}.get(a.arch, 4096)
    a.heads = a.heads or {"gpt2": 25, "gemma2": 8, "gptoss": 64}.get(a.arch, 32)
    a.kv_heads = a.kv_heads or (a.heads if a.arch in ("olmo2", "phi3") else 4 if a.arch == "gemma2" else 8)
    a.ffn = a.ffn or {"opt": 16384, "llama": 14336, "qwen3": 12288, "gpt2": 6400, "olmo2": 11008, "mixtral": 14336, "gemma2": 9216, "phi3": 8192, "gptoss": 2880}[a.arch]
    a.vocab = a.vocab or {"opt": 50272, "llama": 128256, "qwen3": 151936, "gpt2": 50257, "olmo2": 100352, "mixtral": 32000, "gemma2": 256000, "phi3": 32064, "gptoss": 201088}[a.arch]
    if a.arch == "gptoss":
        a.dtype = "bfloat16"     # the format the checkpoints are published in
    elif a.dtype != "float16" and (a.arch in ("opt", "gpt2", "olmo2", "mixtral", "gemma2", "phi3") or a.session):
        ap.error("--dtype bfloat16 needs --arch llama or qwen3 and has no --session")
    if a.arch == "gptoss":
        if a.session:
            ap.error("--arch gptoss has no --session")
        return main_gptoss(a)
    if a.arch == "mixtral":
        if a.session:
            ap.error("--arch mixtral has no --session")
        return main_mixtral(a)
    if a.arch == "gemma2":
        if a.session:
            ap.error("--arch gemma2 has no --session")
        return main_gemma2(a)
    if a.arch == "phi3":
        if a.session:
            ap.error("--arch phi3 has no --session")
        return main_phi3(a)
    if a.arch == "olmo2":
        if a.session:
            ap.error("--arch olmo2 has no --session")
        return main_olmo2(a)
    if a.arch == "gpt2":
        return main_gpt2(a)
    if a.weights == "fp8":
        if a.arch not in ("llama", "qwen3") or a.session:
            ap.error("--weights fp8 needs --arch llama or qwen3 and has no --session")
        return main_fp8(a)
    if a.arch != "opt":
        return main_llama(a)
    import torch
    import torch.nn.functional as F
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, ffn, V, L = a.d, a.heads, a.ffn, a.vocab, a.layers
    hd = d // H
    dims = dict(n_layers=L, d_model=d, n_heads=H, ffn_dim=ffn, vocab=V, max_pos=2048)
    rng = np.random.default_rng(0)
    calls = session_calls(a, rng, dims["max_pos"]) if a.session else None   # before the model is built
    dev = "cuda"
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).half()
    st = {"decoder.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "decoder.embed_positions.weight": rn(2050, d, std=0.5),
          "decoder.final_layer_norm.weight": torch.ones(d, device=dev).half(), "decoder.final_layer_norm.bias": rn(d, std=0.1)}
    for l in range(L):
        p = f"decoder.layers.{l}."
        for n, (o, i) in {"self_attn.q_proj": (d, d), "self_attn.k_proj": (d, d), "self_attn.v_proj": (d, d),
                          "self_attn.out_proj": (d, d), "fc1": (ffn, d), "fc2": (d, ffn)}.items():
            st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
            st[p + n + ".bias"] = rn(o, std=0.1)
        for n in ("self_attn_layer_norm", "final_layer_norm"):
            st[p + n + ".weight"] = torch.ones(d, device=dev).half()
            st[p + n + ".bias"] = rn(d, std=0.1)
    lay = R.device_layout({k: v for k, v in st.items()}, dims)   # (host copies; the device copies below are the scorer's)
    sc = R.OptScorer(dims, lay, dev, context_cache_tokens=dims["max_pos"] if a.session else 0)
    del lay
    if a.session:
        return session(a, sc, *calls)
    ab = a.tree or a.list != "random" or a.context > 0
    if not ab:
        lists = [random_list(rng, V, a.cands) for _ in range(a.lists)]
    else:   # the context differs from list to list, as the sentences decoded so far do
        gen = nbest_list if a.list == "nbest" else random_list
        lists = [gen(rng, V, a.cands, [int(x) for x in rng.integers(4, V, a.context)]) for _ in range(a.lists)]
    ntok = [sum(len(s) for s in l) for l in lists]
    if ab:
        return ab_flat_tree(a, sc, lists, ntok)

    def torch_score(seqs):   # padded batch, fp16 weights, causal + key-padding mask through SDPA
        B, T = len(seqs), max(len(s) for s in seqs)
        ids = torch.zeros(B, T, dtype=torch.long, device=dev)
        mask = torch.zeros(B, T, dtype=torch.bool, device=dev)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.as_tensor(s, device=dev); mask[i, :len(s)] = True
        x = st["decoder.embed_tokens.weight"][ids] + st["decoder.embed_positions.weight"][torch.arange(T, device=dev) + 2]
        am = torch.ones(T, T, dtype=torch.bool, device=dev).tril()[None, None] & mask[:, None, None, :]
        for l in range(L):
            p = f"decoder.layers.{l}."
            h = F.layer_norm(x, (d,), st[p + "self_attn_layer_norm.weight"], st[p + "self_attn_layer_norm.bias"])
            q = F.linear(h, st[p + "self_attn.q_proj.weight"], st[p + "self_attn.q_proj.bias"]) * hd ** -0.5
            k = F.linear(h, st[p + "self_attn.k_proj.weight"], st[p + "self_attn.k_proj.bias"])
            v = F.linear(h, st[p + "self_attn.v_proj.weight"], st[p + "self_attn.v_proj.bias"])
            sh = lambda t: t.view(B, T, H, hd).transpose(1, 2)
            o = F.scaled_dot_product_attention(sh(q), sh(k), sh(v), attn_mask=am, scale=1.0).transpose(1, 2).reshape(B, T, d)
            x = x + F.linear(o, st[p + "self_attn.out_proj.weight"], st[p + "self_attn.out_proj.bias"])
            h = F.layer_norm(x, (d,), st[p + "final_layer_norm.weight"], st[p + "final_layer_norm.bias"])
            x = x + F.linear(F.relu(F.linear(h, st[p + "fc1.weight"], st[p + "fc1.bias"])), st[p + "fc2.weight"], st[p + "fc2.bias"])
        h = F.layer_norm(x, (d,), st["decoder.final_layer_norm.weight"], st["decoder.final_layer_norm.bias"])
        lp = torch.log_softmax(F.linear(h, st["decoder.embed_tokens.weight"]).float(), -1)
        g = lp[:, :-1].gather(-1, ids[:, 1:, None])[..., 0] * mask[:, 1:]
        return g.sum(1).cpu().numpy()

    def timed(fn):
        for i in range(a.warmup):
            fn(lists[i % len(lists)])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [fn(l) for l in lists]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(lists) * 1e3, outs

    with torch.inference_mode():
        ms_hip, s_hip = timed(lambda l: sc.score(l))
        ms_torch, s_torch = timed(torch_score)
    diff = max(float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max()) for x, y in zip(s_hip, s_torch))
    flop_tok = 2 * (L * (4 * d * d + 2 * d * ffn) + d * V)
    tf = np.mean(ntok) * flop_tok / (ms_hip * 1e-3) / 1e12
    print(json.dumps({"bench": "llm_rescore", "layers": L, "d": d, "heads": H, "ffn": ffn, "vocab": V, "cands": a.cands,
                      "tokens_per_list": float(np.mean(ntok)), "hip_ms_per_list": round(ms_hip, 2),
                      "torch_fp16_ms_per_list": round(ms_torch, 2), "hip_tflops": round(tf, 1),
                      "speedup_vs_torch": round(ms_torch / ms_hip, 3), "max_abs_score_diff_vs_torch": round(diff, 4)}))


def main_llama(a):
    """--arch llama / qwen3: the lists and the protocol of main() with a LlamaScorer, and HF's model in the same dtype (--dtype)
    as the torch side."""
    import torch
    import transformers
    import llm_rescore as R
    torch.manual_seed(0)
    dt = R.clm_dtype(a.dtype)
    d, H, Hkv, ffn, V, L = a.d, a.heads, a.kv_heads, a.ffn, a.vocab, a.layers
    dev = "cuda"
    rng = np.random.default_rng(0)
    max_pos = 2048
    calls = session_calls(a, rng, max_pos) if a.session else None   # before the model is built
    if a.arch == "qwen3":
        cfg = transformers.Qwen3Config(hidden_size=d, num_attention_heads=H, num_key_value_heads=Hkv, head_dim=d // H,
                                       intermediate_size=ffn, vocab_size=V, num_hidden_layers=L, max_position_embeddings=max_pos,
                                       rms_norm_eps=1e-6, tie_word_embeddings=False, attn_implementation="sdpa")
    else:
        cfg = transformers.LlamaConfig(hidden_size=d, num_attention_heads=H, num_key_value_heads=Hkv, intermediate_size=ffn,
                                       vocab_size=V, num_hidden_layers=L, max_position_embeddings=max_pos, rms_norm_eps=1e-5,
                                       tie_word_embeddings=False, attn_implementation="sdpa",
                                       rope_scaling=dict(rope_type="llama3", factor=8.0, low_freq_factor=1.0, high_freq_factor=4.0,
                                                         original_max_position_embeddings=8192, rope_theta=500000.0))
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        with torch.device(dev):
            model = (transformers.Qwen3ForCausalLM if a.arch == "qwen3" else transformers.LlamaForCausalLM)(cfg).eval()
    finally:
        torch.set_default_dtype(old)
    with torch.no_grad():   # HF's init (std 0.02) gives a flat distribution; widths as in the OPT rows
        for k, p in model.named_parameters():
            if p.dim() == 2:
                std = 2.0 / d ** 0.5 if ("embed_tokens" in k or "lm_head" in k) else 1.0 / p.shape[1] ** 0.5
                p.copy_((torch.randn(p.shape, device=dev) * std).to(dt))
    cj = json.loads(cfg.to_json_string())
    dims = R.llama_dims(cj)
    sc = R.LlamaScorer(dims, R.llama_device_layout(model.state_dict(), dims, R.rope_inv_freq(cj), dtype=dt), dev,
                       context_cache_tokens=dims["max_pos"] if a.session else 0, dtype=dt)
    hd = d // H
    flop_tok = 2 * (L * (d * (H + 2 * Hkv) * hd + d * d + 3 * d * ffn) + d * V)
    return against_hf(a, sc, model, calls, rng, flop_tok, {"kv_heads": Hkv})


def main_fp8(a, block=(128, 128)):
    """--arch llama / qwen3 --weights fp8: a checkpoint in the fine-grained FP8 spelling at the chosen shape -- every linear of
    every layer uniform random non-NaN e4m3 codes with one scale 2^U(-14.5, -11.5) a block, which gives weights of about the
    usual 1 / sqrt(K) spread at K = 4096; embedding, head and norms random in --dtype -- through the dense LlamaScorer of its
    expansion and the Fp8LlamaScorer of its bytes, under the protocol of --arch olmo2."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    dt = R.clm_dtype(a.dtype)
    d, H, Hkv, ffn, V, L = a.d, a.heads, a.kv_heads, a.ffn, a.vocab, a.layers
    hd, dev, (bn, bk) = d // H, "cuda", block
    rng = np.random.default_rng(0)
    cfg = dict(model_type=a.arch, hidden_size=d, num_attention_heads=H, num_key_value_heads=Hkv, intermediate_size=ffn, vocab_size=V,
               num_hidden_layers=L, max_position_embeddings=2048, rms_norm_eps=1e-6, tie_word_embeddings=False, rope_theta=1000000.0,
               quantization_config={"quant_method": "fp8", "fmt": "e4m3", "weight_block_size": list(block), "activation_scheme": "dynamic"})
    assert R.fp8_block(cfg) == block
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).to(dt)
    nw = lambda n: (1 + 0.2 * torch.randn(n, device=dev)).to(dt)
    ok = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8, device=dev)
    st = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "lm_head.weight": rn(V, d, std=2.0 / d ** 0.5), "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        st[p + "input_layernorm.weight"], st[p + "post_attention_layernorm.weight"] = nw(d), nw(d)
        if a.arch == "qwen3":
            st[p + "self_attn.q_norm.weight"], st[p + "self_attn.k_norm.weight"] = nw(hd), nw(hd)
        for n, (o, i) in {"self_attn.q_proj": (H * hd, d), "self_attn.k_proj": (Hkv * hd, d), "self_attn.v_proj": (Hkv * hd, d),
                          "self_attn.o_proj": (d, H * hd), "mlp.gate_proj": (ffn, d), "mlp.up_proj": (ffn, d), "mlp.down_proj": (d, ffn)}.items():
            st[p + n + ".weight"] = ok[torch.randint(0, 254, (o, i), device=dev)].view(torch.float8_e4m3fn)
            st[p + n + ".weight_scale_inv"] = torch.exp2(-14.5 + 3 * torch.rand(o // bn, i // bk, device=dev))
    dims, inv = R.llama_dims(cfg), R.rope_inv_freq(cfg)
    scs = {"dense": R.LlamaScorer(dims, R.llama_device_layout(R.fp8_dense_state(st, dims, block, dt), dims, inv, dtype=dt), dev, dtype=dt),
           "fp8": R.Fp8LlamaScorer(dims, R.llama_fp8_device_layout(st, dims, inv, dt, block), dev, dtype=dt)}
    del st
    torch.cuda.empty_cache()
    dense_bytes = sum(v.numel() * v.element_size() for k, v in scs["dense"].w.items() if k.endswith(("qkv_w", "o_w", "gate_up_w", "down_w")))
    lists, ntok, nodes, same, per, stat = alternate(a, rng, V, scs, ("dense", "fp8"))
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["fp8", t], per["dense", t])]
    with torch.inference_mode():
        equal = all(scs["fp8"].score(l, share_prefixes=t).tobytes() == scs["dense"].score(l, share_prefixes=t).tobytes()
                    for l in lists for t in (False, True))
        finite = bool(np.isfinite(scs["dense"].score(lists[0])).all())
    print(json.dumps({"bench": "llm_rescore_fp8", "arch": a.arch, "dtype": a.dtype, "layers": L, "d": d, "heads": H, "kv_heads": Hkv,
                      "ffn": ffn, "vocab": V, "block": list(block), "cands": a.cands, "list": a.list, "context": a.context,
                      "lists": len(lists), "reps": max(1, a.reps), "tokens": float(np.mean(ntok)), "nodes": float(np.mean(nodes)),
                      "dense_flat_ms": stat(("dense", False)), "fp8_flat_ms": stat(("fp8", False)),
                      "dense_tree_ms": stat(("dense", True)), "fp8_tree_ms": stat(("fp8", True)),
                      "fp8_over_dense_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "fp8_over_dense_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same), "fp8_scores_are_dense_bytes": bool(equal), "scores_finite": finite,
                      "dense_weight_bytes": dense_bytes, "fp8_weight_bytes": scs["fp8"].weight_bytes()}))


def main_gpt2(a):
    """--arch gpt2: the lists and the protocol of main_llama() with a Gpt2Scorer and HF's GPT2LMHeadModel in fp16."""
    import torch
    import transformers
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, ffn, V, L = a.d, a.heads, a.ffn, a.vocab, a.layers
    dev = "cuda"
    rng = np.random.default_rng(0)
    max_pos = 1024
    calls = session_calls(a, rng, max_pos) if a.session else None   # before the model is built
    cfg = transformers.GPT2Config(n_embd=d, n_head=H, n_layer=L, n_inner=ffn, n_positions=max_pos, vocab_size=V,
                                  activation_function="gelu_new", attn_implementation="sdpa", bos_token_id=2, eos_token_id=2)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float16)
    try:
        with torch.device(dev):
            model = transformers.GPT2LMHeadModel(cfg).eval()
    finally:
        torch.set_default_dtype(old)
    with torch.no_grad():   # HF's init (std 0.02) gives a flat distribution; widths as in the other rows (Conv1D is [in][out])
        for k, p in model.named_parameters():
            if p.dim() == 2:
                std = 2.0 / d ** 0.5 if "wte" in k else 0.5 if "wpe" in k else 1.0 / p.shape[0] ** 0.5
                p.copy_((torch.randn(p.shape, device=dev) * std).half())
    dims = R.gpt2_dims(json.loads(cfg.to_json_string()))
    sc = R.Gpt2Scorer(dims, R.gpt2_device_layout(model.state_dict(), dims), dev,
                      context_cache_tokens=dims["max_pos"] if a.session else 0)
    return against_hf(a, sc, model, calls, rng, 2 * (L * (4 * d * d + 2 * d * ffn) + d * V), {})


def alternate(a, rng, V, scs, fams):
    """The protocol of --arch olmo2 / gemma2: the scorers scs[f], f in fams (the new family last), flat and tree of each
    alternating list by list in this process, --reps passes over --lists lists after a warm-up of all.  Returns (lists, tokens
    per list, nodes per list, whether flat and tree were bit-identical throughout, per (family, tree) the per-list medians in ms,
    stat(key) = their summary)."""
    import torch
    gen = nbest_list if a.list == "nbest" else random_list
    lists = [gen(rng, V, a.cands, [int(x) for x in rng.integers(4, V, a.context)]) for _ in range(a.lists)]
    ntok = [sum(len(s) for s in l) for l in lists]
    paths = (False, True)
    ms = {(f, t): [[] for _ in lists] for f in fams for t in paths}
    nodes, same = [0] * len(lists), True
    with torch.inference_mode():
        for i in range(max(1, a.warmup)):
            for f in fams:
                for t in paths:
                    scs[f].score(lists[i % len(lists)], share_prefixes=t)
        torch.cuda.synchronize()
        for _ in range(max(1, a.reps)):
            for i, l in enumerate(lists):
                for f in fams:
                    out = {}
                    for t in paths:
                        t0 = time.perf_counter()
                        out[t] = scs[f].score(l, share_prefixes=t)   # returns host scores: the call is complete
                        ms[f, t][i].append((time.perf_counter() - t0) * 1e3)
                    same = same and out[False].tobytes() == out[True].tobytes()
                nodes[i] = scs[fams[-1]].last_stats["nodes"]
    r2 = lambda x: round(float(x), 2)
    per = {k: [float(np.median(v)) for v in ms[k]] for k in ms}   # per list, median over its repeats
    stat = lambda k: {"median": r2(np.median(per[k])), "min": r2(np.min(per[k])), "max": r2(np.max(per[k])),
                      "repeat_spread": r2(max(max(v) - min(v) for v in ms[k])), "per_list": [r2(x) for x in per[k]]}
    return lists, ntok, nodes, same, per, stat


def main_gemma2(a):
    """--arch gemma2: a Gemma2Scorer at the gemma-2-2b shape on random fp16 weights beside a LlamaScorer of equal active FLOPs
    per row (the same d, ffn, vocab and tied head; 18 query / 6 kv heads of 128, whose four projections have gemma-2-2b's
    2304 x 6144 weights), under the protocol of --arch olmo2."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, Hkv, hd, ffn, V, L = a.d, a.heads, a.kv_heads, 256, a.ffn, a.vocab, a.layers
    lH, lHkv, lhd, dev = 18, 6, 128, "cuda"
    if d != lH * lhd or (H + 2 * Hkv) * hd + H * hd != (lH + 2 * lHkv) * lhd + lH * lhd:
        raise SystemExit("--arch gemma2 compares at the gemma-2-2b widths only (d 2304, 8 query / 4 kv heads of 256)")
    rng = np.random.default_rng(0)
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).half()
    nw = lambda n, one: (one + 0.2 * torch.randn(n, device=dev)).half()
    emb = rn(V, d, std=2.0 / d ** 0.5)
    mlp = [{n: rn(o, i, std=1.0 / i ** 0.5) for n, (o, i) in {"mlp.gate_proj": (ffn, d), "mlp.up_proj": (ffn, d),
                                                               "mlp.down_proj": (d, ffn)}.items()} for _ in range(L)]

    def state(Hq, Hk, h, one, norms):
        st = {"model.embed_tokens.weight": emb, "model.norm.weight": nw(d, one)}
        for l in range(L):
            p = f"model.layers.{l}."
            for n, (o, i) in {"self_attn.q_proj": (Hq * h, d), "self_attn.k_proj": (Hk * h, d), "self_attn.v_proj": (Hk * h, d),
                              "self_attn.o_proj": (d, Hq * h)}.items():
                st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
            for n, w in mlp[l].items():
                st[p + n + ".weight"] = w
            for n in norms:
                st[p + n + ".weight"] = nw(d, one)
        return st
    base = dict(hidden_size=d, intermediate_size=ffn, vocab_size=V, num_hidden_layers=L, max_position_embeddings=8192,
                rms_norm_eps=1e-6, rope_theta=10000.0, tie_word_embeddings=True)
    cfg = dict(base, model_type="gemma2", num_attention_heads=H, num_key_value_heads=Hkv, head_dim=hd, sliding_window=4096,
               query_pre_attn_scalar=256, attn_logit_softcapping=50.0, final_logit_softcapping=30.0,
               hidden_activation="gelu_pytorch_tanh")
    dims = R.gemma2_dims(cfg, 2048)
    st = state(H, Hkv, hd, 0.0, ("input_layernorm", "post_attention_layernorm", "pre_feedforward_layernorm",
                                 "post_feedforward_layernorm"))
    scs = {"gemma2": R.Gemma2Scorer(dims, R.gemma2_device_layout(st, dims, R.rope_inv_freq(cfg)), dev)}
    lcfg = dict(base, model_type="llama", num_attention_heads=lH, num_key_value_heads=lHkv, hidden_act="silu")
    ldims = R.llama_dims(lcfg, 2048)
    st = state(lH, lHkv, lhd, 1.0, ("input_layernorm", "post_attention_layernorm"))
    scs["llama"] = R.LlamaScorer(ldims, R.llama_device_layout(st, ldims, R.rope_inv_freq(lcfg)), dev)
    del st, mlp, emb
    torch.cuda.empty_cache()
    lists, ntok, nodes, same, per, stat = alternate(a, rng, V, scs, ("llama", "gemma2"))
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["gemma2", t], per["llama", t])]
    print(json.dumps({"bench": "llm_rescore_gemma2", "layers": L, "d": d, "heads": H, "kv_heads": Hkv, "head_dim": hd, "ffn": ffn,
                      "vocab": V, "llama_heads": lH, "llama_kv_heads": lHkv, "cands": a.cands, "list": a.list,
                      "context": a.context, "lists": len(lists), "reps": max(1, a.reps), "tokens": float(np.mean(ntok)),
                      "nodes": float(np.mean(nodes)), "llama_flat_ms": stat(("llama", False)),
                      "gemma2_flat_ms": stat(("gemma2", False)), "llama_tree_ms": stat(("llama", True)),
                      "gemma2_tree_ms": stat(("gemma2", True)),
                      "ratio_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "ratio_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same)}))


def main_gptoss(a, n_experts=32, top_k=4):
    """--arch gptoss: a GptOssScorer at the gpt-oss-20b shape on random bf16 weights (sinks and biases N(0, 0.5)) beside a dense
    LlamaScorer of equal active matmul FLOPs per row, both in bf16, under the protocol of --arch gemma2.
    --experts mxfp4: the expert matrices are an MXFP4 checkpoint's (random nibbles, scale bytes 119 to 121: about the same spread of
    values) and a third scorer, the GptOssMxScorer that keeps them packed, alternates with the other two list by list; the line
    then also has its times, their ratio to the dense scorer's per list, whether its scores were the dense scorer's bytes, and the
    device bytes that either scorer's construction allocated."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, Hkv, hd, ffn, V, L = a.d, a.heads, a.kv_heads, 64, a.ffn, a.vocab, a.layers
    lH, lHkv, dev, bf = d // 64, 9, "cuda", torch.bfloat16
    lffn = top_k * ffn + ((H + 2 * Hkv) * hd + H * hd - (lH + 2 * lHkv) * 64 - d) // 3
    if d % 64 or lH % lHkv or lffn % 64 or 3 * (lffn - top_k * ffn) != (H + 2 * Hkv) * hd + H * hd - (lH + 2 * lHkv) * 64 - d:
        raise SystemExit("--arch gptoss compares at widths whose dense twin exists (d 2880, 64 / 8 heads of 64, ffn 2880)")
    rng = np.random.default_rng(0)
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).to(bf)
    nw = lambda n: (1 + 0.2 * torch.randn(n, device=dev)).to(bf)
    emb, head = rn(V, d, std=2.0 / d ** 0.5), rn(V, d, std=2.0 / d ** 0.5)
    base = dict(hidden_size=d, vocab_size=V, num_hidden_layers=L, max_position_embeddings=8192, rms_norm_eps=1e-5,
                tie_word_embeddings=False, hidden_act="silu")
    cfg = dict(base, model_type="gpt_oss", intermediate_size=ffn, num_attention_heads=H, num_key_value_heads=Hkv, head_dim=hd,
               num_local_experts=n_experts, num_experts_per_tok=top_k, sliding_window=128)
    st = {"model.embed_tokens.weight": emb, "lm_head.weight": head, "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        for n, (o, i) in {"q_proj": (H * hd, d), "k_proj": (Hkv * hd, d), "v_proj": (Hkv * hd, d), "o_proj": (d, H * hd)}.items():
            st[p + f"self_attn.{n}.weight"], st[p + f"self_attn.{n}.bias"] = rn(o, i, std=1.0 / i ** 0.5), rn(o, std=0.5)
        st[p + "self_attn.sinks"] = rn(H, std=0.5)
        st[p + "mlp.router.weight"], st[p + "mlp.router.bias"] = rn(n_experts, d, std=1.0 / d ** 0.5), rn(n_experts, std=0.5)
        st[p + "mlp.experts.gate_up_proj_bias"] = rn(n_experts, 2 * ffn, std=0.5)
        st[p + "mlp.experts.down_proj_bias"] = rn(n_experts, d, std=0.5)
        if a.experts == "mxfp4":
            for n, rows, K in (("gate_up_proj", 2 * ffn, d), ("down_proj", d, ffn)):
                st[p + f"mlp.experts.{n}_blocks"] = torch.randint(0, 256, (n_experts, rows, K // 32, 16), dtype=torch.uint8, device=dev)
                st[p + f"mlp.experts.{n}_scales"] = torch.randint(119, 122, (n_experts, rows, K // 32), dtype=torch.uint8, device=dev)
        else:
            st[p + "mlp.experts.gate_up_proj"] = rn(n_experts, d, 2 * ffn, std=1.0 / d ** 0.5)
            st[p + "mlp.experts.down_proj"] = rn(n_experts, ffn, d, std=1.0 / ffn ** 0.5)
        st[p + "input_layernorm.weight"], st[p + "post_attention_layernorm.weight"] = nw(d), nw(d)
    dims = R.gptoss_dims(cfg, 2048)
    def built(make):   # (the scorer, the device bytes its construction left allocated)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        sc = make()
        torch.cuda.synchronize()
        return sc, torch.cuda.memory_allocated() - before
    scs, held = {}, {}
    scs["gptoss"], held["gptoss"] = built(lambda: R.GptOssScorer(dims, R.gptoss_device_layout(st, dims, R.gptoss_rope(cfg), bf), dev, dtype=bf))
    fams = ("llama", "gptoss")
    if a.experts == "mxfp4":
        scs["gptoss_mx"], held["gptoss_mx"] = built(
            lambda: R.GptOssMxScorer(dims, R.gptoss_mx_device_layout(st, dims, R.gptoss_rope(cfg), bf), dev, dtype=bf))
        fams += ("gptoss_mx",)
    lst = {"model.embed_tokens.weight": emb, "lm_head.weight": head, "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        for n, (o, i) in {"self_attn.q_proj": (lH * 64, d), "self_attn.k_proj": (lHkv * 64, d), "self_attn.v_proj": (lHkv * 64, d),
                          "self_attn.o_proj": (d, d), "mlp.gate_proj": (lffn, d), "mlp.up_proj": (lffn, d), "mlp.down_proj": (d, lffn)}.items():
            lst[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
        lst[p + "input_layernorm.weight"], lst[p + "post_attention_layernorm.weight"] = nw(d), nw(d)
    lcfg = dict(base, model_type="llama", intermediate_size=lffn, num_attention_heads=lH, num_key_value_heads=lHkv, rope_theta=10000.0)
    ldims = R.llama_dims(lcfg, 2048)
    scs["llama"] = R.LlamaScorer(ldims, R.llama_device_layout(lst, ldims, R.rope_inv_freq(lcfg), bf), dev, dtype=bf)
    del st, lst, emb, head
    torch.cuda.empty_cache()
    lists, ntok, nodes, same, per, stat = alternate(a, rng, V, scs, fams)
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["gptoss", t], per["llama", t])]
    mx = {}
    if a.experts == "mxfp4":
        mx_ratio = lambda t: [round(o / l, 4) for o, l in zip(per["gptoss_mx", t], per["gptoss", t])]
        with torch.inference_mode():
            equal = all(scs["gptoss_mx"].score(l, share_prefixes=t).tobytes() == scs["gptoss"].score(l, share_prefixes=t).tobytes()
                        for l in lists for t in (False, True))
        mx = {"experts": "mxfp4", "gptoss_mx_flat_ms": stat(("gptoss_mx", False)), "gptoss_mx_tree_ms": stat(("gptoss_mx", True)),
              "mx_over_dense_flat": {"median": round(float(np.median(mx_ratio(False))), 4), "per_list": mx_ratio(False)},
              "mx_over_dense_tree": {"median": round(float(np.median(mx_ratio(True))), 4), "per_list": mx_ratio(True)},
              "mx_scores_are_dense_bytes": bool(equal), "dense_device_bytes": held["gptoss"], "mx_device_bytes": held["gptoss_mx"],
              "mx_expert_bytes": scs["gptoss_mx"].expert_bytes()}
    S = lambda rows: -(-rows * top_k // 256) * 256 + 256 * n_experts
    print(json.dumps({"bench": "llm_rescore_gptoss", "dtype": "bfloat16", "layers": L, "d": d, "heads": H, "kv_heads": Hkv, "head_dim": hd,
                      "ffn": ffn, "experts": n_experts, "top_k": top_k, "vocab": V, "llama_heads": lH, "llama_kv_heads": lHkv,
                      "llama_ffn": lffn, "cands": a.cands, "list": a.list, "context": a.context, "lists": len(lists),
                      "reps": max(1, a.reps), "tokens": float(np.mean(ntok)), "nodes": float(np.mean(nodes)),
                      "sorted_rows_flat": float(np.mean([S(n) for n in ntok])), "routed_rows_flat": float(np.mean(ntok)) * top_k,
                      "sorted_rows_tree": float(np.mean([S(n) for n in nodes])), "routed_rows_tree": float(np.mean(nodes)) * top_k,
                      "llama_flat_ms": stat(("llama", False)), "gptoss_flat_ms": stat(("gptoss", False)),
                      "llama_tree_ms": stat(("llama", True)), "gptoss_tree_ms": stat(("gptoss", True)),
                      "ratio_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "ratio_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same), **mx}))


def main_phi3(a):
    """--arch phi3: a Phi3Scorer at the Phi-3-mini shape (heads of 96, the fused qkv_proj / gate_up_proj) on random fp16 weights
    beside a LlamaScorer of equal FLOPs per row (the same weights read as d / 128 heads of 128, rotated in the QKV GEMM's
    epilogue), under the protocol of --arch gemma2."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, Hkv, ffn, V, L = a.d, a.heads, a.kv_heads, a.ffn, a.vocab, a.layers
    hd, lhd, dev = d // H, 128, "cuda"
    if hd != 96 or d % lhd or (Hkv * hd) % lhd:
        raise SystemExit("--arch phi3 compares heads of 96 with heads of 128 over the same widths (d 3072, 32 / 32 heads)")
    lH, lHkv = d // lhd, Hkv * hd // lhd
    rng = np.random.default_rng(0)
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).half()
    nw = lambda n: (1 + 0.2 * torch.randn(n, device=dev)).half()
    st = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "lm_head.weight": rn(V, d, std=2.0 / d ** 0.5),
          "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        for n, (o, i) in {"self_attn.qkv_proj": ((H + 2 * Hkv) * hd, d), "self_attn.o_proj": (d, d), "mlp.gate_up_proj": (2 * ffn, d),
                          "mlp.down_proj": (d, ffn)}.items():
            st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
        st[p + "input_layernorm.weight"], st[p + "post_attention_layernorm.weight"] = nw(d), nw(d)
    base = dict(hidden_size=d, intermediate_size=ffn, vocab_size=V, num_hidden_layers=L, max_position_embeddings=4096,
                rms_norm_eps=1e-5, rope_theta=10000.0, tie_word_embeddings=False, hidden_act="silu")
    cfg = dict(base, model_type="phi3", num_attention_heads=H, num_key_value_heads=Hkv, sliding_window=2047)
    dims = R.phi3_dims(cfg)
    scs = {"phi3": R.Phi3Scorer(dims, R.phi3_device_layout(st, dims, R.phi3_rope(cfg)), dev)}
    lst = {}
    for k, v in st.items():      # the fused tensors split at the same rows
        if "qkv_proj" in k:
            for n, t in zip(("q_proj", "k_proj", "v_proj"), v.split((H * hd, Hkv * hd, Hkv * hd))):
                lst[k.replace("qkv_proj", n)] = t
        elif "gate_up_proj" in k:
            lst[k.replace("gate_up_proj", "gate_proj")], lst[k.replace("gate_up_proj", "up_proj")] = v[:ffn], v[ffn:]
        else:
            lst[k] = v
    lcfg = dict(base, model_type="llama", num_attention_heads=lH, num_key_value_heads=lHkv)
    ldims = R.llama_dims(lcfg, dims["max_pos"])
    scs["llama"] = R.LlamaScorer(ldims, R.llama_device_layout(lst, ldims, R.rope_inv_freq(lcfg)), dev)
    del st, lst
    torch.cuda.empty_cache()
    lists, ntok, nodes, same, per, stat = alternate(a, rng, V, scs, ("llama", "phi3"))
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["phi3", t], per["llama", t])]
    print(json.dumps({"bench": "llm_rescore_phi3", "layers": L, "d": d, "heads": H, "kv_heads": Hkv, "head_dim": hd, "ffn": ffn,
                      "vocab": V, "llama_heads": lH, "llama_kv_heads": lHkv, "cands": a.cands, "list": a.list,
                      "context": a.context, "lists": len(lists), "reps": max(1, a.reps), "tokens": float(np.mean(ntok)),
                      "nodes": float(np.mean(nodes)), "llama_flat_ms": stat(("llama", False)),
                      "phi3_flat_ms": stat(("phi3", False)), "llama_tree_ms": stat(("llama", True)),
                      "phi3_tree_ms": stat(("phi3", True)),
                      "ratio_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "ratio_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same)}))


def main_olmo2(a):
    """--arch olmo2: an Olmo2Scorer and a LlamaScorer of the same dimensions on the same random fp16 weights (the Llama model
    takes post_feedforward_layernorm as its input norm and drops the q / k norms), flat and tree of both alternating list by
    list in this process."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, Hkv, ffn, V, L = a.d, a.heads, a.kv_heads, a.ffn, a.vocab, a.layers
    hd, dev = d // H, "cuda"
    rng = np.random.default_rng(0)
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).half()
    nw = lambda n: (1 + 0.2 * torch.randn(n, device=dev)).half()
    st = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "lm_head.weight": rn(V, d, std=2.0 / d ** 0.5),
          "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        for n, (o, i) in {"self_attn.q_proj": (H * hd, d), "self_attn.k_proj": (Hkv * hd, d), "self_attn.v_proj": (Hkv * hd, d),
                          "self_attn.o_proj": (d, d), "mlp.gate_proj": (ffn, d), "mlp.up_proj": (ffn, d),
                          "mlp.down_proj": (d, ffn)}.items():
            st[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
        st[p + "self_attn.q_norm.weight"], st[p + "self_attn.k_norm.weight"] = nw(H * hd), nw(Hkv * hd)
        st[p + "post_attention_layernorm.weight"], st[p + "post_feedforward_layernorm.weight"] = nw(d), nw(d)
    cfg = dict(model_type="olmo2", hidden_size=d, num_attention_heads=H, num_key_value_heads=Hkv, intermediate_size=ffn,
               vocab_size=V, num_hidden_layers=L, max_position_embeddings=2048, rms_norm_eps=1e-6, rope_theta=500000.0,
               tie_word_embeddings=False, hidden_act="silu")
    dims = R.olmo2_dims(cfg)
    scs = {"olmo2": R.Olmo2Scorer(dims, R.olmo2_device_layout(st, dims, R.rope_inv_freq(cfg)), dev)}
    lst = {k.replace("post_feedforward_layernorm", "input_layernorm"): v for k, v in st.items() if "_norm.weight" not in k}
    lcfg = dict(cfg, model_type="llama")
    ldims = R.llama_dims(lcfg)
    scs["llama"] = R.LlamaScorer(ldims, R.llama_device_layout(lst, ldims, R.rope_inv_freq(lcfg)), dev)
    del st, lst
    torch.cuda.empty_cache()
    lists, ntok, nodes, same, per, stat = alternate(a, rng, V, scs, ("llama", "olmo2"))
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["olmo2", t], per["llama", t])]
    print(json.dumps({"bench": "llm_rescore_olmo2", "layers": L, "d": d, "heads": H, "kv_heads": Hkv, "ffn": ffn, "vocab": V,
                      "cands": a.cands, "list": a.list, "context": a.context, "lists": len(lists), "reps": max(1, a.reps),
                      "tokens": float(np.mean(ntok)), "nodes": float(np.mean(nodes)), "per_list_tokens": ntok,
                      "per_list_nodes": nodes, "llama_flat_ms": stat(("llama", False)), "olmo2_flat_ms": stat(("olmo2", False)),
                      "llama_tree_ms": stat(("llama", True)), "olmo2_tree_ms": stat(("olmo2", True)),
                      "ratio_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "ratio_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same)}))


def main_mixtral(a, n_experts=8, top_k=2):
    """--arch mixtral: a MixtralScorer and a dense LlamaScorer with ffn top_k x the experts' (the same active FLOPs per row) on
    random fp16 weights that share everything but the MLP, flat and tree of both alternating list by list in this process."""
    import torch
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, Hkv, ffn, V, L = a.d, a.heads, a.kv_heads, a.ffn, a.vocab, a.layers
    hd, dev = d // H, "cuda"
    rng = np.random.default_rng(0)
    rn = lambda *s, std: (torch.randn(*s, device=dev) * std).half()
    nw = lambda n: (1 + 0.2 * torch.randn(n, device=dev)).half()
    base = dict(hidden_size=d, num_attention_heads=H, num_key_value_heads=Hkv, vocab_size=V, num_hidden_layers=L,
                max_position_embeddings=2048, rms_norm_eps=1e-5, rope_theta=1e6, tie_word_embeddings=False, hidden_act="silu")
    cfg = dict(base, model_type="mixtral", intermediate_size=ffn, num_local_experts=n_experts, num_experts_per_tok=top_k)
    lcfg = dict(base, model_type="llama", intermediate_size=top_k * ffn)
    dims, ldims = R.mixtral_dims(cfg), R.llama_dims(lcfg)
    shared = {"model.embed_tokens.weight": rn(V, d, std=2.0 / d ** 0.5), "lm_head.weight": rn(V, d, std=2.0 / d ** 0.5),
              "model.norm.weight": nw(d)}
    for l in range(L):
        p = f"model.layers.{l}."
        for n, (o, i) in {"self_attn.q_proj": (H * hd, d), "self_attn.k_proj": (Hkv * hd, d), "self_attn.v_proj": (Hkv * hd, d),
                          "self_attn.o_proj": (d, d)}.items():
            shared[p + n + ".weight"] = rn(o, i, std=1.0 / i ** 0.5)
        shared[p + "input_layernorm.weight"], shared[p + "post_attention_layernorm.weight"] = nw(d), nw(d)
    st = dict(shared)
    for l in range(L):
        p = f"model.layers.{l}.mlp."
        st[p + "gate.weight"] = rn(n_experts, d, std=1.0 / d ** 0.5)
        st[p + "experts.gate_up_proj"] = rn(n_experts, 2 * ffn, d, std=1.0 / d ** 0.5)
        st[p + "experts.down_proj"] = rn(n_experts, d, ffn, std=1.0 / ffn ** 0.5)
    scs = {"mixtral": R.MixtralScorer(dims, R.mixtral_device_layout(st, dims, R.rope_inv_freq(cfg)), dev)}
    del st
    st = dict(shared)
    for l in range(L):
        p = f"model.layers.{l}.mlp."
        st[p + "gate_proj.weight"], st[p + "up_proj.weight"] = (rn(top_k * ffn, d, std=1.0 / d ** 0.5) for _ in range(2))
        st[p + "down_proj.weight"] = rn(d, top_k * ffn, std=1.0 / (top_k * ffn) ** 0.5)
    scs["llama"] = R.LlamaScorer(ldims, R.llama_device_layout(st, ldims, R.rope_inv_freq(lcfg)), dev)
    del st, shared
    torch.cuda.empty_cache()
    gen = nbest_list if a.list == "nbest" else random_list
    lists = [gen(rng, V, a.cands, [int(x) for x in rng.integers(4, V, a.context)]) for _ in range(a.lists)]
    ntok = [sum(len(s) for s in l) for l in lists]
    fams, paths = ("llama", "mixtral"), (False, True)
    ms = {(f, t): [[] for _ in lists] for f in fams for t in paths}
    nodes, same = [0] * len(lists), True
    with torch.inference_mode():
        for i in range(max(1, a.warmup)):
            for f in fams:
                for t in paths:
                    scs[f].score(lists[i % len(lists)], share_prefixes=t)
        torch.cuda.synchronize()
        for _ in range(max(1, a.reps)):
            for i, l in enumerate(lists):
                for f in fams:
                    out = {}
                    for t in paths:
                        t0 = time.perf_counter()
                        out[t] = scs[f].score(l, share_prefixes=t)   # returns host scores: the call is complete
                        ms[f, t][i].append((time.perf_counter() - t0) * 1e3)
                    same = same and out[False].tobytes() == out[True].tobytes()
                nodes[i] = scs["mixtral"].last_stats["nodes"]
    r2 = lambda x: round(float(x), 2)
    per = {k: [float(np.median(v)) for v in ms[k]] for k in ms}   # per list, median over its repeats
    stat = lambda k: {"median": r2(np.median(per[k])), "min": r2(np.min(per[k])), "max": r2(np.max(per[k])),
                      "repeat_spread": r2(max(max(v) - min(v) for v in ms[k])), "per_list": [r2(x) for x in per[k]]}
    ratio = lambda t: [round(o / l, 4) for o, l in zip(per["mixtral", t], per["llama", t])]
    sorted_rows = lambda rows: -(-rows * top_k // 256) * 256 + 256 * n_experts
    print(json.dumps({"bench": "llm_rescore_mixtral", "layers": L, "d": d, "heads": H, "kv_heads": Hkv, "ffn": ffn, "vocab": V,
                      "n_experts": n_experts, "top_k": top_k, "dense_ffn": top_k * ffn, "cands": a.cands, "list": a.list,
                      "context": a.context, "lists": len(lists), "reps": max(1, a.reps), "tokens": float(np.mean(ntok)),
                      "nodes": float(np.mean(nodes)), "per_list_tokens": ntok, "per_list_nodes": nodes,
                      "sorted_rows_over_routed_flat": [round(sorted_rows(n) / (n * top_k), 3) for n in ntok],
                      "sorted_rows_over_routed_tree": [round(sorted_rows(n) / (n * top_k), 3) for n in nodes],
                      "llama_flat_ms": stat(("llama", False)), "mixtral_flat_ms": stat(("mixtral", False)),
                      "llama_tree_ms": stat(("llama", True)), "mixtral_tree_ms": stat(("mixtral", True)),
                      "ratio_flat": {"median": round(float(np.median(ratio(False))), 4), "per_list": ratio(False)},
                      "ratio_tree": {"median": round(float(np.median(ratio(True))), 4), "per_list": ratio(True)},
                      "flat_tree_bit_identical": bool(same)}))


def against_hf(a, sc, model, calls, rng, flop_tok, extra):
    """What --arch llama / qwen3 / gpt2 run behind their scorer and HF model: --session, the flat / tree A/B, or the HIP path
    against the HF model on the same lists; `extra` are the family's own fields of the last row."""
    import torch
    dev, V, d, H, ffn, L = "cuda", a.vocab, a.d, a.heads, a.ffn, a.layers
    if a.session:
        del model
        torch.cuda.empty_cache()
        return session(a, sc, *calls, arch=a.arch)
    ab = a.tree or a.list != "random" or a.context > 0
    if not ab:
        lists = [random_list(rng, V, a.cands) for _ in range(a.lists)]
    else:
        gen = nbest_list if a.list == "nbest" else random_list
        lists = [gen(rng, V, a.cands, [int(x) for x in rng.integers(4, V, a.context)]) for _ in range(a.lists)]
    ntok = [sum(len(s) for s in l) for l in lists]
    if ab:
        del model
        torch.cuda.empty_cache()
        return ab_flat_tree(a, sc, lists, ntok, arch=a.arch)

    def torch_score(seqs):   # padded batch through the HF model, in --dtype
        B, T = len(seqs), max(len(s) for s in seqs)
        ids = torch.zeros(B, T, dtype=torch.long, device=dev)
        mask = torch.zeros(B, T, dtype=torch.long, device=dev)
        for i, s in enumerate(seqs):
            ids[i, :len(s)] = torch.as_tensor(s, device=dev); mask[i, :len(s)] = 1
        lp = torch.log_softmax(model(input_ids=ids, attention_mask=mask).logits.float(), -1)
        g = lp[:, :-1].gather(-1, ids[:, 1:, None])[..., 0] * mask[:, 1:]
        return g.sum(1).cpu().numpy()

    def timed(fn):   # per list, so that the medians and the spread can be reported
        for i in range(a.warmup):
            fn(lists[i % len(lists)])
        torch.cuda.synchronize()
        ms, outs = [], []
        for l in lists:
            t0 = time.perf_counter()
            outs.append(fn(l))   # returns host scores: the call is complete
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms, outs

    with torch.inference_mode():
        ms_hip, s_hip = timed(lambda l: sc.score(l))
        ms_torch, s_torch = timed(torch_score)
        ms_hip2, _ = timed(lambda l: sc.score(l))      # once more after the torch pass: the order does not decide
    diff = max(float(np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).max()) for x, y in zip(s_hip, s_torch))
    r2 = lambda x: round(float(x), 2)
    mh, mt = float(np.mean(ms_hip)), float(np.mean(ms_torch))
    print(json.dumps({"bench": "llm_rescore", "arch": a.arch, "dtype": a.dtype, "layers": L, "d": d, "heads": H, **extra, "ffn": ffn,
                      "vocab": V, "cands": a.cands, "tokens_per_list": float(np.mean(ntok)), "hip_ms_per_list": r2(mh),
                      "torch_fp16_ms_per_list": r2(mt), "hip_tflops": round(np.mean(ntok) * flop_tok / (mh * 1e-3) / 1e12, 1),
                      "speedup_vs_torch": round(mt / mh, 3), "max_abs_score_diff_vs_torch": round(diff, 4),
                      "hip_ms": {"median": r2(np.median(ms_hip)), "min": r2(min(ms_hip)), "max": r2(max(ms_hip))},
                      "hip_ms_second_pass": {"median": r2(np.median(ms_hip2)), "min": r2(min(ms_hip2)), "max": r2(max(ms_hip2))},
                      "torch_ms": {"median": r2(np.median(ms_torch)), "min": r2(min(ms_torch)), "max": r2(max(ms_torch))},
                      "per_list_tokens": ntok, "per_list_hip_ms": [r2(x) for x in ms_hip],
                      "per_list_torch_ms": [r2(x) for x in ms_torch]}))


def ab_flat_tree(a, sc, lists, ntok, arch="opt"):
    """Flat and tree path on the same lists in this process, alternating list by list, --reps passes over the lists; both
    warmed up first.  Lists differ in size, so the run-to-run spread is taken per list: the largest max - min over the
    repeats of one list."""
    import torch
    ms = {False: [[] for _ in lists], True: [[] for _ in lists]}
    nodes, same = [0] * len(lists), True
    with torch.inference_mode():
        for i in range(max(1, a.warmup)):
            for tree in (False, True):
                sc.score(lists[i % len(lists)], share_prefixes=tree)
        torch.cuda.synchronize()
        for _ in range(max(1, a.reps)):
            for i, l in enumerate(lists):
                out = {}
                for tree in (False, True):
                    t0 = time.perf_counter()
                    out[tree] = sc.score(l, share_prefixes=tree)   # returns host scores: the call is complete
                    ms[tree][i].append((time.perf_counter() - t0) * 1e3)
                nodes[i] = sc.last_stats["nodes"]
                same = same and out[False].tobytes() == out[True].tobytes()
    r2 = lambda x: round(float(x), 2)
    per = {t: [float(np.median(v)) for v in ms[t]] for t in ms}   # per list, median over its repeats
    st = lambda t: {"median": r2(np.median(per[t])), "min": r2(np.min(per[t])), "max": r2(np.max(per[t])),
                    "repeat_spread": r2(max(max(v) - min(v) for v in ms[t]))}
    print(json.dumps({"bench": "llm_rescore_tree", "arch": arch, "layers": a.layers, "d": a.d, "heads": a.heads, "ffn": a.ffn, "vocab": a.vocab,
                      "cands": a.cands, "list": a.list, "context": a.context, "lists": len(lists), "reps": max(1, a.reps),
                      "tokens": float(np.mean(ntok)), "nodes": float(np.mean(nodes)),
                      "hip_ms_per_list": st(False)["median"], "hip_tree_ms_per_list": st(True)["median"],
                      "flat_ms": st(False), "tree_ms": st(True), "per_list_tokens": ntok, "per_list_nodes": nodes,
                      "per_list_flat_ms": [r2(x) for x in per[False]], "per_list_tree_ms": [r2(x) for x in per[True]],
                      "scores_bit_identical": bool(same)}))


def session_calls(a, rng, max_pos):
    """(the lists of the conversation, the context length of each); exits when the conversation outgrows max_pos."""
    calls, ctx_len, ctx = [], [], []
    for _ in range(a.sentences):
        calls.append(nbest_list(rng, a.vocab, a.cands, ctx))
        ctx_len.append(len(ctx))
        ctx = [int(x) for x in calls[-1][0][1:]]   # the context so far + the base sentence of this call
    if len(ctx) + 1 > max_pos:
        raise SystemExit(f"--sentences {a.sentences}: the conversation outgrows max_pos {max_pos}")
    return calls, ctx_len


def session(a, sc, calls, ctx_len, arch="opt"):
    """Tree path against the cached path (stage A, stage A + B) call by call over one conversation; see the module docstring."""
    import torch
    ENV = "B2T_CLM_TRUNK_ATTN"
    paths = ("tree", "cached_a", "cached_ab")
    ms = {p: [[] for _ in calls] for p in paths}
    info, same = [None] * len(calls), True
    old = os.environ.get(ENV)
    try:
        with torch.inference_mode():
            for rep in range(max(1, a.reps) + 1):   # pass 0 warms every path and is not timed
                sc.cache_reset()
                for k, l in enumerate(calls):
                    held, out = sc.cache_len, {}
                    for p in paths:
                        if p != "tree":
                            os.environ[ENV] = "0" if p == "cached_a" else "1"
                            sc.cache_reset(keep=held)
                        t0 = time.perf_counter()
                        out[p] = sc.score(l, share_prefixes=True, use_cache=p != "tree")   # host scores: the call is complete
                        if rep:
                            ms[p][k].append((time.perf_counter() - t0) * 1e3)
                        if p == "tree":
                            nodes = sc.last_stats["nodes"]
                    same = same and out["tree"].tobytes() == out["cached_a"].tobytes() == out["cached_ab"].tobytes()
                    info[k] = {"context": ctx_len[k], "tokens": sum(map(len, l)), "nodes": nodes, "rows": sc.last_stats["nodes"],
                               "reused": sc.last_stats["reused"]}
    finally:
        if old is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = old
    r2 = lambda x: round(float(x), 2)
    for k in range(len(calls)):
        for p in paths:
            info[k][p + "_ms"] = r2(np.median(ms[p][k]))
            info[k][p + "_spread"] = r2(max(ms[p][k]) - min(ms[p][k]))
    print(json.dumps({"bench": "llm_rescore_session", "arch": arch, "layers": a.layers, "d": a.d, "heads": a.heads, "ffn": a.ffn, "vocab": a.vocab,
                      "cands": a.cands, "sentences": len(calls), "reps": max(1, a.reps), "per_call": info,
                      "scores_bit_identical": bool(same)}))


if __name__ == "__main__":
    main()
