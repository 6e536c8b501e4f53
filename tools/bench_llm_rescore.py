#!/usr/bin/env python3
"""OPT n-best rescoring throughput: b2t_clm_score_f16 against a plain-torch fp16 restatement of the same forward (F.linear on
hipBLASLt, SDPA) on the same weights.  OPT-6.7b shape (32 layers, d 4096, 32 x 128 heads, ffn 16384, vocab 50272) with random
fp16 weights (~13.3 GB); one "list" = 100 candidates of 10-40 tokens.  Prints one JSON line.

  python tools/bench_llm_rescore.py [--layers 32] [--lists 5] [--warmup 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nejm-brain-to-text_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--d", type=int, default=4096)
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--ffn", type=int, default=16384)
    ap.add_argument("--vocab", type=int, default=50272)
    ap.add_argument("--cands", type=int, default=100)
    ap.add_argument("--lists", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import llm_rescore as R
    torch.manual_seed(0)
    d, H, ffn, V, L = a.d, a.heads, a.ffn, a.vocab, a.layers
    hd = d // H
    dims = dict(n_layers=L, d_model=d, n_heads=H, ffn_dim=ffn, vocab=V, max_pos=2048)
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
    sc = R.OptScorer(dims, lay, dev)
    del lay
    rng = np.random.default_rng(0)
    lists = [[[2] + list(rng.integers(4, V, int(n) - 1)) for n in rng.integers(10, 41, a.cands)] for _ in range(a.lists)]
    ntok = [sum(len(s) for s in l) for l in lists]

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


if __name__ == "__main__":
    main()
