"""LLM n-best rescoring (OPT, GPT-2, and the Llama family: Llama, Mistral, Qwen2, Qwen3): the LLM stage of language_model/language-model-standalone.py (build_opt :92-124, rescore_with_gpt2
:127-162, gpt2_lm_decode :165-251, get_string_differences :273-311, augment_nbest :327-411) with the causal-LM forward on the
HIP path (b2t_clm_score_f16, csrc/causal_lm.hip; opt-in b2t_clm_score_tree_f16, csrc/causal_lm_tree.hip, which computes the
prefixes the candidates share once; opt-in b2t_clm_score_tree_cached_f16, csrc/causal_lm_cache.hip, which also keeps the
decoding context's keys, values and log-probs from one call to the next; the Llama family has the same three paths).

Call surfaces are the reference's: `build_opt(model_name, cache_dir, device)` returns `(model, tokenizer)`, and the three
functions take them as the reference's do.  `model` here is an `OptScorer`: the checkpoint's fp16 weights converted once into
the device layout of include/b2t.h, scored on packed variable-length token ids (no padding).  Tokenisation stays on the host.
`build_opt` never reaches the network: it reads a local directory (the model name itself, or the hub-cache layout under
`cache_dir`) and refuses what the kernels do not run (post-LN OPT, opt-350m's projection layers, non-ReLU activations).

`build_opt` dispatches on config.json's model_type, as the reference's AutoModelForCausalLM does: "opt" gives an OptScorer;
"llama", "mistral" and "qwen2" give a `LlamaScorer` (b2t_clm_llama_score_f16 / b2t_clm_llama_score_tree_f16 /
b2t_clm_llama_score_tree_cached_f16, csrc/causal_lm_llama.hip: RMSNorm, rotary positions, grouped-query attention, SwiGLU) with
the same `score` / `token_logprobs` surface and the same opt-in context cache, so the three functions and
remote_lm.LocalLMService take either.

The Llama family also computes in bfloat16, the format its checkpoints are published in: `dtype="bfloat16"` (or `"auto"`, which
follows config.json's torch_dtype) on `build_opt` / `build_scorer` / `LlamaScorer` keeps the weights in bf16 and scores
through b2t_clm_llama_score_bf16 / b2t_clm_llama_score_tree_bf16 (csrc/causal_lm_llama_bf16.hip), on the flat and tree paths.
The default stays fp16; OPT is fp16 only.

"qwen3" gives a `LlamaScorer` too: Qwen3 is the same forward with an RMSNorm over every q and k head between the projection
and the rotation, which runs in the QKV GEMM's epilogue (b2t_clm_qwen3_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 /
_tree_bf16, csrc/causal_lm_qwen3.hip).  The loader adds the norm weights to the layout and the scorer takes those entry points
when its arrays hold them.  Checkpoints whose head_dim is not hidden_size / heads (Qwen3-0.6B, 4B, 32B) are refused.

"gpt2" (distilgpt2, gpt2, -medium, -large, -xl) gives a `Gpt2Scorer`, an OptScorer on the entry points b2t_clm_gpt2_score_f16 /
_tree_f16 / _tree_cached_f16 (csrc/causal_lm_gpt2.hip): behind the loader (Conv1D weights transposed, c_attn split into q | k | v
rows, wpe behind two zero rows) GPT-2 is the OPT forward with gelu_new in the fc1 GEMM's epilogue where OPT has ReLU.  fp16
only.  The GPT-2 tokenizer prepends no BOS, so a candidate's first token is unscored, as in the reference.

"gpt_neox" with head dim 64 or 128 (pythia-70m, 160m, 410m, 1.4b, 6.9b, 12b) gives a `NeoxScorer` on b2t_clm_neox_score_f16 / _tree_f16 / _tree_cached_f16
(csrc/causal_lm_neox.hip): OPT's LayerNorm, biased projections and attention with rotary positions on the first rotary_pct of
every head (in the QKV GEMM's epilogue, on rows the loader de-interleaves and permutes: neox_device_layout), the erf GELU (or
the tanh form, by hidden_act) in the fc1 GEMM's, and the parallel residual.  fp16 only; head dims 64 and 128 (not pythia-1b's
256, pythia-2.8b's 80 or gpt-neox-20b's 96), parallel residual, biased attention, eps 1e-5 and default rope only.
"""
from __future__ import annotations

import glob
import json
import logging
import os
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

ROWPAD = 256   # weight rows are padded to this multiple (b2t_clm_t layout)
HEAD_DIMS = (64, 80, 128)

_LAYER_FIELDS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "out_w", "out_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")


# ---- n-best arithmetic of the reference (pure host code) ---------------------------------------------------------------
def get_string_differences(cue: str, decoder_output: str):
    """Word-level edit distance from decoder_output to cue with its backtrace: (cost, path, spans).  path holds, per word of
    decoder_output in order, its index when it matches or 'R' / 'D', with 'I' for words of cue that are inserted; 'I' entries
    are then dropped.  spans are the (start, end) character ranges of decoder_output's replaced or deleted words.  Ties are
    broken insertion first, then deletion, then substitution, as in the reference."""
    out_w, cue_w = decoder_output.split(), cue.split()
    n, m = len(out_w), len(cue_w)
    # cost[i][j]: distance between the first i words of decoder_output and the first j words of cue
    cost = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0:
                cost[i][j] = j
            elif j == 0:
                cost[i][j] = i
            elif out_w[i - 1] == cue_w[j - 1]:
                cost[i][j] = cost[i - 1][j - 1]
            else:
                cost[i][j] = 1 + min(cost[i][j - 1], cost[i - 1][j], cost[i - 1][j - 1])
    rev = []
    i, j = n, m
    while i > 0 and j > 0:
        if out_w[i - 1] == cue_w[j - 1]:
            rev.append(i - 1); i -= 1; j -= 1
            continue
        ins, dele, sub = cost[i][j - 1], cost[i - 1][j], cost[i - 1][j - 1]
        if ins <= dele and ins <= sub:
            rev.append("I"); j -= 1
        elif dele <= ins and dele <= sub:
            rev.append("D"); i -= 1
        else:
            rev.append("R"); i -= 1; j -= 1
    rev.extend(["D"] * i)
    rev.extend(["I"] * j)
    path = [p for p in reversed(rev) if p != "I"]
    spans, pos = [], 0
    for label, word in zip(path, out_w):
        if label in ("R", "D"):
            spans.append((pos, pos + len(word)))
        pos += len(word) + 1
    return cost[n][m], path, spans


def _sorted_desc(total: Sequence[float]) -> np.ndarray:
    return np.argsort(total)[::-1]


def augment_nbest(nbest, top_candidates_to_augment=20, acoustic_scale=0.3, score_penalty_percent=0.01):
    """Grow an n-best list of [sentence, ac, lm] by exchanging substituted words between pairs of the top candidates of equal
    word count.  A new sentence gets the pair's mean scores, each lowered by score_penalty_percent of its magnitude; the result
    is sorted by acoustic_scale * ac + lm, best first."""
    sent = [e[0].strip() for e in nbest]
    ac = [e[1] for e in nbest]
    lm = [e[2] for e in nbest]
    tot = [acoustic_scale * a + b for a, b in zip(ac, lm)]
    order = _sorted_desc(tot)
    sent, ac, lm, tot = ([x[i] for i in order] for x in (sent, ac, lm, tot))

    new_s, new_ac, new_lm, new_tot = [], [], [], []
    top = top_candidates_to_augment
    for a in range(min(len(sent) - 1, top)):
        wa = sent[a].split()
        for b in range(a + 1, min(len(sent), top)):
            wb = sent[b].split()
            if len(wa) != len(wb):
                continue
            _, path_ab, _ = get_string_differences(sent[a], sent[b])
            _, path_ba, _ = get_string_differences(sent[b], sent[a])
            ra = [k for k, p in enumerate(path_ba) if p == "R"]
            rb = [k for k, p in enumerate(path_ab) if p == "R"]
            mac, mlm = np.mean([ac[a], ac[b]]), np.mean([lm[a], lm[b]])
            for ia, ib in zip(ra, rb):
                xa, xb = list(wa), list(wb)
                xa[ia], xb[ib] = wb[ib], wa[ia]
                for cand in (" ".join(xa), " ".join(xb)):
                    if cand in sent or cand in new_s:
                        continue
                    new_s.append(cand)
                    new_ac.append(mac - score_penalty_percent * np.abs(mac))
                    new_lm.append(mlm - score_penalty_percent * np.abs(mlm))
                    new_tot.append(acoustic_scale * new_ac[-1] + new_lm[-1])
    sent += new_s; ac += new_ac; lm += new_lm; tot += new_tot
    order = _sorted_desc(tot)
    return [[sent[i], ac[i], lm[i]] for i in order]


# ---- scoring ------------------------------------------------------------------------------------------------------------
def rescore_with_gpt2(model, tokenizer, device, hypotheses, length_penalty):
    """LLM score of every hypothesis: sum over t >= 1 of log p(token t | tokens < t) - n_tokens * length_penalty, n_tokens
    counting the tokenizer's BOS.  `model` is an OptScorer (or any object with its `score`); `device` is kept for the
    reference's signature (the scorer's weights say where it runs)."""
    enc = tokenizer(list(hypotheses))
    ids = []
    for row, mask in zip(enc["input_ids"], enc["attention_mask"]):
        row, mask = np.asarray(row), np.asarray(mask)
        ids.append(row[mask != 0].astype(np.int32))
    return list(model.score(ids, length_penalty))


def _normalise(hyp: str) -> str:
    for a, b in ((">", ""), ("  ", " "), (" ,", ","), (" .", "."), (" ?", "?")):
        hyp = hyp.replace(a, b)
    return hyp


def gpt2_lm_decode(model, tokenizer, device, nbest, acoustic_scale, length_penalty, alpha, returnConfidence=False,
                   current_context_str=None):
    """Pick the best of an n-best list [sentence, ac, lm, ...] by acoustic_scale * ac + (1 - alpha) * lm + alpha * llm.
    Returns (best, nbest_out) or (best, nbest_out, confidence); nbest_out entries are 'sentence;ac;lm;llm;total'.  Empty
    hypotheses are skipped, and -- as in the reference -- nbest_out still pairs nbest[i] with the i-th kept hypothesis' scores."""
    ctx = current_context_str if current_context_str is not None and len(current_context_str.split()) > 0 else None
    hyps, ac, old_lm = [], [], []
    for e in nbest:
        h = e[0].strip()
        if not h:
            continue
        if ctx is not None:
            h = ctx + " " + h
        hyps.append(_normalise(h))
        ac.append(e[1])
        old_lm.append(e[2])
    if not hyps:
        logging.error("gpt2_lm_decode: no hypotheses")
        return ("", [], 0.0) if returnConfidence else ("", [])
    ac, old_lm = np.array(ac), np.array(old_lm)
    try:
        new_lm = np.array(rescore_with_gpt2(model, tokenizer, device, hyps, length_penalty))
    except Exception as e:   # the reference retries in five slices, then gives up with zeros
        logging.error(f"OPT rescore failed: {e}")
        try:
            step = int(np.ceil(len(hyps) / 5))
            parts = []
            for i in range(0, len(hyps), step):
                parts.extend(rescore_with_gpt2(model, tokenizer, device, hyps[i:i + step], length_penalty))
            new_lm = np.array(parts)
        except Exception as e2:
            logging.error(f"OPT rescore failed: {e2}")
            new_lm = np.zeros(len(hyps))
    if ctx is not None:
        hyps = [h[len(ctx) + 1:] for h in hyps]
    total = acoustic_scale * ac + (1 - alpha) * old_lm + alpha * new_lm
    best = int(np.argmax(total))
    n_out = min(len(nbest), len(new_lm), len(total))
    out = [";".join(map(str, [nbest[i][0], nbest[i][1], nbest[i][2], new_lm[i], total[i]])) for i in range(n_out)]
    if not returnConfidence:
        return hyps[best], out
    p = np.exp(total - np.max(total))
    return hyps[best], out, p[best] / np.sum(p)


# ---- checkpoint loading -------------------------------------------------------------------------------------------------
def resolve_model_dir(model_name: str, cache_dir: Optional[str] = None) -> str:
    """The local directory of a checkpoint: model_name itself, or its snapshot in the hub-cache layout
    (<cache>/models--org--name/snapshots/<revision>/) under cache_dir (default: $HF_HUB_CACHE, $HF_HOME/hub,
    ~/.cache/huggingface/hub).  Never downloads."""
    if os.path.isdir(model_name):
        return model_name
    caches = [cache_dir] if cache_dir else [os.environ.get("HF_HUB_CACHE"),
                                             os.path.join(os.environ.get("HF_HOME", os.path.expanduser("~/.cache/huggingface")), "hub")]
    tried = []
    for c in caches:
        if not c:
            continue
        repo = os.path.join(c, "models--" + model_name.replace("/", "--"))
        tried.append(repo)
        snaps = os.path.join(repo, "snapshots")
        if not os.path.isdir(snaps):
            continue
        ref = os.path.join(repo, "refs", "main")
        if os.path.exists(ref):
            with open(ref) as f:
                cand = os.path.join(snaps, f.read().strip())
            if os.path.isdir(cand):
                return cand
        revs = sorted(os.listdir(snaps))
        if revs:
            return os.path.join(snaps, revs[-1])
    raise FileNotFoundError(f"build_opt: no local copy of {model_name!r} (looked for a directory of that name and in {tried}); "
                            "model files are read from disk only, never downloaded")


def _load_state_dict(model_dir: str) -> Dict[str, "object"]:
    import torch
    def st(path):
        from safetensors.torch import load_file
        return load_file(path)

    def pt(path):
        return torch.load(path, map_location="cpu", weights_only=True)
    for index, loader in (("model.safetensors.index.json", st), ("pytorch_model.bin.index.json", pt)):
        p = os.path.join(model_dir, index)
        if os.path.exists(p):
            with open(p) as f:
                files = sorted(set(json.load(f)["weight_map"].values()))
            sd = {}
            for fn in files:
                sd.update(loader(os.path.join(model_dir, fn)))
            return sd
    for single, loader in (("model.safetensors", st), ("pytorch_model.bin", pt)):
        p = os.path.join(model_dir, single)
        if os.path.exists(p):
            return loader(p)
    found = sorted(glob.glob(os.path.join(model_dir, "*.safetensors")) + glob.glob(os.path.join(model_dir, "pytorch_model*.bin")))
    if len(found) == 1:
        return (st if found[0].endswith(".safetensors") else pt)(found[0])
    raise FileNotFoundError(f"build_opt: no weights (*.safetensors or pytorch_model*.bin) in {model_dir}")


def opt_dims(cfg: dict) -> dict:
    """The dimensions b2t_clm_t needs, after refusing what the kernels do not run."""
    d = int(cfg["hidden_size"])
    if not cfg.get("do_layer_norm_before", True):
        raise ValueError("OPT with do_layer_norm_before=False (post-LN, opt-350m) is not supported")
    if int(cfg.get("word_embed_proj_dim", d)) != d:
        raise ValueError(f"OPT with word_embed_proj_dim {cfg['word_embed_proj_dim']} != hidden_size {d} (opt-350m's "
                         "projection layers) is not supported")
    act = cfg.get("activation_function", "relu")
    if act != "relu":
        raise ValueError(f"OPT activation {act!r} is not supported (ReLU only)")
    heads = int(cfg["num_attention_heads"])
    if d % heads or d // heads not in HEAD_DIMS:
        raise ValueError(f"head dim {d}/{heads} is not supported (one of {HEAD_DIMS})")
    ffn = int(cfg["ffn_dim"])
    if d % 64 or ffn % 64:
        raise ValueError(f"hidden_size {d} and ffn_dim {ffn} must be multiples of 64")
    return dict(n_layers=int(cfg["num_hidden_layers"]), d_model=d, n_heads=heads, ffn_dim=ffn, vocab=int(cfg["vocab_size"]),
                max_pos=int(cfg["max_position_embeddings"]))


def _pad_rows(w, rows):
    import torch
    if w.shape[0] == rows:
        return w
    return torch.cat([w, w.new_zeros((rows - w.shape[0],) + tuple(w.shape[1:]))], 0)


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def device_layout(state: dict, dims: dict) -> Dict[str, "object"]:
    """Host (CPU) fp16 tensors in the layout of b2t_clm_t from an OPT state dict (keys with or without the 'model.' prefix,
    lm_head tied to embed_tokens).  Names: embed_tokens, embed_positions, final_ln_w, final_ln_b, layers.<i>.<field>."""
    import torch
    sd = {}
    for k, v in state.items():
        sd[k[len("model."):] if k.startswith("model.") else k] = v
    d, ffn, V = dims["d_model"], dims["ffn_dim"], dims["vocab"]

    def get(name, shape=None, default=None):
        if name not in sd:
            if default is None:
                raise KeyError(f"OPT checkpoint lacks {name}")
            return default
        t = sd[name].detach().to("cpu", torch.float16).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    ones, zeros = torch.ones(d, dtype=torch.float16), torch.zeros(d, dtype=torch.float16)
    emb = get("decoder.embed_tokens.weight", (V, d))
    if "lm_head.weight" in sd and not torch.equal(get("lm_head.weight", (V, d)), emb):
        raise ValueError("OPT checkpoint with an lm_head not tied to embed_tokens is not supported")
    out = {"embed_tokens": _pad_rows(emb, _rup(V, ROWPAD)),
           "embed_positions": get("decoder.embed_positions.weight", (dims["max_pos"] + 2, d)),
           "final_ln_w": get("decoder.final_layer_norm.weight", (d,), ones),
           "final_ln_b": get("decoder.final_layer_norm.bias", (d,), zeros)}
    for i in range(dims["n_layers"]):
        p = f"decoder.layers.{i}."
        lin = lambda n, shp: get(p + n + ".weight", shp)
        bias = lambda n, sz: get(p + n + ".bias", (sz,), torch.zeros(sz, dtype=torch.float16))
        L = {"ln1_w": get(p + "self_attn_layer_norm.weight", (d,), ones), "ln1_b": get(p + "self_attn_layer_norm.bias", (d,), zeros),
             "qkv_w": _pad_rows(torch.cat([lin("self_attn.q_proj", (d, d)), lin("self_attn.k_proj", (d, d)),
                                           lin("self_attn.v_proj", (d, d))], 0), _rup(3 * d, ROWPAD)),
             "qkv_b": torch.cat([bias("self_attn.q_proj", d), bias("self_attn.k_proj", d), bias("self_attn.v_proj", d)]),
             "out_w": _pad_rows(lin("self_attn.out_proj", (d, d)), _rup(d, ROWPAD)), "out_b": bias("self_attn.out_proj", d),
             "ln2_w": get(p + "final_layer_norm.weight", (d,), ones), "ln2_b": get(p + "final_layer_norm.bias", (d,), zeros),
             "fc1_w": _pad_rows(lin("fc1", (ffn, d)), _rup(ffn, ROWPAD)), "fc1_b": bias("fc1", ffn),
             "fc2_w": _pad_rows(lin("fc2", (d, ffn)), _rup(d, ROWPAD)), "fc2_b": bias("fc2", d)}
        for f in _LAYER_FIELDS:
            out[f"layers.{i}.{f}"] = L[f]
    return out


def load_opt_arrays(model_dir: str) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host fp16 tensors in the device layout) of the checkpoint in model_dir."""
    with open(os.path.join(model_dir, "config.json")) as f:
        cfg = json.load(f)
    dims = opt_dims(cfg)
    return dims, device_layout(_load_state_dict(model_dir), dims)


class _Scorer:
    """What OptScorer and LlamaScorer share: packing and validating the ids, growing the workspace, the outputs, the context
    cache and the `score` / `token_logprobs` / `eval` surface.  A subclass builds its descriptor (`desc`, with `device`,
    `share_prefixes`, `last_stats` and `_ws` = None) and calls `_alloc_cache`; the names and the leading arguments of its library
    calls on the path "flat", "tree" or "cached" (`_cache_kv_bytes`, `_sizes`, `_score`) follow from the class data below."""
    _cache = None
    _NO_CACHE = ""    # the ValueError of use_cache=True on a scorer without a context cache
    _CONTEXT_CACHE = True   # False: the family has no cached call, and refuses context_cache_tokens > 0 itself
    _SIZES = ""       # the family's size functions: _SIZES + ws_bytes / tree_ws_bytes / cache_kv_bytes / tree_cached_ws_bytes
    _size_args = ()   # what the workspace size functions take between the model and the sizes (Mixtral: its MoE descriptor)
    _CACHE_SIZES = None   # where the cache is another family's (Mixtral: Llama's), that family's _SIZES: its cache_kv_bytes takes
    #                       the model alone.  None: _SIZES + cache_kv_bytes, with _size_args
    _ENTRY = None     # the entry points: _ENTRY + score_<suffix> / score_tree_<suffix> / score_tree_cached_f16.  None:
    #                   b2t_clm_<_family>_, from the instance's _family
    _qk = ()          # what the entry points take between the model and the lists (or the cache)
    _suffix = "f16"   # the compute dtype in the entry points' names

    def eval(self):   # the reference calls model.eval(); scoring has no training mode
        return self

    def _cache_kv_bytes(self, lib, cap):
        """Bytes of the cache's K / V for `cap` positions by the family's library call (0: cap outside [1, max_pos])."""
        import ctypes as C
        prefix, args = (self._SIZES, self._size_args) if self._CACHE_SIZES is None else (self._CACHE_SIZES, ())
        return getattr(lib, prefix + "cache_kv_bytes")(C.byref(self.desc), *args, cap)

    def _alloc_cache(self, context_cache_tokens):
        """context_cache_tokens > 0: the caller-owned b2t_clm_cache_t of that many positions, on the scorer's device."""
        import torch
        import b2t_native as N
        name = type(self).__name__
        self.context_cache_tokens = int(context_cache_tokens)
        self._cache = None
        if self.context_cache_tokens < 0:
            raise ValueError(f"{name}: context_cache_tokens < 0")
        if self.context_cache_tokens > 0:
            cap = self.context_cache_tokens
            nbytes = self._cache_kv_bytes(N.load(), cap)
            if nbytes == 0:
                raise ValueError(f"{name}: context_cache_tokens {cap} outside [1, max_pos {self.dims['max_pos']}]")
            self._cache_kv = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._cache_logp = torch.empty(cap, dtype=torch.float32, device=self.device)
            self._cache_ids = np.zeros(cap, np.int32)
            self._cache = N.ClmCache(self._cache_kv.data_ptr(), self._cache_logp.data_ptr(), self._cache_ids.ctypes.data, cap, 0)

    @property
    def cache_len(self) -> int:
        """Positions the context cache holds (0 without a cache)."""
        return int(self._cache.n) if self._cache is not None else 0

    @property
    def cache_ids(self) -> np.ndarray:
        """The cached token chain (a copy)."""
        return self._cache_ids[:self.cache_len].copy() if self._cache is not None else np.zeros(0, np.int32)

    def cache_reset(self, keep: int = 0) -> None:
        """Forget the cached context beyond its first `keep` positions (default: all of it).  Never needed for correctness
        (the cache is matched by token ids)."""
        if self._cache is not None:
            self._cache.n = max(0, min(int(keep), int(self._cache.n)))

    def _sizes(self, lib, path, ids, off):
        """(rows computed, positions reused, workspace bytes) of a call on `path` for the packed ids / offsets."""
        import ctypes as C
        desc, M, n_seq = (C.byref(self.desc),) + tuple(self._size_args), len(ids), len(off) - 1
        if path == "cached":
            plan = cache_plan(self._cache_ids[:self._cache.n], self._cache.cap, ids, off)
            return plan["rows"], plan["reused"], getattr(lib, self._SIZES + "tree_cached_ws_bytes")(*desc, plan["rows"], M, n_seq)
        if path == "tree":
            nodes = tree_plan(ids, off)[2]
            return nodes, 0, getattr(lib, self._SIZES + "tree_ws_bytes")(*desc, nodes, M, n_seq)
        return M, 0, getattr(lib, self._SIZES + "ws_bytes")(*desc, M, n_seq)

    def _score(self, lib, path, update_cache, ids, off, n_seq, scores, tok, ws, ws_bytes, stream):
        """The library call of `path`; every array argument is an address (tok may be None)."""
        import ctypes as C
        import b2t_native as N
        desc = C.byref(self.desc)
        pre = (self._ENTRY or f"b2t_clm_{self._family}_") + "score_"
        if path == "cached":
            name = pre + "tree_cached_f16"
            N.check(getattr(lib, name)(desc, *self._qk, C.byref(self._cache), 1 if update_cache else 0, ids, off, n_seq,
                                       scores, tok, None, None, ws, ws_bytes, stream), name)
        elif path == "tree":
            name = pre + "tree_" + self._suffix
            N.check(getattr(lib, name)(desc, *self._qk, ids, off, n_seq, scores, tok, None, ws, ws_bytes, stream), name)
        else:
            name = pre + self._suffix
            N.check(getattr(lib, name)(desc, *self._qk, ids, off, n_seq, scores, tok, ws, ws_bytes, stream), name)

    def _run(self, ids_list, want_tokens: bool, share_prefixes: Optional[bool] = None, use_cache: Optional[bool] = None,
             update_cache: bool = True):
        import torch
        import b2t_native as N
        name = type(self).__name__
        tree = self.share_prefixes if share_prefixes is None else bool(share_prefixes)
        cached = self._cache is not None if use_cache is None else bool(use_cache)
        if cached and self._cache is None:
            raise ValueError(f"{name}: {self._NO_CACHE}")
        lib = N.load()
        seqs = [np.asarray(s, dtype=np.int64).reshape(-1) for s in ids_list]
        if not seqs:
            self.last_stats = {"tokens": 0, "nodes": 0}
            return np.zeros(0, np.float32), np.zeros(0, np.int64), None
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        if int(lens.min()) < 1:
            raise ValueError(f"{name}: empty token sequence")
        if lens.sum() > np.iinfo(np.int32).max:
            raise ValueError(f"{name}: too many tokens")
        ids = np.ascontiguousarray(np.concatenate(seqs).astype(np.int32))
        off = np.zeros(len(seqs) + 1, dtype=np.int32)
        off[1:] = np.cumsum(lens)
        M = int(off[-1])
        path = "cached" if cached else "tree" if tree else "flat"
        nodes, reused, need = self._sizes(lib, path, ids, off)
        if need == 0:
            raise RuntimeError(f"{self._SIZES}ws_bytes: invalid sizes: {N.last_error()}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        scores = torch.empty(len(seqs), dtype=torch.float32, device=self.device)
        tok = torch.empty(M, dtype=torch.float32, device=self.device) if want_tokens else None
        with torch.cuda.device(self.device):
            self._score(lib, path, update_cache, ids.ctypes.data, off.ctypes.data, len(seqs), scores.data_ptr(),
                        tok.data_ptr() if tok is not None else None, self._ws.data_ptr(), self._ws.numel(),
                        torch.cuda.current_stream(self.device).cuda_stream)
            s = scores.cpu().numpy()
            t = tok.cpu().numpy() if tok is not None else None
        self.last_stats = {"tokens": M, "nodes": int(nodes)}
        if cached:
            self.last_stats["reused"] = int(reused)
        return s, lens, t

    def score(self, ids_list, length_penalty: float = 0.0, share_prefixes: Optional[bool] = None,
              use_cache: Optional[bool] = None, update_cache: bool = True) -> np.ndarray:
        """Per sequence: sum_{t>=1} log p(id[t] | id[<t]) - len * length_penalty, in fp32 as the reference's numpy scores.
        share_prefixes: None = the scorer's own setting.  use_cache: None = cached iff the scorer has a context cache (True
        on a scorer without one raises); a cached call shares prefixes whatever share_prefixes says.  update_cache=False
        reads the cache and leaves it as it was."""
        s, lens, _ = self._run(ids_list, False, share_prefixes, use_cache, update_cache)
        return s.astype(np.float32) - (lens * float(length_penalty)).astype(np.float32)

    def token_logprobs(self, ids_list, share_prefixes: Optional[bool] = None, use_cache: Optional[bool] = None,
                       update_cache: bool = True) -> List[np.ndarray]:
        """Per sequence the fp32 log-prob of each token given its prefix (0 for the first token)."""
        _, lens, t = self._run(ids_list, True, share_prefixes, use_cache, update_cache)
        off = np.concatenate([[0], np.cumsum(lens)])
        return [t[off[i]:off[i + 1]] for i in range(len(lens))]


class OptScorer(_Scorer):
    """An OPT decoder on the GPU in the b2t_clm_t layout; `score` runs b2t_clm_score_f16 on packed ids, or, with
    share_prefixes, b2t_clm_score_tree_f16: the same forward over the list's shared-prefix token tree (each distinct prefix
    computed once; results bit-identical to the flat call).  `share_prefixes` here is the default of `score` and
    `token_logprobs`; after a call `last_stats` = {"tokens": packed tokens, "nodes": rows computed}.

    context_cache_tokens > 0 allocates a context cache of that many positions (n_layers * 4 * d_model bytes each: 512 KiB at
    the OPT-6.7b shape, 1 GiB for 2048) and makes `score` / `token_logprobs` take b2t_clm_score_tree_cached_f16: the tree
    forward (prefixes shared by construction) in which the positions of the list's common prefix that an earlier call already
    computed are read from the cache instead.  The cache is matched by token ids, so it is never wrong, only more or less
    useful; results stay bit-identical.  Per call `use_cache` = None (the scorer's setting) | True | False; after a cached
    call `last_stats` = {"tokens", "nodes": rows computed, "reused": positions taken from the cache}."""

    _NO_CACHE = "use_cache=True on a scorer built without context_cache_tokens"
    _SIZES = "b2t_clm_"   # GPT-2's too
    _ENTRY = "b2t_clm_"
    _dtype_of = staticmethod(lambda dtype: opt_dtype(dtype))

    def __init__(self, dims: dict, arrays: Dict[str, "object"], device="cuda", share_prefixes: bool = False,
                 context_cache_tokens: int = 0, dtype=None):
        import torch
        import b2t_native as N
        self.dtype = self._dtype_of(dtype)   # fp16 alone: bfloat16 is refused
        self.dims = dict(dims)
        self.device = torch.device(device)
        self.share_prefixes = bool(share_prefixes)
        self.last_stats = None
        self.w = {k: v.to(self.device, torch.float16).contiguous() for k, v in arrays.items()}
        self._layers = (N.ClmLayer * max(1, dims["n_layers"]))()
        for i in range(dims["n_layers"]):
            for f in _LAYER_FIELDS:
                setattr(self._layers[i], f, self.w[f"layers.{i}.{f}"].data_ptr())
        self.desc = N.ClmDesc(dims["n_layers"], dims["d_model"], dims["n_heads"], dims["ffn_dim"], dims["vocab"], dims["max_pos"],
                              self.w["embed_tokens"].data_ptr(), self.w["embed_positions"].data_ptr(),
                              self.w["final_ln_w"].data_ptr(), self.w["final_ln_b"].data_ptr(), self._layers)
        self._ws = None
        self._alloc_cache(context_cache_tokens)


# ---- the compute dtype ----------------------------------------------------------------------------------------------------
CLM_DTYPES = ("float16", "bfloat16")


def clm_dtype(dtype, cfg: Optional[dict] = None):
    """The torch dtype a scorer computes in, from the `dtype` argument of the scorers and builders: None or "float16" (or
    torch.float16) -> torch.float16; "bfloat16" (or torch.bfloat16) -> torch.bfloat16; "auto" -> what config.json (cfg) says
    the checkpoint was saved in, under "torch_dtype" or the newer "dtype": bfloat16 if it says so, float16 for anything
    else.  Any other value is a ValueError."""
    import torch
    if dtype is None:
        return torch.float16
    if isinstance(dtype, torch.dtype):
        dtype = str(dtype).replace("torch.", "")
    if dtype == "auto":
        if cfg is None:
            raise ValueError('dtype "auto" needs the checkpoint\'s config.json (build_scorer / build_opt)')
        saved = cfg.get("torch_dtype", cfg.get("dtype"))
        dtype = "bfloat16" if str(saved).replace("torch.", "") == "bfloat16" else "float16"
    if dtype not in CLM_DTYPES:
        raise ValueError(f"dtype {dtype!r} is not supported (None, {', '.join(repr(d) for d in CLM_DTYPES)} or 'auto')")
    return getattr(torch, dtype)


def opt_dtype(dtype, cfg: Optional[dict] = None):
    """clm_dtype for an OPT checkpoint, which computes in fp16 alone ("auto" is fp16 whatever the config says)."""
    import torch
    if dtype == "auto":
        return torch.float16
    if clm_dtype(dtype, cfg) != torch.float16:
        raise ValueError("OptScorer: dtype 'bfloat16' is not supported for OPT checkpoints (the reference loads OPT in float16); "
                         "the Llama family has a bfloat16 mode")
    return torch.float16


def gpt2_dtype(dtype, cfg: Optional[dict] = None):
    """clm_dtype for a GPT-2 checkpoint, which computes in fp16 alone, as OPT does ("auto" is fp16 whatever the config says)."""
    import torch
    if dtype == "auto":
        return torch.float16
    if clm_dtype(dtype, cfg) != torch.float16:
        raise ValueError("Gpt2Scorer: dtype 'bfloat16' is not supported for GPT-2 checkpoints (they are published in float32 and "
                         "the reference loads them in float16); the Llama family has a bfloat16 mode")
    return torch.float16


def llama_check_dtype_cache(dtype, context_cache_tokens) -> None:
    """Refuses bfloat16 together with a context cache: the cached path exists in fp16 only."""
    import torch
    if dtype == torch.bfloat16 and int(context_cache_tokens) > 0:
        raise ValueError("LlamaScorer: dtype 'bfloat16' with context_cache_tokens > 0 is not supported yet: the context cache "
                         "behind bfloat16 is the follow-up to the bfloat16 mode; use dtype 'float16' or context_cache_tokens=0")


def reader(state: dict, wdt, who: str = "", device=None):
    """get(name, shape, to=None) over a state dict, for every *_device_layout: the tensor `name` cast to `to` (default wdt) on
    `device` (default: where it is) and contiguous, after checking that it is there (a KeyError that starts with `who` and names
    the tensor) and, cast, has `shape` (ValueError).  get.raw(name) is the tensor as stored, behind the first check alone."""
    def raw(name):
        if name not in state:
            raise KeyError(f"{who}checkpoint lacks {name}")
        return state[name].detach()

    def get(name, shape, to=None):
        t = raw(name).to(device=device, dtype=to or wdt).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    get.raw = raw
    return get


# ---- GPT-2 (HF GPT2LMHeadModel) ------------------------------------------------------------------------------------------
GPT2_ACTIVATIONS = ("gelu_new", "gelu_pytorch_tanh")   # two names of 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3)))


def gpt2_dims(cfg: dict) -> dict:
    """The dimensions b2t_clm_t needs from a GPT-2 config.json, after refusing what the kernels do not run.  Behind the loader
    GPT-2 is the pre-LN OPT forward with gelu_new in the fc1 GEMM's epilogue (csrc/causal_lm_gpt2.hip)."""
    act = cfg.get("activation_function", "gelu_new")
    if act not in GPT2_ACTIVATIONS:
        raise ValueError(f"gpt2 activation_function {act!r} is not supported ({' or '.join(GPT2_ACTIVATIONS)}: the tanh form; "
                         '"gelu", the erf form, is a different function and is not built)')
    if not cfg.get("scale_attn_weights", True):
        raise ValueError("gpt2 with scale_attn_weights=False is not supported (q is scaled by head_dim^-0.5)")
    if cfg.get("scale_attn_by_inverse_layer_idx", False):
        raise ValueError("gpt2 with scale_attn_by_inverse_layer_idx=True is not supported")
    if cfg.get("add_cross_attention", False):
        raise ValueError("gpt2 with add_cross_attention=True is not supported")
    eps = float(cfg.get("layer_norm_epsilon", 1e-5))
    if eps != 1e-5:
        raise ValueError(f"gpt2 layer_norm_epsilon {eps} is not supported (the LayerNorm kernel's eps is the constant 1e-5)")
    d, heads = int(cfg["n_embd"]), int(cfg["n_head"])
    if d % heads or d // heads not in HEAD_DIMS:
        raise ValueError(f"head dim n_embd {d} / n_head {heads} is not supported (one of {HEAD_DIMS})")
    ffn = int(cfg["n_inner"]) if cfg.get("n_inner") is not None else 4 * d
    if d % 64 or ffn % 64:
        raise ValueError(f"n_embd {d} and the ffn width (n_inner) {ffn} must be multiples of 64")
    # reorder_and_upcast_attn changes where HF scales and in which format it multiplies, not the function: accepted either way
    return dict(n_layers=int(cfg["n_layer"]), d_model=d, n_heads=heads, ffn_dim=ffn, vocab=int(cfg["vocab_size"]),
                max_pos=int(cfg["n_positions"]))


def gpt2_device_layout(state: dict, dims: dict) -> Dict[str, "object"]:
    """Host (CPU) fp16 tensors in the layout of b2t_clm_t (device_layout's names) from a GPT2LMHeadModel state dict, keys with
    or without the 'transformer.' prefix; the attn.bias / attn.masked_bias buffers of old checkpoints are ignored.  The
    checkpoint's Conv1D weights are [in][out]: c_attn [d][3d] becomes qkv_w [3d][d] with rows q | k | v, and attn.c_proj,
    mlp.c_fc, mlp.c_proj are transposed the same way to out_w, fc1_w, fc2_w; rows are padded to 256.  embed_positions is wpe
    behind two zero rows (the embed kernel reads row position + 2, OPT's offset); ln_f is the final LayerNorm; the head is wte
    (an lm_head that is not wte is refused).  fp32 checkpoints are rounded to fp16 once, as torch_dtype=float16 does."""
    import torch
    sd = {}
    for k, v in state.items():
        k = k[len("transformer."):] if k.startswith("transformer.") else k
        if k.endswith(".attn.bias") or k.endswith(".attn.masked_bias"):
            continue
        sd[k] = v
    d, ffn, V = dims["d_model"], dims["ffn_dim"], dims["vocab"]

    get = reader(sd, torch.float16, "GPT-2 ", device="cpu")

    def conv1d(name, n_in, n_out):   # Conv1D weight [in][out] -> nn.Linear rows [out][in], padded
        return _pad_rows(get(name + ".weight", (n_in, n_out)).t().contiguous(), _rup(n_out, ROWPAD))
    emb = get("wte.weight", (V, d))
    if "lm_head.weight" in sd and not torch.equal(get("lm_head.weight", (V, d)), emb):
        raise ValueError("GPT-2 checkpoint with an lm_head that is not wte (untied) is not supported")
    wpe = get("wpe.weight", (dims["max_pos"], d))
    out = {"embed_tokens": _pad_rows(emb, _rup(V, ROWPAD)),
           "embed_positions": torch.cat([wpe.new_zeros((2, d)), wpe], 0).contiguous(),
           "final_ln_w": get("ln_f.weight", (d,)), "final_ln_b": get("ln_f.bias", (d,))}
    for i in range(dims["n_layers"]):
        p = f"h.{i}."
        L = {"ln1_w": get(p + "ln_1.weight", (d,)), "ln1_b": get(p + "ln_1.bias", (d,)),
             "qkv_w": conv1d(p + "attn.c_attn", d, 3 * d), "qkv_b": get(p + "attn.c_attn.bias", (3 * d,)),
             "out_w": conv1d(p + "attn.c_proj", d, d), "out_b": get(p + "attn.c_proj.bias", (d,)),
             "ln2_w": get(p + "ln_2.weight", (d,)), "ln2_b": get(p + "ln_2.bias", (d,)),
             "fc1_w": conv1d(p + "mlp.c_fc", d, ffn), "fc1_b": get(p + "mlp.c_fc.bias", (ffn,)),
             "fc2_w": conv1d(p + "mlp.c_proj", ffn, d), "fc2_b": get(p + "mlp.c_proj.bias", (d,))}
        for f in _LAYER_FIELDS:
            out[f"layers.{i}.{f}"] = L[f]
    return out


def load_gpt2_arrays(model_dir: str) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host fp16 tensors in the device layout) of the GPT-2 checkpoint in model_dir."""
    return _load_arrays(FAMILIES["gpt2"], model_dir)


class Gpt2Scorer(OptScorer):
    """A GPT-2 decoder on the GPU in the b2t_clm_t layout (gpt2_device_layout): OptScorer's constructor, `score` /
    `token_logprobs`, share_prefixes and context cache, with the b2t_clm_gpt2_score_f16 / _tree_f16 / _tree_cached_f16 entry
    points (csrc/causal_lm_gpt2.hip), whose fc1 GEMM applies gelu_new where OPT's applies ReLU.  Sizes and the cache are the
    OPT calls'.  fp16 only, like OPT."""

    _ENTRY = "b2t_clm_gpt2_"
    _dtype_of = staticmethod(lambda dtype: gpt2_dtype(dtype))


# ---- GPT-NeoX (HF GPTNeoXForCausalLM with head dim 64 or 128: Pythia) ------------------------------------------------------
NEOX_HEAD_DIMS = (64, 128)
NEOX_ACT_GELU_ERF, NEOX_ACT_GELU_TANH = 0, 1   # b2t_clm_neox_t.act (B2T_CLM_NEOX_ACT_*)
# hidden_act -> act: "gelu" is the erf form; the other three are one tanh function, GPT-2's gelu_new
NEOX_ACTIVATIONS = {"gelu": NEOX_ACT_GELU_ERF, "gelu_new": NEOX_ACT_GELU_TANH, "gelu_fast": NEOX_ACT_GELU_TANH,
                    "gelu_pytorch_tanh": NEOX_ACT_GELU_TANH}


def neox_dtype(dtype, cfg: Optional[dict] = None):
    """clm_dtype for a GPT-NeoX checkpoint, which computes in fp16 alone, the format the family is published in ("auto" is
    fp16 whatever the config says)."""
    import torch
    if dtype == "auto":
        return torch.float16
    if clm_dtype(dtype, cfg) != torch.float16:
        raise ValueError("NeoxScorer: dtype 'bfloat16' is not supported for GPT-NeoX checkpoints (the Pythia suite is "
                         "published in float16); the Llama family has a bfloat16 mode")
    return torch.float16


def _neox_rope(cfg: dict) -> Tuple[float, float, str]:
    """(partial rotary factor, theta, rope type) of a GPT-NeoX config in either spelling: rotary_pct / rotary_emb_base (the
    Hub's config.json files, with an optional rope_scaling) or rope_parameters.{partial_rotary_factor, rope_theta, rope_type}."""
    rp = dict(cfg.get("rope_parameters") or cfg.get("rope_scaling") or {})
    pct = rp.get("partial_rotary_factor", cfg.get("rotary_pct", cfg.get("partial_rotary_factor", 0.25)))
    theta = rp.get("rope_theta", cfg.get("rotary_emb_base", cfg.get("rope_theta", 10000)))
    return float(pct), float(theta), str(rp.get("rope_type", rp.get("type", "default")))


def neox_dims(cfg: dict) -> dict:
    """The dimensions b2t_clm_neox_t needs from a GPT-NeoX config.json, after refusing what the kernels do not run."""
    if not cfg.get("use_parallel_residual", True):
        raise ValueError("gpt_neox with use_parallel_residual=False is not supported (the forward is x + attn(ln1(x)) + "
                         "mlp(ln2(x)); sequential-residual checkpoints are not built)")
    if not cfg.get("attention_bias", True):
        raise ValueError("gpt_neox with attention_bias=False is not supported (the projections are biased)")
    eps = float(cfg.get("layer_norm_eps", 1e-5))
    if eps != 1e-5:
        raise ValueError(f"gpt_neox layer_norm_eps {eps} is not supported (the LayerNorm kernel's eps is the constant 1e-5)")
    pct, _, kind = _neox_rope(cfg)
    if kind != "default":
        raise ValueError(f"gpt_neox rope_type {kind!r} is not supported (default only)")
    act = cfg.get("hidden_act", "gelu")
    if act not in NEOX_ACTIVATIONS:
        raise ValueError(f"gpt_neox hidden_act {act!r} is not supported ({', '.join(NEOX_ACTIVATIONS)})")
    d, heads = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    if d % heads or d // heads not in NEOX_HEAD_DIMS:
        raise ValueError(f"gpt_neox head dim hidden_size {d} / num_attention_heads {heads} is not supported (one of "
                         f"{NEOX_HEAD_DIMS}; pythia-2.8b has head dim 80, gpt-neox-20b 96 and pythia-1b 256, which are not built)")
    hd = d // heads
    rot = int(hd * pct)
    if rot not in (hd // 4, hd // 2, hd):
        raise ValueError(f"gpt_neox rotary_pct {pct} gives {rot} rotary dims of head dim {hd}, which is not supported "
                         f"({hd // 4}, {hd // 2} or {hd})")
    ffn = int(cfg["intermediate_size"])
    if d % 64 or ffn % 64:
        raise ValueError(f"hidden_size {d} and intermediate_size {ffn} must be multiples of 64")
    return dict(n_layers=int(cfg["num_hidden_layers"]), d_model=d, n_heads=heads, ffn_dim=ffn, vocab=int(cfg["vocab_size"]),
                max_pos=int(cfg["max_position_embeddings"]), rotary_ndims=rot, act=NEOX_ACTIVATIONS[act],
                tied=bool(cfg.get("tie_word_embeddings", False)))


def neox_inv_freq(cfg: dict) -> np.ndarray:
    """fp32 inv_freq[rotary_ndims / 2] of a GPT-NeoX config, computed as HF computes it (fp32 torch arithmetic): the default
    rope over the rotary dims, 1 / theta^(2 i / rotary_ndims)."""
    import torch
    pct, theta, _ = _neox_rope(cfg)
    dim = neox_dims(cfg)["rotary_ndims"]
    return (1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))).numpy().astype(np.float32)


def neox_head_perm(hd: int, rotary_ndims: int) -> np.ndarray:
    """stored row i of a q / k head = original row perm[i], such that every rotary pair (f, f + rotary_ndims / 2) sits 32 rows
    apart inside one 64-row slice -- pair f in slice f // 32 at rows f % 32 and 32 + f % 32, which is where EP_ROPE_PART
    (csrc/clm_gemm.h) looks for it -- and the pass-through rows fill the remaining places in order.  hd 64 with 16 rotary dims:
    [0..7, 16..39, 8..15, 40..63]; hd 128 with 32: [0..15, 32..47, 16..31, 48..63, 64..127]; rotary_ndims == hd: head_dim_perm."""
    if hd not in NEOX_HEAD_DIMS or rotary_ndims not in (hd // 4, hd // 2, hd):
        raise ValueError(f"head dim {hd} with {rotary_ndims} rotary dims is not supported")
    half = rotary_ndims // 2
    perm = np.full(hd, -1, np.int64)
    for f in range(half):
        at = 64 * (f // 32) + f % 32
        perm[at], perm[at + 32] = f, f + half
    perm[perm < 0] = np.arange(rotary_ndims, hd)
    return perm


def neox_device_layout(state: dict, dims: dict, inv_freq: np.ndarray) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_neox_t from a GPTNeoXForCausalLM state dict, on the device the state dict is on (the
    CPU for a checkpoint read from disk; the rotary tables are CPU tensors either way).  Keys with or without the 'gpt_neox.'
    prefix; the attention.bias / masked_bias / rotary_emb.inv_freq buffers of old checkpoints are ignored.  fp16
    embed_in, embed_out (the same tensor when tied), final_ln_w / final_ln_b, layers.<i>.<field> under device_layout's names,
    and the fp32 rope_cos / rope_sin [max_pos][rotary_ndims / 2].  query_key_value's rows are interleaved per head,
    [h][q | k | v][hd]: they are de-interleaved to q | k | v rows, then every q and k head's rows (and bias entries) are stored
    under neox_head_perm.  v and attention.dense are stored as they are; rows are padded to 256."""
    import torch
    sd = {}
    for k, v in state.items():
        k = k[len("gpt_neox."):] if k.startswith("gpt_neox.") else k
        if k.endswith((".attention.bias", ".attention.masked_bias", ".rotary_emb.inv_freq")):
            continue
        sd["embed_out.weight" if k == "lm_head.weight" else k] = v   # the head's name in memory in recent transformers
    d, ffn, V, H = dims["d_model"], dims["ffn_dim"], dims["vocab"], dims["n_heads"]
    hd = d // H

    get = reader(sd, torch.float16, "GPT-NeoX ")
    emb = _pad_rows(get("embed_in.weight", (V, d)), _rup(V, ROWPAD))
    dev = emb.device
    tied = dims.get("tied", False) or "embed_out.weight" not in sd
    cos, sin = rope_tables(inv_freq, dims["max_pos"])
    out = {"embed_in": emb, "embed_out": emb if tied else _pad_rows(get("embed_out.weight", (V, d)), _rup(V, ROWPAD)),
           "final_ln_w": get("final_layer_norm.weight", (d,)), "final_ln_b": get("final_layer_norm.bias", (d,)),
           "rope_cos": torch.from_numpy(cos), "rope_sin": torch.from_numpy(sin)}
    hp = neox_head_perm(hd, dims["rotary_ndims"])
    # stored row i of qkv = de-interleaved row perm[i]: the head permutation inside every q and k head, v as it is
    perm = torch.from_numpy(np.concatenate([h * hd + hp for h in range(2 * H)] + [np.arange(2 * d, 3 * d)])).to(dev)
    # de-interleaved row (j, h, c) = checkpoint row (h, j, c), j = q, k, v
    split = lambda t: t.view(H, 3, hd, *t.shape[1:]).transpose(0, 1).reshape(3 * d, *t.shape[1:])
    for i in range(dims["n_layers"]):
        p = f"layers.{i}."
        L = {"ln1_w": get(p + "input_layernorm.weight", (d,)), "ln1_b": get(p + "input_layernorm.bias", (d,)),
             "qkv_w": _pad_rows(split(get(p + "attention.query_key_value.weight", (3 * d, d)))[perm].contiguous(), _rup(3 * d, ROWPAD)),
             "qkv_b": split(get(p + "attention.query_key_value.bias", (3 * d,)))[perm].contiguous(),
             "out_w": _pad_rows(get(p + "attention.dense.weight", (d, d)), _rup(d, ROWPAD)), "out_b": get(p + "attention.dense.bias", (d,)),
             "ln2_w": get(p + "post_attention_layernorm.weight", (d,)), "ln2_b": get(p + "post_attention_layernorm.bias", (d,)),
             "fc1_w": _pad_rows(get(p + "mlp.dense_h_to_4h.weight", (ffn, d)), _rup(ffn, ROWPAD)),
             "fc1_b": get(p + "mlp.dense_h_to_4h.bias", (ffn,)),
             "fc2_w": _pad_rows(get(p + "mlp.dense_4h_to_h.weight", (d, ffn)), _rup(d, ROWPAD)),
             "fc2_b": get(p + "mlp.dense_4h_to_h.bias", (d,))}
        for f in _LAYER_FIELDS:
            out[f"layers.{i}.{f}"] = L[f]
    return out


def load_neox_arrays(model_dir: str) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the GPT-NeoX checkpoint in model_dir."""
    return _load_arrays(FAMILIES["gpt_neox"], model_dir)


class NeoxScorer(_Scorer):
    """A GPT-NeoX decoder (Pythia; head dim 64 or 128) on the GPU in the b2t_clm_neox_t layout (neox_device_layout), with OptScorer's
    constructor and scoring surface -- `score` / `token_logprobs`, share_prefixes, the context cache with `use_cache` /
    `update_cache` / `cache_len` / `cache_ids` / `cache_reset`, `last_stats` -- on the entry points b2t_clm_neox_score_f16 /
    _tree_f16 / _tree_cached_f16 (csrc/causal_lm_neox.hip): partial rotary positions in the QKV GEMM's epilogue, the erf (or
    tanh) GELU in the fc1 GEMM's, the parallel residual.  A cached position costs n_layers * 4 * d_model bytes.  fp16 only."""

    _NO_CACHE = "use_cache=True on a scorer built without context_cache_tokens"
    _SIZES = _ENTRY = "b2t_clm_neox_"

    def __init__(self, dims: dict, arrays: Dict[str, "object"], device="cuda", share_prefixes: bool = False,
                 context_cache_tokens: int = 0, dtype=None):
        import torch
        import b2t_native as N
        self.dtype = neox_dtype(dtype)   # fp16 alone: bfloat16 is refused
        self.dims = dict(dims)
        self.device = torch.device(device)
        self.share_prefixes = bool(share_prefixes)
        self.last_stats = None
        tied = dims.get("tied", False) or arrays["embed_out"] is arrays["embed_in"]   # then the head is never copied
        self.w = {k: v.to(self.device, torch.float32 if k.startswith("rope_") else torch.float16).contiguous()
                  for k, v in arrays.items() if not (tied and k == "embed_out")}
        if tied:
            self.w["embed_out"] = self.w["embed_in"]
        self._layers = (N.ClmLayer * max(1, dims["n_layers"]))()
        for i in range(dims["n_layers"]):
            for f in _LAYER_FIELDS:
                setattr(self._layers[i], f, self.w[f"layers.{i}.{f}"].data_ptr())
        self.desc = N.ClmNeoxDesc(dims["n_layers"], dims["d_model"], dims["n_heads"], dims["ffn_dim"], dims["vocab"], dims["max_pos"],
                                  dims["rotary_ndims"], dims["act"], self.w["embed_in"].data_ptr(), self.w["embed_out"].data_ptr(),
                                  self.w["final_ln_w"].data_ptr(), self.w["final_ln_b"].data_ptr(),
                                  self.w["rope_cos"].data_ptr(), self.w["rope_sin"].data_ptr(), self._layers)
        self._ws = None
        self._alloc_cache(context_cache_tokens)


# ---- the Llama family (HF LlamaForCausalLM, MistralForCausalLM, Qwen2ForCausalLM, Qwen3ForCausalLM) ---------------------
LLAMA_MODEL_TYPES = ("llama", "mistral", "qwen2", "qwen3")
QK_NORM_MODEL_TYPES = ("qwen3",)   # an RMSNorm over every q and k head in front of the rotation
LLAMA_HEAD_DIMS = (64, 128)
LLAMA_MAX_POSITIONS = 8192   # default cap of the rotary cos / sin table: max_pos * head_dim * 4 bytes (4 MiB at head dim 128)
_LLAMA_LAYER_FIELDS = ("norm1_w", "norm2_w", "qkv_w", "qkv_b", "o_w", "gate_up_w", "down_w")


def _rope_parameters(cfg: dict) -> dict:
    """config.json's rotary description in one dict, from either spelling: rope_parameters (rope_theta inside), or rope_theta
    beside an optional rope_scaling (whose type is under "rope_type" or the older "type")."""
    rp = dict(cfg.get("rope_parameters") or cfg.get("rope_scaling") or {})
    if "rope_type" not in rp:
        rp["rope_type"] = rp.get("type", "default")
    if "rope_theta" not in rp:
        rp["rope_theta"] = cfg.get("rope_theta", 10000.0)
    return rp


def rope_inv_freq(cfg: dict) -> np.ndarray:
    """fp32 inv_freq[head_dim / 2] of a Llama-family config, computed as HF's ROPE_INIT_FUNCTIONS compute it (fp32 torch
    arithmetic, same operation order) for rope_type "default" and "llama3"; every other type is refused."""
    import math
    import torch
    rp = _rope_parameters(cfg)
    kind = rp["rope_type"]
    if kind not in ("default", "llama3"):
        raise ValueError(f"rope_type {kind!r} is not supported (default or llama3)")
    if float(rp.get("partial_rotary_factor", cfg.get("partial_rotary_factor", 1.0)) or 1.0) != 1.0:
        raise ValueError("partial rotary embeddings are not supported")
    dim = int(cfg.get("head_dim") or int(cfg["hidden_size"]) // int(cfg["num_attention_heads"]))
    base = rp["rope_theta"]
    if kind == "default":
        inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))
        return inv.numpy().astype(np.float32)
    inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.int64).to(dtype=torch.float) / dim))
    factor, low, high = rp["factor"], rp["low_freq_factor"], rp["high_freq_factor"]
    old_len = rp["original_max_position_embeddings"]
    low_wavelen, high_wavelen = old_len / low, old_len / high
    wavelen = 2 * math.pi / inv
    inv_l = torch.where(wavelen > low_wavelen, inv / factor, inv)
    smooth = (old_len / wavelen - low) / (high - low)
    smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
    medium = ~(wavelen < high_wavelen) * ~(wavelen > low_wavelen)
    return torch.where(medium, smoothed, inv_l).numpy().astype(np.float32)


def rope_tables(inv_freq: np.ndarray, max_pos: int) -> Tuple[np.ndarray, np.ndarray]:
    """fp32 cos / sin [max_pos][head_dim / 2] of position * inv_freq, the angle and the functions evaluated in double."""
    ang = np.arange(max_pos, dtype=np.float64)[:, None] * np.asarray(inv_freq, np.float32).astype(np.float64)[None, :]
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


# What the *_dims of the families on the b2t_clm_llama_t descriptor share.  Each family calls these in the order of its checks:
# _dims_open, its own head-dim rules, _check_gqa, (_check_moe,) _check_64, its rotary and window rules, _dims_close.
def _dims_open(cfg: dict, types: Tuple[str, ...], act_field: str = "hidden_act", act: str = "silu", act_word: Optional[str] = None,
               act_note: str = "") -> Tuple[str, int, int, int]:
    """(model_type, hidden_size, heads, key / value heads) of a config whose model_type is one of `types` and whose activation
    (config field act_field, called act_word in the message) is `act`."""
    mt = cfg.get("model_type")
    if mt not in types:
        raise ValueError(f"model_type {mt!r} is not " + (f"one of {types}" if len(types) > 1 else repr(types[0])))
    d, Hq = int(cfg["hidden_size"]), int(cfg["num_attention_heads"])
    Hkv = int(cfg.get("num_key_value_heads") or Hq)
    got = cfg.get(act_field, act)
    if got != act:
        raise ValueError(f"{mt} {act_word or act_field} {got!r} is not supported ({act} only{act_note})")
    return mt, d, Hq, Hkv


def _check_gqa(Hq: int, Hkv: int) -> None:
    if Hkv < 1 or Hq % Hkv:
        raise ValueError(f"num_attention_heads {Hq} is not a multiple of num_key_value_heads {Hkv}")


def _check_64(d: int, ffn: int, more: Optional[Dict[str, int]] = None) -> None:
    """Refuses GEMM widths that are not multiples of 64: hidden_size, intermediate_size and the family's further ones, `more`,
    which maps the wording of each in the message to its value."""
    widths = {"hidden_size": d, "intermediate_size": ffn, **(more or {})}
    if any(w % 64 for w in widths.values()):
        said = [f"{k} {w}" for k, w in widths.items()]
        raise ValueError(f"{', '.join(said[:-1])} and {said[-1]} must be multiples of 64")


def _check_moe(ne: int, k: int, max_experts: int, max_top_k: int) -> None:
    if not 1 <= ne <= max_experts:
        raise ValueError(f"num_local_experts {ne} outside [1, {max_experts}]")
    if not 1 <= k <= min(max_top_k, ne):
        raise ValueError(f"num_experts_per_tok {k} outside [1, min({max_top_k}, num_local_experts {ne})]")


def _dims_close(cfg: dict, d: int, Hq: int, Hkv: int, ffn: int, max_pos: int, max_positions: Optional[int], rms_eps: float,
                **own) -> dict:
    """The dims every family's descriptor starts from, max_pos (already lowered to the family's window) capped by max_positions
    (default LLAMA_MAX_POSITIONS) and rms_eps the family's default; `own` adds the family's entries (or fixes `tied`)."""
    cap = LLAMA_MAX_POSITIONS if max_positions is None else int(max_positions)
    if cap < 1:
        raise ValueError(f"max_positions {cap} < 1")
    dims = dict(n_layers=int(cfg["num_hidden_layers"]), d_model=d, n_heads=Hq, n_kv_heads=Hkv, ffn_dim=ffn,
                vocab=int(cfg["vocab_size"]), max_pos=min(max_pos, cap), rms_eps=float(cfg.get("rms_norm_eps", rms_eps)),
                tied=bool(cfg.get("tie_word_embeddings", False)))
    dims.update(own)
    return dims


def llama_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t needs, after refusing what the kernels do not run.  max_pos is the model's
    max_position_embeddings, lowered to the sliding window where one is configured and in use (within it full causal attention
    is what the model computes) and to max_positions (default LLAMA_MAX_POSITIONS), which sizes the rotary table."""
    mt, d, Hq, Hkv = _dims_open(cfg, LLAMA_MODEL_TYPES, act_word="activation")
    if d % Hq or d // Hq not in LLAMA_HEAD_DIMS or int(cfg.get("head_dim") or d // Hq) != d // Hq:
        hint = ""
        if mt == "qwen3":
            hint = ("; Qwen3-1.7B, 8B and 14B have head_dim = hidden_size / heads, Qwen3-0.6B, 4B and 32B a head_dim of its own, "
                    "which is not supported")
        raise ValueError(f"head dim {cfg.get('head_dim') or d}/{Hq} is not supported (hidden_size / heads, one of "
                         f"{LLAMA_HEAD_DIMS}){hint}")
    if mt in QK_NORM_MODEL_TYPES and cfg.get("attention_bias"):
        raise ValueError(f"{mt} with attention_bias=True is not supported (the q / k norm epilogue adds no bias)")
    _check_gqa(Hq, Hkv)
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn)
    if cfg.get("mlp_bias"):
        raise ValueError("mlp_bias=True is not supported")
    rope_inv_freq(cfg)   # refuses the rotary variants the table does not describe
    max_pos = int(cfg["max_position_embeddings"])
    window = cfg.get("sliding_window")
    in_use = window is not None and (mt == "mistral" or (bool(cfg.get("use_sliding_window")) and
                                                         "sliding_attention" in (cfg.get("layer_types") or ["sliding_attention"])))
    if in_use:
        max_pos = min(max_pos, int(window))
    return _dims_close(cfg, d, Hq, Hkv, ffn, max_pos, max_positions, 1e-6, qk_norm=mt in QK_NORM_MODEL_TYPES)


def head_dim_perm(hd: int) -> np.ndarray:
    """stored row i of a q / k head = original row perm[i]: the identity for 64; for 128 [0..31, 64..95, 32..63, 96..127], so
    that the rotary pair (c, c + hd / 2) is 32 rows apart."""
    if hd == 64:
        return np.arange(64)
    return np.concatenate([np.arange(0, 32), np.arange(64, 96), np.arange(32, 64), np.arange(96, 128)])


def qkv_row_perm(Hq: int, Hkv: int, hd: int) -> np.ndarray:
    """stored row i of qkv_w = row perm[i] of cat(q_proj, k_proj, v_proj): head_dim_perm inside every q and k head."""
    p = head_dim_perm(hd)
    rows = [h * hd + p for h in range(Hq + Hkv)] + [np.arange((Hq + Hkv) * hd, (Hq + 2 * Hkv) * hd)]
    return np.concatenate(rows)


def gate_up_row_perm(ffn: int) -> np.ndarray:
    """stored row i of gate_up_w = row perm[i] of cat(gate_proj, up_proj): row 64b + i = gate[32b + i], 64b + 32 + i = up[32b + i]."""
    b = np.arange(ffn // 32)[:, None] * 32 + np.arange(32)[None, :]
    return np.concatenate([b, ffn + b], axis=1).reshape(-1)


# What the *_device_layout of the families on the b2t_clm_llama_t descriptor share; `get` is reader's, `sd` the state dict.
def _trunk(sd: dict, get, dims: dict, inv_freq: np.ndarray, att: float = 1.0, head: str = "tied or untied") -> Dict[str, "object"]:
    """The layout's entries outside the layers: embed_tokens (rows padded to 256), lm_head, final_norm_w and the fp32 rope_cos /
    rope_sin (CPU) = rope_tables of inv_freq, times the attention factor `att` in fp32 where that is not 1.  head: "tied or
    untied" -- the embedding itself where dims say tied or the checkpoint has no lm_head.weight, else that tensor; "untied" --
    always lm_head.weight; "embedding" -- the embedding itself, an lm_head.weight that differs from it refused."""
    import torch
    V, d = dims["vocab"], dims["d_model"]
    emb = _pad_rows(get("model.embed_tokens.weight", (V, d)), _rup(V, ROWPAD))
    if head == "embedding":
        tied = True
        if "lm_head.weight" in sd and not torch.equal(get.raw("lm_head.weight").to(emb.dtype), emb[:V]):
            raise ValueError("lm_head.weight differs from model.embed_tokens.weight: an untied head is not supported")
    else:
        tied = head != "untied" and (dims.get("tied", False) or "lm_head.weight" not in sd)
    out = {"embed_tokens": emb, "lm_head": emb if tied else _pad_rows(get("lm_head.weight", (V, d)), _rup(V, ROWPAD)),
           "final_norm_w": get("model.norm.weight", (d,))}
    cos, sin = rope_tables(inv_freq, dims["max_pos"])
    if att != 1.0:
        cos, sin = cos * np.float32(att), sin * np.float32(att)
    out["rope_cos"], out["rope_sin"] = torch.from_numpy(cos), torch.from_numpy(sin)
    return out


def _qkv_widths(dims: dict, hd: int) -> Dict[str, int]:
    return {"q_proj": dims["n_heads"] * hd, "k_proj": dims["n_kv_heads"] * hd, "v_proj": dims["n_kv_heads"] * hd}


def _layer(get, p: str, dims: dict, hd: int, qperm=None, gperm=None, norms=("input_layernorm", "post_attention_layernorm"),
           fused: bool = False) -> Dict[str, "object"]:
    """One layer's norm1_w, norm2_w (the checkpoint's `norms`), qkv_w (q | k | v rows, or Phi-3's `fused` qkv_proj, under the
    row permutation qperm if there is one), o_w [d][Hq hd] and, with gperm = gate_up_row_perm (a layer with a dense MLP),
    gate_up_w (gate | up rows, or the fused gate_up_proj, under gperm) and down_w; matrix rows padded to 256.  The family puts
    its own entries around these."""
    import torch
    d, ffn = dims["d_model"], dims["ffn_dim"]
    widths = _qkv_widths(dims, hd)
    if fused:
        qkv = get(p + "self_attn.qkv_proj.weight", (sum(widths.values()), d))
    else:
        qkv = torch.cat([get(p + f"self_attn.{n}.weight", (w, d)) for n, w in widths.items()], 0)
    if qperm is not None:
        qkv = qkv[qperm].contiguous()
    L = {"norm1_w": get(p + norms[0] + ".weight", (d,)), "norm2_w": get(p + norms[1] + ".weight", (d,)),
         "qkv_w": _pad_rows(qkv, _rup(qkv.shape[0], ROWPAD)),
         "o_w": _pad_rows(get(p + "self_attn.o_proj.weight", (d, widths["q_proj"])), _rup(d, ROWPAD))}
    if gperm is not None:
        if fused:
            gate_up = get(p + "mlp.gate_up_proj.weight", (2 * ffn, d))
        else:
            gate_up = torch.cat([get(p + "mlp.gate_proj.weight", (ffn, d)), get(p + "mlp.up_proj.weight", (ffn, d))], 0)
        L["gate_up_w"] = _pad_rows(gate_up[gperm].contiguous(), _rup(2 * ffn, ROWPAD))
        L["down_w"] = _pad_rows(get(p + "mlp.down_proj.weight", (d, ffn)), _rup(d, ROWPAD))
    return L


def _put_layer(out: dict, i: int, L: dict, order: Optional[Tuple[str, ...]] = None) -> None:
    """Layer i's entries into the layout, in the family's field order (default: L's own)."""
    for f in order or L:
        out[f"layers.{i}.{f}"] = L[f]


def _refuse_biases(sd: dict, prefix: str, who: str, names: Optional[Sequence[str]] = None) -> None:
    """Refuses the first bias of a layer: any key behind `prefix` that ends in .bias, or those of `names` alone."""
    for n in (prefix + n for n in names) if names is not None else (n for n in sd if n.startswith(prefix) and n.endswith(".bias")):
        if n in sd:
            raise ValueError(f"{n}: {who} are not supported")


def _stack_padded(t, rows: int):
    """[E][rows](...) of an expert tensor [E][r](...), r <= rows: zeros behind every expert's own rows (mixtral_strides)."""
    out = t.new_zeros((t.shape[0], rows) + tuple(t.shape[2:]))
    out[:, :t.shape[1]] = t
    return out


def llama_device_layout(state: dict, dims: dict, inv_freq: np.ndarray, dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t from a Llama / Mistral / Qwen2 / Qwen3 state dict, on the device the state dict
    is on (the CPU for a checkpoint read from disk): fp16 embed_tokens, lm_head (the same tensor when tied), final_norm_w,
    layers.<i>.<field> (qkv_b absent when the model has no q / k / v biases), and the fp32 rope_cos / rope_sin tables (CPU).
    With dims["qk_norm"] (Qwen3) also layers.<i>.q_norm_w / k_norm_w, the [hd] weights of b2t_clm_qknorm_t, under
    head_dim_perm like the q and k rows they scale; q / k / v biases are then refused.
    dtype=torch.bfloat16 (clm_dtype's spellings) makes the weights bf16 in the same layout: a bf16 checkpoint's values are
    kept exactly, an fp32 or fp16 one is rounded to nearest even."""
    wdt = clm_dtype(dtype)
    sd = dict(state)
    return _llama_layout(sd, dims, inv_freq, wdt, reader(sd, wdt))


def _llama_layout(sd: dict, dims: dict, inv_freq: np.ndarray, wdt, get) -> Dict[str, "object"]:
    """llama_device_layout's body over the reader `get`: llama_fp8_device_layout hands it one that yields the packed matrices'
    codes, which take the same row permutations and the same padding."""
    import torch
    Hq, Hkv, hd = dims["n_heads"], dims["n_kv_heads"], dims["d_model"] // dims["n_heads"]
    out = _trunk(sd, get, dims, inv_freq)
    dev = out["embed_tokens"].device
    qperm = torch.from_numpy(qkv_row_perm(Hq, Hkv, hd)).to(dev)
    hperm = torch.from_numpy(head_dim_perm(hd)).to(dev)
    qk_norm = bool(dims.get("qk_norm", False))
    gperm = torch.from_numpy(gate_up_row_perm(dims["ffn_dim"])).to(dev)
    widths = _qkv_widths(dims, hd)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        _refuse_biases(sd, p, "biases other than q / k / v's",
                       ("self_attn.o_proj.bias", "mlp.gate_proj.bias", "mlp.up_proj.bias", "mlp.down_proj.bias"))
        L = _layer(get, p, dims, hd, qperm, gperm)
        if qk_norm:
            if any(p + f"self_attn.{n}.bias" in sd for n in widths):
                raise ValueError(f"{p}self_attn: q / k / v biases beside q / k norms are not supported")
            L["q_norm_w"] = get(p + "self_attn.q_norm.weight", (hd,))[hperm].contiguous()
            L["k_norm_w"] = get(p + "self_attn.k_norm.weight", (hd,))[hperm].contiguous()
        elif p + "self_attn.q_norm.weight" in sd or p + "self_attn.k_norm.weight" in sd:
            raise ValueError(f"{p}self_attn: q / k norm weights in a model that is not one of {QK_NORM_MODEL_TYPES}")
        if any(p + f"self_attn.{n}.bias" in sd for n in widths):
            zero = lambda w: torch.zeros(w, dtype=wdt, device=dev)
            L["qkv_b"] = torch.cat([get(p + f"self_attn.{n}.bias", (w,)) if p + f"self_attn.{n}.bias" in sd else zero(w)
                                    for n, w in widths.items()])[qperm].contiguous()
        _put_layer(out, i, L)
    return out


def load_config(model_dir: str) -> dict:
    with open(os.path.join(model_dir, "config.json")) as f:
        return json.load(f)


def load_llama_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the Llama-family checkpoint in model_dir; dtype as clm_dtype reads it."""
    return _load_arrays(FAMILIES["llama"], model_dir, max_positions, dtype)


class LlamaScorer(_Scorer):
    """A Llama-family decoder on the GPU in the b2t_clm_llama_t layout, with OptScorer's scoring surface: `score` runs
    b2t_clm_llama_score_f16 on packed ids, or, with share_prefixes, b2t_clm_llama_score_tree_f16 over the list's shared-prefix
    token tree (bit-identical to the flat call); after a call `last_stats` = {"tokens", "nodes": rows computed}.

    context_cache_tokens > 0 allocates a context cache of that many positions and makes `score` / `token_logprobs` take
    b2t_clm_llama_score_tree_cached_f16, with OptScorer's `use_cache` / `update_cache` / `cache_len` / `cache_ids` /
    `cache_reset` and `last_stats` = {"tokens", "nodes", "reused"}.  With grouped-query K / V a position costs n_layers * 4 *
    n_kv_heads * head_dim bytes: 128 KiB at the Llama-3-8B shape, 256 MiB for 2048.  The cache is GPU memory for kernels that
    have no CPU path, so on another device context_cache_tokens > 0 raises ValueError.

    dtype: None or "float16" computes in fp16; "bfloat16" computes in bf16, the format these families are published in
    (b2t_clm_llama_score_bf16 / b2t_clm_llama_score_tree_bf16: the same contract with bf16 roundings, no fp16 overflow or
    underflow of weights and activations, about ten times the rounding error).  The arrays must already have that dtype
    (llama_device_layout(..., dtype=...)); `self.dtype` is the torch dtype.  bfloat16 with a context cache is refused.

    Arrays that hold layers.<i>.q_norm_w / k_norm_w (a Qwen3 layout) make the scorer take the b2t_clm_qwen3_* entry points, which
    norm every q and k head in the QKV GEMM's epilogue, on all those paths; sizes and the cache are the Llama calls'."""

    _SIZES = "b2t_clm_llama_"
    _NO_CACHE = "use_cache=True on a scorer built without a context cache (context_cache_tokens)"
    _OWN_ARRAYS = ()      # suffixes of the arrays that _point copies itself (they are not in the compute dtype)

    # A family is a subclass with class data and two hooks.  The constructor runs, in this order: _describe (which raises the
    # family's KeyError before anything else happens); the dtype / cache and device refusals; the copy of the weights to the
    # device, each checked against the dtype; the b2t_clm_llama_t; _point; the cache's allocation, which sizes it through
    # _size_args.  Every ctypes array and struct a descriptor points at stays an attribute of the scorer.
    def __init__(self, dims: dict, arrays: Dict[str, "object"], device="cuda", share_prefixes: bool = False,
                 context_cache_tokens: int = 0, dtype=None):
        import torch
        import b2t_native as N
        self._describe(dims, arrays, dtype, context_cache_tokens)
        self.dtype = clm_dtype(dtype)
        self._suffix = "bf16" if self.dtype == torch.bfloat16 else "f16"
        llama_check_dtype_cache(self.dtype, context_cache_tokens)
        self.dims = dict(dims)
        self.device = torch.device(device)
        self.check_cache_device(self.device, context_cache_tokens)   # before the weights are copied
        self.share_prefixes = bool(share_prefixes)
        self.last_stats = None
        self.w = {k: v.to(self.device).contiguous() for k, v in arrays.items() if not k.endswith(self._OWN_ARRAYS)}
        if dims.get("tied", False) or arrays["lm_head"] is arrays["embed_tokens"]:
            self.w["lm_head"] = self.w["embed_tokens"]
        for k, v in self.w.items():
            want = torch.float32 if k.startswith("rope_") else self.dtype
            if v.dtype != want:
                raise ValueError(f"LlamaScorer: {k} is {v.dtype}, expected {want}")
        self._layers = (N.ClmLlamaLayer * max(1, dims["n_layers"]))()
        for i in range(dims["n_layers"]):
            for f in _LLAMA_LAYER_FIELDS:
                t = self.w.get(f"layers.{i}.{f}")
                setattr(self._layers[i], f, t.data_ptr() if t is not None else None)
        self.desc = N.ClmLlamaDesc(dims["n_layers"], dims["d_model"], dims["n_heads"], dims["n_kv_heads"], dims["ffn_dim"],
                                   dims["vocab"], dims["max_pos"], dims["rms_eps"], self.w["embed_tokens"].data_ptr(),
                                   self.w["lm_head"].data_ptr(), self.w["final_norm_w"].data_ptr(),
                                   self.w["rope_cos"].data_ptr(), self.w["rope_sin"].data_ptr(), self._layers)
        self._point(arrays)
        self._ws = None
        self._alloc_cache(context_cache_tokens if self._CONTEXT_CACHE else 0)

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        """The first hook, before anything is copied: refuses dims / arrays that are not the family's (KeyError), builds the
        family's descriptor from dims / dtype with its per-layer arrays still empty, and sets _family (the entry points are
        b2t_clm_<_family>_score_*), _qk (what they take between the model and the lists) and _size_args.
        Here: arrays that hold layers.<i>.q_norm_w / k_norm_w are Qwen3's, whose b2t_clm_qknorm_t list goes in front of the lists."""
        import b2t_native as N
        self._family, self._qk = "llama", ()
        if dims["n_layers"] > 0 and "layers.0.q_norm_w" in arrays:
            self._qkn = (N.ClmQkNorm * dims["n_layers"])()
            self._family, self._qk = "qwen3", (self._qkn,)

    def _point(self, arrays):
        """The second hook, once self.w holds the weights on the device: fills the family's per-layer pointers (and copies
        the arrays named by _OWN_ARRAYS into self.w)."""
        for i in range(len(getattr(self, "_qkn", ()))):
            self._qkn[i].q_norm_w = self.w[f"layers.{i}.q_norm_w"].data_ptr()
            self._qkn[i].k_norm_w = self.w[f"layers.{i}.k_norm_w"].data_ptr()

    @staticmethod
    def check_cache_device(device, context_cache_tokens) -> None:
        """Refuses context_cache_tokens > 0 on a device without GPU memory (the cached kernels have no CPU path)."""
        import torch
        if int(context_cache_tokens) > 0 and torch.device(device).type != "cuda":
            raise ValueError(f"LlamaScorer: the context cache (context_cache_tokens > 0) lives in GPU memory; device "
                             f"{torch.device(device)} has none")


# ---- the fine-grained FP8 spelling of a Llama-family checkpoint (HF FineGrainedFP8Config; Qwen3-*-FP8) ---------------------
LINEAR_WEIGHTS = ("dense", "fp8")   # build_scorer's linear_weights: expanded to the compute dtype, or kept as the checkpoint has them
# the four GEMMs of a layer and the checkpoint's linears behind each: a group is wholly packed or wholly plain
_FP8_GROUPS = (("qkv", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj")), ("o", ("self_attn.o_proj",)),
               ("gate_up", ("mlp.gate_proj", "mlp.up_proj")), ("down", ("mlp.down_proj",)))
_FP8_FIELDS = tuple(g + t for g, _ in _FP8_GROUPS for t in ("_q", "_s"))   # b2t_clm_llama_fp8_layer_t
FP8_ROWS = 32   # stored rows a scale row of the packed layout serves: the row permutations move rows in chunks of 32


def fp8_block(cfg: dict) -> Optional[Tuple[int, int]]:
    """The block [bn, bk] of a config.json whose quantization_config is the fine-grained FP8 spelling (quant_method "fp8", fmt
    absent or "e4m3", weight_block_size [bn, bk]); None for a checkpoint without a quantization_config, and for gpt-oss's own
    "mxfp4".  activation_scheme is ignored: this scorer quantises no activation.  Refused, by name and before any weight is
    read: every other quant_method, every other fmt, FP8 without weight_block_size (per-tensor or per-channel), a block whose
    rows are no multiple of 32 or whose columns no multiple of 64 (with the numbers), and FP8 for a model_type outside the
    Llama row of FAMILIES."""
    qc = cfg.get("quantization_config")
    if not qc:
        return None
    qm, mt = qc.get("quant_method"), cfg.get("model_type")
    if qm == "mxfp4" and mt == "gpt_oss":
        return None
    if qm != "fp8":
        raise ValueError(f"quantization_config: quant_method {qm!r} is not supported ('fp8' with weight_block_size for "
                         f"{', '.join(LLAMA_MODEL_TYPES)}; 'mxfp4' for gpt_oss)")
    fmt = qc.get("fmt")
    if fmt not in (None, "e4m3"):
        raise ValueError(f"quantization_config: fmt {fmt!r} is not supported (e4m3 only)")
    wbs = qc.get("weight_block_size")
    if not isinstance(wbs, (list, tuple)) or len(wbs) != 2:
        raise ValueError(f"quantization_config: weight_block_size {wbs!r} is not supported ([rows, columns]; per-tensor and "
                         f"per-channel FP8 are not built)")
    bn, bk = int(wbs[0]), int(wbs[1])
    if bn < 1 or bk < 1 or bn % FP8_ROWS or bk % 64:
        raise ValueError(f"quantization_config: weight_block_size [{bn}, {bk}] is not supported (rows a multiple of {FP8_ROWS}, the "
                         f"grain of the stored row order; columns a multiple of 64, the GEMM's k tile)")
    if mt not in LLAMA_MODEL_TYPES:
        raise ValueError(f"quantization_config: FP8 checkpoints are read for {', '.join(LLAMA_MODEL_TYPES)} only, not model_type {mt!r}")
    return bn, bk


def fp8_dequant(q, s, bn: int, bk: int, name: str = "fp8"):
    """fp32 [N][K] of e4m3fn codes q [N][K] (torch.float8_e4m3fn, or the same bytes as uint8) and fp32 scales s [N / bn][K / bk]:
    f32(q[n][k]) * s[n / bn][k / bk], one fp32 multiplication (round to nearest even, subnormals kept) of the exactly widened
    code -- HF's Fp8Dequantize rule.  The one host definition of the expansion: the caller casts the result."""
    import torch
    if q.dtype == torch.uint8:
        q = q.view(torch.float8_e4m3fn)
    if q.dtype != torch.float8_e4m3fn or q.dim() != 2:
        raise ValueError(f"{name}: codes {q.dtype} {tuple(q.shape)} must be a float8_e4m3fn matrix")
    N, K = q.shape
    if N % bn or K % bk:
        raise ValueError(f"{name}: shape {N} x {K} is not a multiple of the block [{bn}, {bk}]")
    if tuple(s.shape) != (N // bn, K // bk):
        raise ValueError(f"{name}: scales {tuple(s.shape)} do not go with codes {N} x {K} in blocks of [{bn}, {bk}] "
                         f"(expected {(N // bn, K // bk)})")
    return (q.float().reshape(N // bn, bn, K // bk, bk) * s.float()[:, None, :, None]).reshape(N, K)


def _fp8_groups(sd: dict, n_layers: int) -> Tuple[bool, ...]:
    """Which of a layer's four GEMMs (_FP8_GROUPS) the checkpoint holds packed: a linear is packed iff its weight_scale_inv is
    there.  Refused by tensor name: a group with only some of its linears packed, and a layer that differs from layer 0."""
    first = None
    for i in range(n_layers):
        p = f"model.layers.{i}."
        flags = []
        for _, names in _FP8_GROUPS:
            has = [p + n + ".weight_scale_inv" in sd for n in names]
            if any(has) and not all(has):
                lack = p + names[has.index(False)] + ".weight_scale_inv"
                raise ValueError(f"checkpoint lacks {lack} while {p + names[has.index(True)]} is packed: the linears of one GEMM "
                                 f"({' | '.join(names)}) are all FP8 or all plain")
            flags.append(all(has))
        if first is None:
            first = tuple(flags)
        elif tuple(flags) != first:
            g, on = [(ns[0], a) for (_, ns), a, b in zip(_FP8_GROUPS, flags, first) if a != b][0]
            raise ValueError(f"{p}{g} is {'FP8' if on else 'plain'} and model.layers.0.{g} is not: the layers of one checkpoint "
                             f"must agree")
    return first or (False,) * len(_FP8_GROUPS)


def _fp8_linear(sd: dict, name: str, bn: int, bk: int, wdt):
    """The packed linear `name` (.weight float8_e4m3fn [N][K], .weight_scale_inv fp32 [N / bn][K / bk]) expanded and cast:
    fp8_dequant(...).to(wdt).  Refused by tensor name: a weight that is not float8_e4m3fn, an N or K the block does not divide
    (with the numbers), scales of another shape, a NaN code (0x7F, 0xFF), a scale that is not finite, and a value that is not
    finite in wdt (448 s > 65504 in fp16)."""
    import torch
    q, s = sd[name + ".weight"].detach(), sd[name + ".weight_scale_inv"].detach()
    if q.dtype != torch.float8_e4m3fn:
        raise ValueError(f"{name}.weight is {q.dtype} beside a weight_scale_inv, expected torch.float8_e4m3fn")
    if ((q.view(torch.uint8) & 0x7F) == 0x7F).any():
        raise ValueError(f"{name}.weight: a NaN code (0x7F or 0xFF)")
    if not torch.isfinite(s.float()).all():
        raise ValueError(f"{name}.weight_scale_inv: a scale is not finite")
    w = fp8_dequant(q, s, bn, bk, name + ".weight").to(wdt)
    if not torch.isfinite(w).all():
        raise ValueError(f"{name}.weight / weight_scale_inv: a value is not finite in {wdt}")
    return w


def _fp8_names(sd: dict, n_layers: int, groups: Tuple[bool, ...]) -> List[str]:
    """The packed linears' names (without .weight), after refusing every other weight_scale_inv and every float8 tensor that
    has none: embedding, head, norms and biases stay 16-bit, as they are published."""
    import torch
    names = [f"model.layers.{i}.{n}" for i in range(n_layers) for (_, ns), on in zip(_FP8_GROUPS, groups) if on for n in ns]
    known = set(names)
    for k, v in sd.items():
        if k.endswith(".weight_scale_inv") and k[:-len(".weight_scale_inv")] not in known:
            raise ValueError(f"{k}: only the layers' q / k / v / o / gate / up / down projections may be FP8 (a packed head or "
                             f"embedding is not built)")
        if getattr(v, "dtype", None) in (torch.float8_e4m3fn, torch.float8_e5m2) and not (k.endswith(".weight") and k[:-len(".weight")] in known):
            raise ValueError(f"{k} is {v.dtype} without a weight_scale_inv beside it")
    return names


def fp8_dense_state(state: dict, dims: dict, block: Tuple[int, int], dtype=None) -> Dict[str, "object"]:
    """The plain state dict of an FP8 one: every packed linear's .weight replaced by fp8_dequant(...).to(dtype) and its
    .weight_scale_inv dropped, everything else as it is -- what llama_device_layout then reads as any other checkpoint."""
    wdt = clm_dtype(dtype)
    sd = dict(state)
    for name in _fp8_names(sd, dims["n_layers"], _fp8_groups(sd, dims["n_layers"])):
        sd[name + ".weight"] = _fp8_linear(sd, name, block[0], block[1], wdt)
        del sd[name + ".weight_scale_inv"]
    return sd


def llama_fp8_device_layout(state: dict, dims: dict, inv_freq: np.ndarray, dtype=None, block: Tuple[int, int] = (128, 128)) -> Dict[str, "object"]:
    """llama_device_layout for build_scorer(..., linear_weights="fp8"): every tensor but the four matrices of a layer is that
    layout's, made by the same code, and in place of qkv_w / o_w / gate_up_w / down_w the layers have the checkpoint's FP8 form
    as the kernels of csrc/causal_lm_llama_fp8.hip read it (b2t_clm_llama_fp8_layer_t), for a checkpoint in blocks of block =
    [bn, bk] (fp8_block): <g>_q uint8 [rows padded to 256][K], the e4m3fn codes under the row permutation and the zero padding of
    <g>_w, and <g>_s fp32 [rows padded / 32][K / bk], the scale of every 32 stored rows -- the checkpoint's block rows expanded to
    that grain, which qkv_row_perm and gate_up_row_perm respect because they move rows in chunks of 32 and bn is a multiple
    of 32.  Padding rows have code 0 and scale 0.  The bytes are permuted by row and padded, never expanded: one byte a weight
    and 4 / (32 bk) for the scales, here and on the device.  fp8_dequant(q, s, 32, bk).to(dtype) of these arrays is the <g>_w of
    llama_device_layout on fp8_dense_state(state) to the byte.
    Every refusal of the dense reading (_fp8_groups, _fp8_linear) is made here too, with the same message; a checkpoint that
    holds one of the four GEMMs plain is refused by that projection's name."""
    import torch
    wdt = clm_dtype(dtype)
    sd = dict(state)
    bn, bk = block
    groups = _fp8_groups(sd, dims["n_layers"])
    if not all(groups):
        plain = [f"model.layers.0.{ns[0]}" for (_, ns), on in zip(_FP8_GROUPS, groups) if not on]
        raise ValueError(f"linear_weights='fp8': the checkpoint lacks {plain[0]}.weight_scale_inv (the packed layout needs all four "
                         f"GEMMs of a layer in FP8; use linear_weights='dense')")
    names = _fp8_names(sd, dims["n_layers"], groups)
    for n in names:
        _fp8_linear(sd, n, bn, bk, wdt)   # the refusals alone, in the dense reading's order; the expansion is dropped
    packed = {n + ".weight" for n in names}
    plain = reader(sd, wdt)

    def shaped(name, t, shape):
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t.contiguous()

    def codes(name, shape, to=None):
        return shaped(name, plain.raw(name).view(torch.uint8), shape) if name in packed else plain(name, shape, to)
    codes.raw = plain.raw

    def scales(name, shape, to=None):   # a packed matrix's scale per row: [N][K / bk]
        if name not in packed:
            return plain(name, shape, to)
        return shaped(name, plain.raw(name + "_scale_inv").float().repeat_interleave(bn, 0), (shape[0], shape[1] // bk))
    out = _llama_layout(sd, dims, inv_freq, wdt, codes)
    Hq, Hkv, hd = dims["n_heads"], dims["n_kv_heads"], dims["d_model"] // dims["n_heads"]
    dev = out["embed_tokens"].device
    qperm = torch.from_numpy(qkv_row_perm(Hq, Hkv, hd)).to(dev)
    gperm = torch.from_numpy(gate_up_row_perm(dims["ffn_dim"])).to(dev)
    for i in range(dims["n_layers"]):
        S = _layer(scales, f"model.layers.{i}.", dims, hd, qperm, gperm)
        for g, _ in _FP8_GROUPS:
            rows = S[g + "_w"]
            s = rows[::FP8_ROWS].contiguous()
            if not torch.equal(s.repeat_interleave(FP8_ROWS, 0), rows):
                raise ValueError(f"layers.{i}.{g}: 32 consecutive stored rows do not share one scale (block rows {bn})")
            out[f"layers.{i}.{g}_q"] = out.pop(f"layers.{i}.{g}_w")
            out[f"layers.{i}.{g}_s"] = s
    return out


class Fp8LlamaScorer(LlamaScorer):
    """A LlamaScorer that keeps the four projections of every layer in block-scaled FP8 on the device (build_scorer(...,
    linear_weights="fp8"), for a Llama / Mistral / Qwen2 / Qwen3 checkpoint in the fine-grained FP8 spelling): `w` holds
    llama_fp8_device_layout's layers.<i>.{qkv,o,gate_up,down}_q (uint8 codes) and _s (fp32 scales) and no qkv_w / o_w / gate_up_w /
    down_w (the model descriptor's are NULL); the calls are b2t_clm_llama_fp8_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 /
    _tree_bf16 (csrc/causal_lm_llama_fp8.hip) with the q / k norm array (Qwen3) or NULL and the b2t_clm_llama_fp8_t of those
    tensors, which unpack in the tile GEMM.  Activations are never quantised.  Scores, token log-probs and last_stats are the
    LlamaScorer's of the same checkpoint to the byte; workspace, context cache and their size functions are the same."""

    _OWN_ARRAYS = tuple("." + f for f in _FP8_FIELDS)

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import b2t_native as N
        super()._describe(dims, arrays, dtype, context_cache_tokens)
        n = dims["n_layers"]
        if n > 0 and ("layers.0.qkv_q" not in arrays or "layers.0.qkv_w" in arrays):
            raise KeyError("Fp8LlamaScorer: the arrays lack layers.<i>.qkv_q / qkv_s / ... / down_s or hold qkv_w beside them "
                           "(llama_fp8_device_layout makes them)")
        ks = {"qkv": dims["d_model"], "o": dims["d_model"], "gate_up": dims["d_model"], "down": dims["ffn_dim"]}
        bks = {K // arrays[f"layers.0.{g}_s"].shape[1] for g, K in ks.items()} if n > 0 else {128}
        if len(bks) != 1:
            raise ValueError(f"Fp8LlamaScorer: the scale arrays disagree on the block's columns ({sorted(bks)})")
        self.block_k = bks.pop()
        self._fp8_layers = (N.ClmLlamaFp8Layer * max(1, n))()
        self._fp8 = N.ClmLlamaFp8(self.block_k, self._fp8_layers)
        qkn = self._qk[0] if self._qk else None   # Qwen3's array, or NULL
        self._family, self._qk = "llama_fp8", (qkn, self._fp8)

    def _point(self, arrays):
        import torch
        super()._point(arrays)
        for k, v in arrays.items():
            if k.endswith(self._OWN_ARRAYS):
                want = torch.uint8 if k.endswith("_q") else torch.float32
                if v.dtype != want:
                    raise ValueError(f"Fp8LlamaScorer: {k} is {v.dtype}, expected {want}")
                self.w[k] = v.to(self.device).contiguous()
        for i in range(self.dims["n_layers"]):
            for f in _FP8_FIELDS:
                setattr(self._fp8_layers[i], f, self.w[f"layers.{i}.{f}"].data_ptr())

    def weight_bytes(self) -> int:
        """bytes of the packed projections held: per layer the sum over the four GEMMs of rows_padded K + 4 (rows_padded / 32)
        (K / block_k)"""
        return sum(v.numel() * v.element_size() for k, v in self.w.items() if k.endswith(self._OWN_ARRAYS))


# ---- OLMo-2 (HF Olmo2ForCausalLM): whole-row q / k norms and a post-norm layer ---------------------------------------------
OLMO2_HEAD_DIMS = (64, 128)
_OLMO2_ORDER = ("norm1_w", "norm2_w", "qkv_w", "q_norm_w", "k_norm_w", "o_w", "gate_up_w", "down_w")   # the layout's per layer


def olmo2_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t needs for an "olmo2" config, after refusing, by the field's name, what the kernels do not
    run.  max_pos is max_position_embeddings lowered to max_positions (default LLAMA_MAX_POSITIONS), which sizes the rotary
    table.  "olmo" (no q / k norm, a LayerNorm without weights) and "olmo3" (sliding-window layers) are other forwards."""
    _, d, Hq, Hkv = _dims_open(cfg, ("olmo2",))
    if d % Hq or d // Hq not in OLMO2_HEAD_DIMS or int(cfg.get("head_dim") or d // Hq) != d // Hq:
        raise ValueError(f"head dim {cfg.get('head_dim') or d}/{Hq} is not supported (hidden_size / num_attention_heads, one of "
                         f"{OLMO2_HEAD_DIMS})")
    if cfg.get("attention_bias"):
        raise ValueError("olmo2 with attention_bias=True is not supported (the QKV GEMM's fp32 epilogue adds no bias)")
    _check_gqa(Hq, Hkv)
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn)
    rope_inv_freq(cfg)   # refuses a rope_type other than default / llama3
    return _dims_close(cfg, d, Hq, Hkv, ffn, int(cfg["max_position_embeddings"]), max_positions, 1e-5)


def olmo2_device_layout(state: dict, dims: dict, inv_freq: np.ndarray, dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t / b2t_clm_qknorm_t from an OLMo-2 state dict, as llama_device_layout makes them,
    with the family's differences: norm1_w / norm2_w are post_attention_layernorm / post_feedforward_layernorm; the q and k rows
    of qkv_w and the norm weights q_norm_w [Hq * hd] / k_norm_w [Hkv * hd] stay in checkpoint order (the rotation runs in a
    kernel that sees whole heads, so there is no head_dim_perm); gate / up rows are interleaved as for Llama; any bias is
    refused."""
    import torch
    sd = dict(state)
    Hq, Hkv, hd = dims["n_heads"], dims["n_kv_heads"], dims["d_model"] // dims["n_heads"]
    get = reader(sd, clm_dtype(dtype))
    out = _trunk(sd, get, dims, inv_freq)
    gperm = torch.from_numpy(gate_up_row_perm(dims["ffn_dim"])).to(out["embed_tokens"].device)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        _refuse_biases(sd, p, "OLMo-2 biases", [n + ".bias" for n in (
            "self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
            "mlp.down_proj")])
        L = _layer(get, p, dims, hd, None, gperm, norms=("post_attention_layernorm", "post_feedforward_layernorm"))
        L["q_norm_w"] = get(p + "self_attn.q_norm.weight", (Hq * hd,))
        L["k_norm_w"] = get(p + "self_attn.k_norm.weight", (Hkv * hd,))
        _put_layer(out, i, L, _OLMO2_ORDER)
    return out


def load_olmo2_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the OLMo-2 checkpoint in model_dir; dtype as clm_dtype reads it."""
    return _load_arrays(FAMILIES["olmo2"], model_dir, max_positions, dtype)


class Olmo2Scorer(LlamaScorer):
    """An OLMo-2 decoder on the GPU: a LlamaScorer (same descriptor, scoring surface, context cache in fp16 and dtype rules) whose
    calls are b2t_clm_olmo2_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_olmo2.hip) with the
    per-layer q / k norm weights of olmo2_device_layout, and whose workspace sizes are the b2t_clm_olmo2_* size functions'
    (the Llama workspace plus an fp32 region for the rows the two norms read)."""

    _SIZES = "b2t_clm_olmo2_"

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        if dims["n_layers"] > 0 and "layers.0.q_norm_w" not in arrays:
            raise KeyError("Olmo2Scorer: the arrays lack layers.<i>.q_norm_w / k_norm_w (olmo2_device_layout makes them)")
        super()._describe(dims, arrays, dtype, context_cache_tokens)   # the norm weights' list, which _point fills
        self._family = "olmo2"
        if not self._qk:     # no layers: the calls still take the array argument
            self._qk = (None,)


# ---- Mixtral (HF MixtralForCausalLM): the Llama layer with routed experts in the dense MLP's place ---------------------------
MIXTRAL_MAX_EXPERTS, MIXTRAL_MAX_TOP_K = 64, 8


def mixtral_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t and b2t_clm_moe_t need for a "mixtral" config, after refusing, by the field's name, what the
    kernels do not run.  max_pos is max_position_embeddings lowered to the sliding window where one is configured (as for
    Mistral: within it full causal attention is what the model computes) and to max_positions (default LLAMA_MAX_POSITIONS)."""
    _, d, Hq, Hkv = _dims_open(cfg, ("mixtral",))
    if d % Hq or int(cfg.get("head_dim") or d // Hq) != d // Hq:
        raise ValueError(f"head_dim {cfg.get('head_dim')} is not hidden_size / num_attention_heads = {d}/{Hq}")
    if d // Hq not in LLAMA_HEAD_DIMS:
        raise ValueError(f"head_dim {d // Hq} is not supported (one of {LLAMA_HEAD_DIMS})")
    _check_gqa(Hq, Hkv)
    ne, k = int(cfg.get("num_local_experts", 8)), int(cfg.get("num_experts_per_tok", 2))
    _check_moe(ne, k, MIXTRAL_MAX_EXPERTS, MIXTRAL_MAX_TOP_K)
    for f in ("attention_bias", "mlp_bias"):
        if cfg.get(f):
            raise ValueError(f"mixtral with {f}=True is not supported (no bias anywhere)")
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn)
    rope_inv_freq(cfg)   # refuses a rope_type other than default / llama3
    max_pos = int(cfg["max_position_embeddings"])
    if cfg.get("sliding_window") is not None:
        max_pos = min(max_pos, int(cfg["sliding_window"]))
    return _dims_close(cfg, d, Hq, Hkv, ffn, max_pos, max_positions, 1e-5, n_experts=ne, top_k=k)


def mixtral_device_layout(state: dict, dims: dict, inv_freq: np.ndarray, dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t / b2t_clm_moe_t from a Mixtral state dict.  Embedding, head, norms, qkv_w (under
    qkv_row_perm), o_w and the rotary tables are llama_device_layout's; per layer also router_w [E][d], gate_up_w
    [E][round_up(2F, 256)][d] -- every expert's gate (w1) and up (w3) rows interleaved in blocks of 32 (gate_up_row_perm) and
    zero-padded, so the expert stride is dims-only: mixtral_strides -- and down_w [E][round_up(d, 256)][F] (w2).  Both spellings
    of a checkpoint are read: the published one (block_sparse_moe.gate.weight, block_sparse_moe.experts.<e>.w1 / w3 / w2.weight)
    and the fused one (mlp.gate.weight, mlp.experts.gate_up_proj [E][2F][d] with gate rows then up rows, mlp.experts.down_proj
    [E][d][F]).  Any bias in a layer is refused."""
    import torch
    sd = dict(state)
    d, ffn, Hq, Hkv = dims["d_model"], dims["ffn_dim"], dims["n_heads"], dims["n_kv_heads"]
    ne, hd = dims["n_experts"], dims["d_model"] // dims["n_heads"]
    get = reader(sd, clm_dtype(dtype))
    out = _trunk(sd, get, dims, inv_freq)
    dev = out["embed_tokens"].device
    qperm = torch.from_numpy(qkv_row_perm(Hq, Hkv, hd)).to(dev)
    gperm = torch.from_numpy(gate_up_row_perm(ffn)).to(dev)
    gus, dns = mixtral_strides(dims)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        _refuse_biases(sd, p, "Mixtral biases")
        L = _layer(get, p, dims, hd, qperm)
        if p + "mlp.experts.gate_up_proj" in sd:     # the fused spelling
            router = get(p + "mlp.gate.weight", (ne, d))
            gate_up = get(p + "mlp.experts.gate_up_proj", (ne, 2 * ffn, d))
            down = get(p + "mlp.experts.down_proj", (ne, d, ffn))
        else:                                        # the published spelling
            m = p + "block_sparse_moe."
            router = get(m + "gate.weight", (ne, d))
            gate_up = torch.stack([torch.cat([get(m + f"experts.{e}.w1.weight", (ffn, d)), get(m + f"experts.{e}.w3.weight", (ffn, d))], 0)
                                   for e in range(ne)])
            down = torch.stack([get(m + f"experts.{e}.w2.weight", (d, ffn)) for e in range(ne)])
        L.update(router_w=router, gate_up_w=_stack_padded(gate_up[:, gperm], gus), down_w=_stack_padded(down, dns))
        _put_layer(out, i, L)
    return out


def mixtral_strides(dims: dict) -> Tuple[int, int]:
    """Rows from one expert to the next in gate_up_w and in down_w: round_up(2F, 256) and round_up(d, 256)."""
    return _rup(2 * dims["ffn_dim"], ROWPAD), _rup(dims["d_model"], ROWPAD)


def load_mixtral_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the Mixtral checkpoint in model_dir; dtype as clm_dtype reads it."""
    return _load_arrays(FAMILIES["mixtral"], model_dir, max_positions, dtype)


class MixtralScorer(LlamaScorer):
    """A Mixtral decoder on the GPU: a LlamaScorer (same descriptor with the experts stacked in gate_up_w / down_w, scoring
    surface, context cache in fp16 and dtype rules) whose calls are b2t_clm_mixtral_score_f16 / _tree_f16 / _tree_cached_f16 /
    _bf16 / _tree_bf16 (csrc/causal_lm_mixtral.hip) with the b2t_clm_moe_t of mixtral_device_layout's arrays, and whose
    workspace sizes are the b2t_clm_mixtral_* size functions' (the Llama workspace plus the routing and the sorted rows); the
    cache's size is the Llama family's."""

    _SIZES = "b2t_clm_mixtral_"
    _CACHE_SIZES = "b2t_clm_llama_"

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import ctypes as C
        import b2t_native as N
        if "n_experts" not in dims or (dims["n_layers"] > 0 and "layers.0.router_w" not in arrays):
            raise KeyError("MixtralScorer: dims lack n_experts / top_k or the arrays layers.<i>.router_w (mixtral_dims and "
                           "mixtral_device_layout make them)")
        self._routers = (C.c_void_p * max(1, dims["n_layers"]))()
        gus, dns = mixtral_strides(dims)
        self._moe = N.ClmMoe(dims["n_experts"], dims["top_k"], self._routers, gus, dns, None)
        self._size_args = (self._moe,)
        self._family, self._qk = "mixtral", (self._moe,)

    def _point(self, arrays):
        for i in range(self.dims["n_layers"]):
            self._routers[i] = self.w[f"layers.{i}.router_w"].data_ptr()


# ---- Gemma-2 (HF Gemma2ForCausalLM): a head dim of its own, soft caps, four norms per layer, GeGLU ---------------------------
GEMMA2_HEAD_DIMS = (128, 256)
_GEMMA2_LAYER_FIELDS = ("pre_ffn_norm_w", "post_ffn_norm_w")
_GEMMA2_ORDER = ("norm1_w", "norm2_w") + _GEMMA2_LAYER_FIELDS + ("qkv_w", "o_w", "gate_up_w", "down_w")   # the layout's per layer


def gemma2_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t and b2t_clm_gemma2_t need for a "gemma2" config, after refusing, by the field's name, what
    the kernels do not run.  head_dim is a field of its own (num_attention_heads * head_dim != hidden_size in gemma-2-2b, 9b and
    27b).  max_pos is max_position_embeddings lowered to sliding_window -- within the window a sliding layer computes what a full
    one does, as for Mistral -- and to max_positions (default LLAMA_MAX_POSITIONS), which sizes the rotary table.  A cap of None
    in the config means off (0).  "gemma" and "gemma3" are other forwards."""
    _, d, Hq, Hkv = _dims_open(cfg, ("gemma2",), "hidden_activation", "gelu_pytorch_tanh")
    if cfg.get("attention_bias"):
        raise ValueError("gemma2 with attention_bias=True is not supported (no bias anywhere)")
    if cfg.get("use_bidirectional_attention"):
        raise ValueError("gemma2 with use_bidirectional_attention=True is not supported (causal attention only)")
    if not cfg.get("tie_word_embeddings", True):
        raise ValueError("gemma2 with tie_word_embeddings=False is not supported (the head is the embedding)")
    kind = _rope_parameters(cfg)["rope_type"]
    if kind != "default":
        raise ValueError(f"gemma2 rope_type {kind!r} is not supported (default only)")
    hd = int(cfg.get("head_dim") or 256)
    if hd not in GEMMA2_HEAD_DIMS:
        raise ValueError(f"head_dim {hd} is not supported (one of {GEMMA2_HEAD_DIMS})")
    _check_gqa(Hq, Hkv)
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn, {"num_attention_heads * head_dim": Hq * hd})
    rope_inv_freq(cfg)   # refuses partial rotary embeddings
    caps = {}
    for f in ("attn_logit_softcapping", "final_logit_softcapping"):
        c = cfg.get(f)
        caps[f] = 0.0 if c is None else float(c)
        if not caps[f] >= 0.0:
            raise ValueError(f"{f} {c!r} must be >= 0 or None")
    qpas = float(cfg.get("query_pre_attn_scalar") or 256)
    if not qpas > 0:
        raise ValueError(f"query_pre_attn_scalar {qpas} must be > 0")
    max_pos = int(cfg["max_position_embeddings"])
    if cfg.get("sliding_window") is not None:
        max_pos = min(max_pos, int(cfg["sliding_window"]))
    return _dims_close(cfg, d, Hq, Hkv, ffn, max_pos, max_positions, 1e-6, tied=True, head_dim=hd, q_scale=qpas ** -0.5,
                       attn_cap=caps["attn_logit_softcapping"], final_cap=caps["final_logit_softcapping"])


def gemma2_head_perm(hd: int) -> np.ndarray:
    """stored row i of a q / k head = original row perm[i]: stored 32-row block 2j holds dims [32j, 32j + 32) and block 2j + 1
    dims [hd / 2 + 32j, hd / 2 + 32j + 32), so that the rotary pair (c, c + hd / 2) is 32 rows apart inside one 64-row slice.  At
    128 this is head_dim_perm's order."""
    j = np.arange(hd // 64)[:, None] * 32 + np.arange(32)[None, :]
    return np.concatenate([j, hd // 2 + j], axis=1).reshape(-1)


def gemma2_embed_scale(d_model: int, dtype=None) -> float:
    """sqrt(hidden_size) rounded once to the compute dtype, as HF's scaled embedding does in that dtype."""
    import torch
    return float(torch.tensor(float(d_model) ** 0.5, dtype=torch.float32).to(clm_dtype(dtype)).float())


def gemma2_device_layout(state: dict, dims: dict, inv_freq: np.ndarray, dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t / b2t_clm_gemma2_t from a Gemma-2 state dict, as llama_device_layout makes them,
    with the family's differences: the head dim is dims["head_dim"], so qkv_w is [(Hq + 2 Hkv) hd][d] (q and k heads under
    gemma2_head_perm) and o_w [d][Hq hd]; norm1_w / norm2_w are input_layernorm / post_attention_layernorm and pre_ffn_norm_w /
    post_ffn_norm_w the two feed-forward norms, all as the checkpoint stores them (the kernels add the 1); gate / up rows are
    interleaved as for Llama; the head is the embedding; any bias and an lm_head of its own are refused."""
    import torch
    sd = dict(state)
    d, Hq, Hkv, hd = (dims[k] for k in ("d_model", "n_heads", "n_kv_heads", "head_dim"))
    get = reader(sd, clm_dtype(dtype))
    out = _trunk(sd, get, dims, inv_freq, head="embedding")
    dev = out["embed_tokens"].device
    hp = gemma2_head_perm(hd)
    qperm = torch.from_numpy(np.concatenate([h * hd + hp for h in range(Hq + Hkv)] +
                                            [np.arange((Hq + Hkv) * hd, (Hq + 2 * Hkv) * hd)])).to(dev)
    gperm = torch.from_numpy(gate_up_row_perm(dims["ffn_dim"])).to(dev)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        _refuse_biases(sd, p, "Gemma-2 biases")
        L = _layer(get, p, dims, hd, qperm, gperm)
        L["pre_ffn_norm_w"] = get(p + "pre_feedforward_layernorm.weight", (d,))
        L["post_ffn_norm_w"] = get(p + "post_feedforward_layernorm.weight", (d,))
        _put_layer(out, i, L, _GEMMA2_ORDER)
    return out


def load_gemma2_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the Gemma-2 checkpoint in model_dir; dtype as clm_dtype reads it."""
    return _load_arrays(FAMILIES["gemma2"], model_dir, max_positions, dtype)


class Gemma2Scorer(LlamaScorer):
    """A Gemma-2 decoder on the GPU: a LlamaScorer (same descriptor, scoring surface, context cache in fp16 and dtype rules)
    whose calls are b2t_clm_gemma2_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_gemma2.hip) with
    the b2t_clm_gemma2_t of gemma2_dims / gemma2_device_layout (head dim, q scale, the two caps, the embedding scale in the
    compute dtype, the two feed-forward norms per layer), and whose sizes, the cache's included, are the b2t_clm_gemma2_* size
    functions'."""

    _SIZES = "b2t_clm_gemma2_"

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import b2t_native as N
        if "head_dim" not in dims or (dims["n_layers"] > 0 and "layers.0.pre_ffn_norm_w" not in arrays):
            raise KeyError("Gemma2Scorer: dims lack head_dim or the arrays layers.<i>.pre_ffn_norm_w / post_ffn_norm_w (gemma2_dims "
                           "and gemma2_device_layout make them)")
        self._g2_layers = (N.ClmGemma2Layer * max(1, dims["n_layers"]))()
        self._g2 = N.ClmGemma2(dims["head_dim"], dims["q_scale"], dims["attn_cap"], dims["final_cap"],
                               gemma2_embed_scale(dims["d_model"], dtype), self._g2_layers)
        self._size_args = (self._g2,)
        self._family, self._qk = "gemma2", (self._g2,)

    def _point(self, arrays):
        for i in range(self.dims["n_layers"]):
            for f in _GEMMA2_LAYER_FIELDS:
                setattr(self._g2_layers[i], f, self.w[f"layers.{i}.{f}"].data_ptr())


# ---- Phi-3 (HF Phi3ForCausalLM): head dim 96, partial rotary, LongRoPE, fused qkv_proj / gate_up_proj ------------------------
PHI3_HEAD_DIMS = (64, 96, 128)


def _phi3_rope_parameters(cfg: dict) -> dict:
    """_rope_parameters with Phi-3's older spellings folded in: type "su" is "longrope", and partial_rotary_factor /
    original_max_position_embeddings may stand at the config's top level."""
    rp = _rope_parameters(cfg)
    if rp["rope_type"] == "su":
        rp["rope_type"] = "longrope"
    for f in ("partial_rotary_factor", "original_max_position_embeddings"):
        if rp.get(f) is None and cfg.get(f) is not None:
            rp[f] = cfg[f]
    return rp


def _phi3_head_rot(cfg: dict) -> Tuple[int, int]:
    """(head dim, rotary dims = int(head_dim * partial_rotary_factor), as HF computes them) of a phi3 config"""
    hd = int(cfg.get("head_dim") or int(cfg["hidden_size"]) // int(cfg["num_attention_heads"]))
    return hd, int(hd * float(_phi3_rope_parameters(cfg).get("partial_rotary_factor") or 1.0))


def phi3_rope(cfg: dict) -> Tuple[np.ndarray, float]:
    """(fp32 inv_freq[rotary_dims / 2], attention factor) of a "phi3" config, computed as HF's ROPE_INIT_FUNCTIONS compute them
    (fp32 torch arithmetic, same operation order).  rope_type "default": 1 / base^(arange(0, rot, 2) / rot), factor 1.
    "longrope" (older spelling "su"): 1 / (short_factor * base^(...)), and the factor that HF multiplies cos and sin by,
    sqrt(1 + ln(f) / ln(original_max_position_embeddings)) for f = max_position_embeddings / original_max_position_embeddings
    > 1 (or rope's own "factor"), else 1, unless "attention_factor" is given.  The long factors are never used: phi3_dims keeps
    every sequence within original_max_position_embeddings.  Every other type is refused."""
    import math
    import torch
    rp = _phi3_rope_parameters(cfg)
    kind = rp["rope_type"]
    if kind not in ("default", "longrope"):
        raise ValueError(f"phi3 rope_type {kind!r} is not supported (default or longrope)")
    rot = _phi3_head_rot(cfg)[1]
    base = rp["rope_theta"]
    if kind == "default":
        inv = 1.0 / (base ** (torch.arange(0, rot, 2, dtype=torch.float) / rot))
        return inv.numpy().astype(np.float32), 1.0
    short = rp.get("short_factor")
    if short is None or len(short) != rot // 2:
        raise ValueError(f"short_factor has {0 if short is None else len(short)} entries, rotary dims {rot} need {rot // 2}")
    orig = int(rp.get("original_max_position_embeddings") or cfg["max_position_embeddings"])
    factor = rp.get("factor")
    if factor is None:
        factor = int(cfg["max_position_embeddings"]) / orig
    af = rp.get("attention_factor")
    if af is None:
        af = 1.0 if factor <= 1.0 else math.sqrt(1 + math.log(factor) / math.log(orig))
    ext = torch.tensor(short, dtype=torch.float32)
    shape = torch.arange(0, rot, 2, dtype=torch.int64).float() / rot
    return (1.0 / (ext * base ** shape)).numpy().astype(np.float32), float(af)


def phi3_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t and b2t_clm_phi3_t need for a "phi3" config, after refusing, by the field's name, what the
    kernels do not run.  max_pos is max_position_embeddings lowered to sliding_window where one is set (within it full causal
    attention is what the model computes), for a longrope model to original_max_position_embeddings, and to max_positions
    (default LLAMA_MAX_POSITIONS), which sizes the rotary table.  Within the original length HF uses short_factor for the whole
    sequence; beyond it HF switches the whole call to long_factor, so that a row's score would depend on the longest sequence of
    its batch: such lengths are refused like lengths beyond a sliding window.  "phi", "phimoe" and "phi3small" are other
    forwards."""
    _, d, Hq, Hkv = _dims_open(cfg, ("phi3",))
    if not cfg.get("head_dim") and d % Hq:
        raise ValueError(f"hidden_size {d} is not a multiple of num_attention_heads {Hq}")
    hd, rot = _phi3_head_rot(cfg)
    if hd not in PHI3_HEAD_DIMS:
        raise ValueError(f"head_dim {hd} (head_dim, or hidden_size / num_attention_heads) is not supported (one of {PHI3_HEAD_DIMS})")
    if rot < 2 or rot > hd or rot % 2:
        raise ValueError(f"partial_rotary_factor gives {rot} rotary dims of head_dim {hd}: not an even number in [2, {hd}]")
    _check_gqa(Hq, Hkv)
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn, {"num_attention_heads * head_dim": Hq * hd,
                       "(num_attention_heads + 2 num_key_value_heads) * head_dim": (Hq + 2 * Hkv) * hd})
    phi3_rope(cfg)   # refuses the rope types and factor lists the table does not describe
    rp = _phi3_rope_parameters(cfg)
    max_pos = int(cfg["max_position_embeddings"])
    if cfg.get("sliding_window") is not None:
        max_pos = min(max_pos, int(cfg["sliding_window"]))
    if rp["rope_type"] == "longrope" and rp.get("original_max_position_embeddings"):
        max_pos = min(max_pos, int(rp["original_max_position_embeddings"]))
    return _dims_close(cfg, d, Hq, Hkv, ffn, max_pos, max_positions, 1e-5, head_dim=hd, rotary_dims=rot)


def phi3_device_layout(state: dict, dims: dict, rope: Tuple[np.ndarray, float], dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t / b2t_clm_phi3_t from a Phi-3 state dict, as llama_device_layout makes them, with
    the family's differences: the head dim is dims["head_dim"]; qkv_w is the fused self_attn.qkv_proj.weight [(Hq + 2 Hkv) hd][d]
    as stored (q, k and v rows in checkpoint order: the rotation runs in a kernel that sees whole heads, so there is no
    head_dim_perm); o_w is [d][Hq hd]; gate_up_w is the fused mlp.gate_up_proj.weight (gate rows, then up rows) interleaved in
    blocks of 32 (gate_up_row_perm); rope_cos / rope_sin are [max_pos][rotary_dims / 2] = rope_tables of rope's inv_freq times
    its attention factor in fp32 (rope = phi3_rope(cfg)); any bias in a layer is refused; the head is tied or untied as for
    Llama."""
    import torch
    sd = dict(state)
    get = reader(sd, clm_dtype(dtype))
    inv_freq, att = rope
    if len(inv_freq) != dims["rotary_dims"] // 2:
        raise ValueError(f"inv_freq has {len(inv_freq)} entries, rotary_dims {dims['rotary_dims']} need {dims['rotary_dims'] // 2}")
    out = _trunk(sd, get, dims, inv_freq, att)
    gperm = torch.from_numpy(gate_up_row_perm(dims["ffn_dim"])).to(out["embed_tokens"].device)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        _refuse_biases(sd, p, "Phi-3 biases")
        _put_layer(out, i, _layer(get, p, dims, dims["head_dim"], None, gperm, fused=True))
    return out


def load_phi3_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None) -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the Phi-3 checkpoint in model_dir; dtype as clm_dtype reads it."""
    return _load_arrays(FAMILIES["phi3"], model_dir, max_positions, dtype)


class Phi3Scorer(LlamaScorer):
    """A Phi-3 decoder on the GPU: a LlamaScorer (same descriptor, scoring surface, context cache in fp16 and dtype rules) whose
    calls are b2t_clm_phi3_score_f16 / _tree_f16 / _tree_cached_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_phi3.hip) with the
    b2t_clm_phi3_t of phi3_dims (head dim, rotary dims), and whose sizes, the cache's included, are the b2t_clm_phi3_* size
    functions'."""

    _SIZES = "b2t_clm_phi3_"

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import b2t_native as N
        if "head_dim" not in dims or "rotary_dims" not in dims:
            raise KeyError("Phi3Scorer: dims lack head_dim / rotary_dims (phi3_dims makes them)")
        self._phi3 = N.ClmPhi3(dims["head_dim"], dims["rotary_dims"])
        self._size_args = (self._phi3,)
        self._family, self._qk = "phi3", (self._phi3,)   # b2t_clm_phi3_t points at nothing: no _point


# ---- gpt-oss (HF GptOssForCausalLM): attention sinks, a sliding window in the kernel, biased routed experts ------------------
GPTOSS_HEAD_DIM = 64
GPTOSS_MAX_EXPERTS, GPTOSS_MAX_TOP_K = 128, 8
GPTOSS_LAYER_TYPES = ("full_attention", "sliding_attention")
_GPTOSS_LAYER_FIELDS = ("sinks", "o_b", "router_w", "router_b", "gate_up_b", "down_b")
_GPTOSS_ORDER = ("norm1_w", "norm2_w", "qkv_w", "qkv_b", "o_w", "o_b", "sinks", "router_w", "router_b", "gate_up_w", "gate_up_b",
                 "down_w", "down_b")   # the layout's per layer
_FP4_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)   # e2m1
EXPERT_WEIGHTS = ("dense", "mxfp4")   # build_scorer's expert_weights: expanded to the compute dtype, or kept as the checkpoint has them
_GPTOSS_MX_FIELDS = ("gate_up_q", "gate_up_s", "down_q", "down_s")   # b2t_clm_gptoss_mx_t
_GPTOSS_MX_ORDER = tuple(g for f in _GPTOSS_ORDER for g in ({"gate_up_w": ("gate_up_q", "gate_up_s"), "down_w": ("down_q", "down_s")}.get(f, (f,))))


def _gptoss_layer_types(cfg: dict) -> list:
    """layer_types of a gpt_oss config; absent, HF's default: sliding, full, sliding, ..."""
    n = int(cfg["num_hidden_layers"])
    lt = cfg.get("layer_types")
    return ["sliding_attention" if (i + 1) % 2 else "full_attention" for i in range(n)] if lt is None else list(lt)


def gptoss_rope(cfg: dict) -> Tuple[np.ndarray, float]:
    """(fp32 inv_freq[head_dim / 2], attention factor) of a "gpt_oss" config, computed as HF's GptOssRotaryEmbedding computes
    them (fp32 torch arithmetic, same operation order).  rope_type "default": 1 / base^(arange(0, hd, 2) / hd), factor 1.  "yarn":
    HF's _compute_yarn_parameters -- the blend of the interpolated and the extrapolated frequencies over the correction range of
    beta_fast / beta_slow, whose bounds are not rounded to integers when "truncate" is false (the published checkpoints), and the
    factor that HF multiplies cos and sin by, 0.1 ln(factor) + 1 (or the ratio of the two mscale forms, or "attention_factor").
    Every other type is refused.  The default rope_theta is 150000 and absent rope parameters are the published yarn ones."""
    import math
    import torch
    rp = dict(cfg.get("rope_parameters") or cfg.get("rope_scaling") or
              {"rope_type": "yarn", "factor": 32.0, "beta_fast": 32.0, "beta_slow": 1.0, "truncate": False,
               "original_max_position_embeddings": 4096})
    if "rope_type" not in rp:
        rp["rope_type"] = rp.get("type", "default")
    if "rope_theta" not in rp:
        rp["rope_theta"] = cfg.get("rope_theta", 150000.0)
    kind = rp["rope_type"]
    if kind not in ("default", "yarn"):
        raise ValueError(f"gpt_oss rope_type {kind!r} is not supported (yarn or default)")
    dim = int(cfg.get("head_dim") or int(cfg["hidden_size"]) // int(cfg["num_attention_heads"]))
    base = rp["rope_theta"]
    if kind == "default":
        inv = 1.0 / (base ** (torch.arange(0, dim, 2, dtype=torch.float) / dim))
        return inv.numpy().astype(np.float32), 1.0
    orig = rp["original_max_position_embeddings"]
    factor = rp.get("factor")
    if factor is None:
        factor = int(cfg["max_position_embeddings"]) / orig
    mscale_of = lambda scale, m=1: 1.0 if scale <= 1 else 0.1 * m * math.log(scale) + 1.0
    af = rp.get("attention_factor")
    if af is None:
        ms, msa = rp.get("mscale"), rp.get("mscale_all_dim")
        af = float(mscale_of(factor, ms) / mscale_of(factor, msa)) if ms and msa else mscale_of(factor)
    beta_fast, beta_slow = rp.get("beta_fast") or 32, rp.get("beta_slow") or 1
    corr = lambda rot: (dim * math.log(orig / (rot * 2 * math.pi))) / (2 * math.log(base))
    low, high = corr(beta_fast), corr(beta_slow)
    if rp.get("truncate", True):
        low, high = math.floor(low), math.ceil(high)
    low, high = max(low, 0), min(high, dim - 1)
    if low == high:
        high += 0.001
    pos_freqs = base ** (torch.arange(0, dim, 2).to(dtype=torch.float) / dim)
    extra, inter = 1.0 / pos_freqs, 1.0 / (factor * pos_freqs)
    ramp = torch.clamp((torch.arange(dim // 2, dtype=torch.float32) - low) / (high - low), 0, 1)
    keep = 1 - ramp.to(dtype=torch.float)
    inv = inter * (1 - keep) + extra * keep
    return inv.numpy().astype(np.float32), float(af)


def gptoss_dims(cfg: dict, max_positions: Optional[int] = None) -> dict:
    """The dimensions b2t_clm_llama_t and b2t_clm_gptoss_t need for a "gpt_oss" config, after refusing, by the field's name, what
    the kernels do not run.  max_pos is max_position_embeddings lowered to max_positions (default LLAMA_MAX_POSITIONS), which
    sizes the rotary table; the sliding window does NOT lower it: it binds (128 keys on every other layer), so it is a
    per-layer argument of the attention kernel, dims["windows"] (0 = a full layer)."""
    _, d, Hq, Hkv = _dims_open(cfg, ("gpt_oss",), act_note=": the clamped (up + 1) * gate * sigmoid(1.702 gate)")
    hd = int(cfg.get("head_dim") or d // Hq)
    if hd != GPTOSS_HEAD_DIM:
        raise ValueError(f"head_dim {hd} is not supported ({GPTOSS_HEAD_DIM})")
    _check_gqa(Hq, Hkv)
    ne, k = int(cfg.get("num_local_experts", 128)), int(cfg.get("num_experts_per_tok", 4))
    _check_moe(ne, k, GPTOSS_MAX_EXPERTS, GPTOSS_MAX_TOP_K)
    ffn = int(cfg["intermediate_size"])
    _check_64(d, ffn)
    if not cfg.get("attention_bias", True):
        raise ValueError("gpt_oss with attention_bias=False is not supported (the forward adds the q / k / v / o biases)")
    n_layers = int(cfg["num_hidden_layers"])
    types = _gptoss_layer_types(cfg)
    if len(types) != n_layers:
        raise ValueError(f"layer_types has {len(types)} entries, num_hidden_layers is {n_layers}")
    for i, t in enumerate(types):
        if t not in GPTOSS_LAYER_TYPES:
            raise ValueError(f"layer_types[{i}] {t!r} is not one of {GPTOSS_LAYER_TYPES}")
    window = cfg.get("sliding_window")
    if "sliding_attention" in types and (window is None or int(window) < 1):
        raise ValueError(f"sliding_window {window} < 1 with sliding_attention layers")
    gptoss_rope(cfg)   # refuses a rope_type other than yarn / default
    if cfg.get("tie_word_embeddings", False):
        raise ValueError("gpt_oss with tie_word_embeddings=True is not supported (the head is untied)")
    limit = float(cfg.get("swiglu_limit", 7.0))
    if not limit > 0:
        raise ValueError(f"swiglu_limit {limit} must be > 0")
    return _dims_close(cfg, d, Hq, Hkv, ffn, int(cfg["max_position_embeddings"]), max_positions, 1e-5, tied=False, head_dim=hd,
                       n_experts=ne, top_k=k, swiglu_limit=limit,
                       windows=[int(window) if t == "sliding_attention" else 0 for t in types])


def mxfp4_dequant(blocks, scales, name: str = "mxfp4"):
    """fp32 [..., rows, 32 G] of MXFP4 blocks uint8 [..., rows, G, 16] (two e2m1 values per byte, low nibble first) and scales
    uint8 [..., rows, G]: value * 2^(scale - 127), exact in fp32 wherever the result is an fp32 number."""
    import torch
    if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
        raise ValueError(f"{name}: blocks {blocks.dtype} and scales {scales.dtype} must be uint8")
    if blocks.shape[-1] != 16 or tuple(blocks.shape[:-1]) != tuple(scales.shape):
        raise ValueError(f"{name}: blocks {tuple(blocks.shape)} do not go with scales {tuple(scales.shape)}")
    lut = torch.tensor(_FP4_VALUES, dtype=torch.float32, device=blocks.device)
    b = blocks.long()
    vals = torch.stack([lut[b & 15], lut[b >> 4]], -1).reshape(*blocks.shape[:-1], 32)      # low nibble first
    out = torch.ldexp(vals, (scales.to(torch.int32) - 127)[..., None])
    return out.reshape(*scales.shape[:-1], scales.shape[-1] * 32)


def mxfp4_block_finite(blocks, scales, wdt):
    """Per block (bool, the shape of scales): whether every value of the block is finite after mxfp4_dequant(...).to(wdt),
    decided from the block's largest nibble magnitude and its scale byte without expanding anything: the magnitudes are
    monotone in the 3-bit code, a value has at most two significant bits (so no rounding carries it over the dtype's largest
    number), and a scale byte of 255 is 0 * 2^128 = NaN at best."""
    import torch
    code = torch.maximum(blocks & 7, (blocks >> 4) & 7).amax(-1).long()                    # the largest magnitude's code, 0..7
    top = torch.ldexp(torch.tensor(_FP4_VALUES[:8], dtype=torch.float32, device=blocks.device)[code], scales.to(torch.int32) - 127)
    return (top <= torch.finfo(wdt).max) & (scales != 255)


def gptoss_device_layout(state: dict, dims: dict, rope: Tuple[np.ndarray, float], dtype=None) -> Dict[str, "object"]:
    """Tensors in the layout of b2t_clm_llama_t / b2t_clm_gptoss_t from a gpt-oss state dict.  Embedding, untied head, norms and the
    rotary tables ([max_pos][32], rope_tables of rope's inv_freq times its attention factor in fp32; rope = gptoss_rope(cfg)) are
    made as for Phi-3; qkv_w / qkv_b are q, k, v rows in checkpoint order (at head dim 64 the rotary pair (c, c + 32) is 32 rows
    apart as stored); o_w is [round_up(d, 256)][Hq hd].  Per layer also sinks (fp32 [Hq]; a non-finite one is refused by name),
    o_b, router_w [E][d], router_b [E], gate_up_w [E][round_up(2F, 256)][d], gate_up_b [E][round_up(2F, 256)], down_w
    [E][round_up(d, 256)][F] and down_b [E][round_up(d, 256)] (mixtral_strides), zero-padded.  Both spellings of a checkpoint are
    read: the plain one -- mlp.experts.gate_up_proj [E][d][2F] with gate in the even columns and up in the odd ones,
    gate_up_proj_bias [E][2F] interleaved the same way, down_proj [E][F][d], down_proj_bias [E][d] -- and the published MXFP4 one
    -- gate_up_proj_blocks / _scales [E][2F][d / 32]([16]) and down_proj_blocks / _scales [E][d][F / 32]([16]), dequantised to
    fp32 exactly (mxfp4_dequant) and then cast; a value that does not survive the cast as a finite number is refused by name.
    The expert matrices are transposed to [rows][K], and gate / up are de-interleaved into gate_up_row_perm's blocks of 32."""
    return _gptoss_layout(state, dims, rope, dtype, False)


def gptoss_mx_device_layout(state: dict, dims: dict, rope: Tuple[np.ndarray, float], dtype=None) -> Dict[str, "object"]:
    """gptoss_device_layout for build_scorer(..., expert_weights="mxfp4"): every tensor but the expert matrices is that layout's,
    made by the same code, and in place of gate_up_w / down_w the layers have the checkpoint's MXFP4 bytes as the kernels of
    csrc/causal_lm_gptoss_mx.hip read them (b2t_clm_gptoss_mx_t): gate_up_q uint8 [E][round_up(2F, 256)][d / 2] and gate_up_s
    uint8 [E][round_up(2F, 256)][d / 32], the blocks and scale bytes of gate_up_proj under the row order of gate_up_w
    (de-interleaved into gate_up_row_perm's blocks of 32), down_q [E][round_up(d, 256)][F / 2] and down_s [E][round_up(d,
    256)][F / 32]; the rows behind an expert's own are zero bytes, which unpack to zero.  The bytes are permuted by row and
    padded, never expanded: 4.25 bits a weight here and on the device.  mxfp4_dequant(q, s).to(dtype) of these arrays is
    gate_up_w / down_w of gptoss_device_layout to the byte.
    A checkpoint in the plain spelling is refused with the name of the first _blocks tensor it lacks, before anything else is
    read; a block with a value that is not finite in the compute dtype is refused as the dense loader refuses it (same
    message, same tensor), decided by mxfp4_block_finite."""
    return _gptoss_layout(state, dims, rope, dtype, True)


def _gptoss_layout(state: dict, dims: dict, rope, dtype, packed: bool) -> Dict[str, "object"]:
    """gptoss_device_layout (packed False) and gptoss_mx_device_layout (True)"""
    import torch
    wdt = clm_dtype(dtype)
    sd = dict(state)
    if packed:
        for i in range(dims["n_layers"]):
            for n in ("gate_up_proj", "down_proj"):
                name = f"model.layers.{i}.mlp.experts.{n}_blocks"
                if name not in sd:
                    raise ValueError(f"expert_weights='mxfp4': the checkpoint lacks {name} (its experts are not in the MXFP4 "
                                     f"spelling; quantising a plain checkpoint is not built: use expert_weights='dense')")
    d, ffn, Hq, hd, ne = (dims[k] for k in ("d_model", "ffn_dim", "n_heads", "head_dim", "n_experts"))
    inv_freq, att = rope
    if len(inv_freq) != hd // 2:
        raise ValueError(f"inv_freq has {len(inv_freq)} entries, head_dim {hd} needs {hd // 2}")
    get = reader(sd, wdt)
    raw = get.raw

    def expert_rows(name, rows, K):
        """[E][rows][K] in wdt of the expert matrix `name`, from either spelling; packed: (its blocks as [E][rows][K / 2], its
        scale bytes [E][rows][K / 32]), as stored"""
        if name + "_blocks" in sd:
            blocks, scales = raw(name + "_blocks"), raw(name + "_scales")
            if tuple(blocks.shape) != (ne, rows, K // 32, 16) or tuple(scales.shape) != (ne, rows, K // 32) or K % 32:
                raise ValueError(f"{name}_blocks / _scales: shapes {tuple(blocks.shape)} / {tuple(scales.shape)}, expected "
                                 f"{(ne, rows, K // 32, 16)} / {(ne, rows, K // 32)}")
            if packed:
                if blocks.dtype != torch.uint8 or scales.dtype != torch.uint8:
                    raise ValueError(f"{name}: blocks {blocks.dtype} and scales {scales.dtype} must be uint8")
                if not mxfp4_block_finite(blocks, scales, wdt).all():
                    raise ValueError(f"{name}_blocks / _scales: a value is not finite in {wdt}")
                return blocks.reshape(ne, rows, K // 2), scales
            t = mxfp4_dequant(blocks, scales, name).to(wdt)
            if not torch.isfinite(t).all():
                raise ValueError(f"{name}_blocks / _scales: a value is not finite in {wdt}")
            return t
        return get(name, (ne, K, rows)).transpose(1, 2).contiguous()
    out = _trunk(sd, get, dims, inv_freq, att, head="untied")
    dev = out["embed_tokens"].device
    gperm = torch.from_numpy(gate_up_row_perm(ffn)).to(dev)
    deint = torch.cat([torch.arange(0, 2 * ffn, 2), torch.arange(1, 2 * ffn, 2)]).to(dev)[gperm]   # stored row -> interleaved row
    gus, dns = mixtral_strides(dims)
    for i in range(dims["n_layers"]):
        p = f"model.layers.{i}."
        L = _layer(get, p, dims, hd)
        L["sinks"] = get(p + "self_attn.sinks", (Hq,), torch.float32)
        if not torch.isfinite(L["sinks"]).all():
            raise ValueError(f"{p}self_attn.sinks: a sink is not finite")
        gate_up = expert_rows(p + "mlp.experts.gate_up_proj", 2 * ffn, d)        # [E][2F][d], gate rows even, up rows odd
        down = expert_rows(p + "mlp.experts.down_proj", d, ffn)                  # [E][d][F]
        L.update(qkv_b=torch.cat([get(p + f"self_attn.{n}.bias", (w,)) for n, w in _qkv_widths(dims, hd).items()]),
                 o_b=get(p + "self_attn.o_proj.bias", (d,)),
                 router_w=get(p + "mlp.router.weight", (ne, d)), router_b=get(p + "mlp.router.bias", (ne,)),
                 gate_up_b=_stack_padded(get(p + "mlp.experts.gate_up_proj_bias", (ne, 2 * ffn))[:, deint], gus),
                 down_b=_stack_padded(get(p + "mlp.experts.down_proj_bias", (ne, d)), dns))
        if packed:
            L.update(gate_up_q=_stack_padded(gate_up[0][:, deint], gus), gate_up_s=_stack_padded(gate_up[1][:, deint], gus),
                     down_q=_stack_padded(down[0], dns), down_s=_stack_padded(down[1], dns))
        else:
            L.update(gate_up_w=_stack_padded(gate_up[:, deint], gus), down_w=_stack_padded(down, dns))
        _put_layer(out, i, L, _GPTOSS_MX_ORDER if packed else _GPTOSS_ORDER)
    return out


def load_gptoss_arrays(model_dir: str, max_positions: Optional[int] = None, dtype=None,
                       expert_weights: str = "dense") -> Tuple[dict, Dict[str, "object"]]:
    """(dims, host tensors in the device layout) of the gpt-oss checkpoint in model_dir; dtype as clm_dtype reads it;
    expert_weights="mxfp4": gptoss_mx_device_layout's."""
    return _load_arrays(_family_for(FAMILIES["gpt_oss"], expert_weights), model_dir, max_positions, dtype)


def gptoss_check_cache(context_cache_tokens) -> None:
    """Refuses a context cache for gpt-oss: the cached and trunk attention kernels have neither sink nor window."""
    if int(context_cache_tokens) > 0:
        raise ValueError("gpt_oss: the context cache (context_cache_tokens > 0) is not supported for this family: the cached "
                         "attention kernels have neither the sink nor the sliding window (a follow-up)")


class GptOssScorer(LlamaScorer):
    """A gpt-oss decoder on the GPU: a LlamaScorer (same descriptor with the experts stacked in gate_up_w / down_w, scoring surface
    and dtype rules) whose calls are b2t_clm_gptoss_score_f16 / _tree_f16 / _bf16 / _tree_bf16 (csrc/causal_lm_gptoss.hip) with the
    b2t_clm_gptoss_t of gptoss_device_layout's arrays, and whose workspace sizes are the b2t_clm_gptoss_* size functions'.  There
    is no context cache for this family: context_cache_tokens > 0 raises ValueError."""

    _SIZES = "b2t_clm_gptoss_"
    _CONTEXT_CACHE = False
    _OWN_ARRAYS = (".sinks",)   # fp32 in either compute dtype
    _PACKED = ()                # those of _OWN_ARRAYS that are uint8 (GptOssMxScorer)

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import b2t_native as N
        gptoss_check_cache(context_cache_tokens)
        if "windows" not in dims or (dims["n_layers"] > 0 and "layers.0.sinks" not in arrays):
            raise KeyError("GptOssScorer: dims lack windows / n_experts or the arrays layers.<i>.sinks (gptoss_dims and "
                           "gptoss_device_layout make them)")
        self._oss_layers = (N.ClmGptOssLayer * max(1, dims["n_layers"]))()
        gus, dns = mixtral_strides(dims)
        self._oss = N.ClmGptOss(dims["head_dim"], dims["swiglu_limit"], dims["n_experts"], dims["top_k"], gus, dns, None,
                                self._oss_layers)
        self._size_args = (self._oss,)
        self._family, self._qk = "gptoss", (self._oss,)

    def _point(self, arrays):
        import torch
        for k, v in arrays.items():
            if k.endswith(self._OWN_ARRAYS):
                want = torch.uint8 if k.endswith(self._PACKED) else torch.float32
                if v.dtype != want:
                    raise ValueError(f"GptOssScorer: {k} is {v.dtype}, expected {want}")
                self.w[k] = v.to(self.device).contiguous()
        for i in range(self.dims["n_layers"]):
            for f in _GPTOSS_LAYER_FIELDS:
                setattr(self._oss_layers[i], f, self.w[f"layers.{i}.{f}"].data_ptr())
            self._oss_layers[i].window = self.dims["windows"][i]


class GptOssMxScorer(GptOssScorer):
    """A GptOssScorer that keeps the experts in MXFP4 on the device (build_scorer(..., expert_weights="mxfp4")): `w` holds
    gptoss_mx_device_layout's uint8 layers.<i>.gate_up_q / gate_up_s / down_q / down_s, 4.25 bits a weight, and no gate_up_w /
    down_w (the model descriptor's are NULL); the calls are b2t_clm_gptoss_mx_score_f16 / _tree_f16 / _bf16 / _tree_bf16
    (csrc/causal_lm_gptoss_mx.hip) with the b2t_clm_gptoss_mx_t array of those tensors, which unpack in the grouped GEMM.  Scores,
    token log-probs and last_stats are the GptOssScorer's of the same checkpoint to the byte; the workspace is the same."""

    _OWN_ARRAYS = (".sinks",) + tuple("." + f for f in _GPTOSS_MX_FIELDS)
    _PACKED = tuple("." + f for f in _GPTOSS_MX_FIELDS)

    def _describe(self, dims, arrays, dtype, context_cache_tokens):
        import b2t_native as N
        super()._describe(dims, arrays, dtype, context_cache_tokens)
        if dims["n_layers"] > 0 and ("layers.0.gate_up_q" not in arrays or "layers.0.gate_up_w" in arrays):
            raise KeyError("GptOssMxScorer: the arrays lack layers.<i>.gate_up_q / gate_up_s / down_q / down_s or hold gate_up_w "
                           "beside them (gptoss_mx_device_layout makes them)")
        self._mx = (N.ClmGptOssMx * max(1, dims["n_layers"]))()
        self._family, self._qk = "gptoss_mx", (self._oss, self._mx)   # the size functions are the dense twins': _size_args stays

    def _point(self, arrays):
        super()._point(arrays)
        for i in range(self.dims["n_layers"]):
            for f in _GPTOSS_MX_FIELDS:
                setattr(self._mx[i], f, self.w[f"layers.{i}.{f}"].data_ptr())

    def expert_bytes(self) -> int:
        """bytes of the packed experts held: n_layers E (gate_up_stride (d / 2 + d / 32) + down_stride (F / 2 + F / 32))"""
        return sum(v.numel() for k, v in self.w.items() if k.endswith(self._PACKED))


def tree_plan(ids, seq_off, cap: Optional[int] = None):
    """b2t_clm_tree_plan_host on packed int32 ids / offsets (host only, no GPU): (node_of_token, parent_of_node, n_nodes).
    A node is a distinct token prefix, numbered by first appearance; parent_of_node is -1 at roots."""
    import ctypes as C
    import b2t_native as N
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(seq_off, np.int32)
    cap = len(ids) if cap is None else int(cap)
    node = np.empty(len(ids), np.int32)
    parent = np.empty(max(cap, 1), np.int32)
    n = C.c_longlong(0)
    N.check(N.load().b2t_clm_tree_plan_host(ids.ctypes.data, off.ctypes.data, len(off) - 1, node.ctypes.data, parent.ctypes.data,
                                            cap, C.byref(n)), "b2t_clm_tree_plan_host")
    return node, parent[:n.value], int(n.value)


def cache_plan(cache_ids, cap: int, ids, seq_off) -> dict:
    """b2t_clm_cache_plan_host (host only, no GPU): what a cached call on the packed list does against the cached chain
    cache_ids of capacity cap: {"trunk": Tn, "common": P, "reused": R, "nodes", "rows": nodes - R, "n_after": min(Tn, cap)}."""
    import ctypes as C
    import b2t_native as N
    cid = np.ascontiguousarray(cache_ids, np.int32)
    ids = np.ascontiguousarray(ids, np.int32)
    off = np.ascontiguousarray(seq_off, np.int32)
    tn, p, r, na = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    nn, nr = C.c_longlong(0), C.c_longlong(0)
    N.check(N.load().b2t_clm_cache_plan_host(cid.ctypes.data if len(cid) else None, len(cid), int(cap), ids.ctypes.data,
                                             off.ctypes.data, len(off) - 1, C.byref(tn), C.byref(p), C.byref(r), C.byref(nn),
                                             C.byref(nr), C.byref(na)), "b2t_clm_cache_plan_host")
    return {"trunk": tn.value, "common": p.value, "reused": r.value, "nodes": int(nn.value), "rows": int(nr.value),
            "n_after": na.value}


class Family(NamedTuple):
    """One row of FAMILIES: what build_scorer and the load_*_arrays need to know about a model family."""
    model_types: Tuple[str, ...]   # config.json's model_type values the family serves
    dims: Callable                 # config (and, for a LlamaScorer, max_positions) -> dims, refusing what the kernels do not run
    rope: Optional[Callable]       # config -> the layout's rotary argument (None: the layout takes none)
    layout: Callable               # state dict, dims (, rope (, dtype)) -> arrays
    scorer: type
    dtype: Callable                # the family's reading of the dtype argument: clm_dtype, or an fp16-only rule
    # whether the family has a context cache is the scorer's: scorer._CONTEXT_CACHE


_FAMILY_ROWS = (
    Family(("opt",), opt_dims, None, device_layout, OptScorer, opt_dtype),
    Family(("gpt2",), gpt2_dims, None, gpt2_device_layout, Gpt2Scorer, gpt2_dtype),
    Family(("gpt_neox",), neox_dims, neox_inv_freq, neox_device_layout, NeoxScorer, neox_dtype),
    Family(LLAMA_MODEL_TYPES, llama_dims, rope_inv_freq, llama_device_layout, LlamaScorer, clm_dtype),
    Family(("olmo2",), olmo2_dims, rope_inv_freq, olmo2_device_layout, Olmo2Scorer, clm_dtype),
    Family(("mixtral",), mixtral_dims, rope_inv_freq, mixtral_device_layout, MixtralScorer, clm_dtype),
    Family(("gemma2",), gemma2_dims, rope_inv_freq, gemma2_device_layout, Gemma2Scorer, clm_dtype),
    Family(("phi3",), phi3_dims, phi3_rope, phi3_device_layout, Phi3Scorer, clm_dtype),
    Family(("gpt_oss",), gptoss_dims, gptoss_rope, gptoss_device_layout, GptOssScorer, clm_dtype),
)
FAMILIES = {mt: fam for fam in _FAMILY_ROWS for mt in fam.model_types}   # by config.json's model_type


def _family_for(fam: Family, expert_weights: str, linear_weights: str = "dense", cfg: Optional[dict] = None) -> Family:
    """The family's row for build_scorer's expert_weights and linear_weights: itself for "dense"; for "mxfp4" gpt-oss with the
    packed layout and scorer, any other family refused; for "fp8" the Llama row with the packed layout and scorer, any other
    family and a checkpoint whose config.json (cfg) has no FP8 quantization_config refused.  Reads no weight."""
    if expert_weights not in EXPERT_WEIGHTS:
        raise ValueError(f"expert_weights {expert_weights!r} is not one of {EXPERT_WEIGHTS}")
    if linear_weights not in LINEAR_WEIGHTS:
        raise ValueError(f"linear_weights {linear_weights!r} is not one of {LINEAR_WEIGHTS}")
    if linear_weights == "fp8":
        if fam.scorer is not LlamaScorer:
            raise ValueError(f"linear_weights='fp8' is for {', '.join(LLAMA_MODEL_TYPES)} checkpoints in the fine-grained FP8 "
                             f"spelling; model_type {fam.model_types[0]!r} has no packed form")
        if expert_weights != "dense":
            raise ValueError(f"expert_weights={expert_weights!r} with linear_weights='fp8': model_type {fam.model_types[0]!r} has no experts")
        if fp8_block(cfg or {}) is None:
            raise ValueError("linear_weights='fp8': the checkpoint's config.json has no FP8 quantization_config (quantising a plain "
                             "checkpoint is not built: use linear_weights='dense')")
        return fam._replace(layout=llama_fp8_device_layout, scorer=Fp8LlamaScorer)
    if expert_weights == "dense":
        return fam
    if fam.scorer is not GptOssScorer:
        raise ValueError(f"expert_weights='mxfp4' is for gpt_oss checkpoints, whose experts are published in MXFP4; model_type "
                         f"{fam.model_types[0]!r} has none")
    return fam._replace(layout=gptoss_mx_device_layout, scorer=GptOssMxScorer)


def _load_arrays(fam: Family, model_dir: str, max_positions: Optional[int] = None, dtype=None):
    """(dims, host tensors in the device layout) of the family's checkpoint in model_dir: what every load_*_arrays returns."""
    cfg = load_config(model_dir)
    if not issubclass(fam.scorer, LlamaScorer):   # OPT, GPT-2, GPT-NeoX: fp16 alone, positions as the checkpoint has them
        dims = fam.dims(cfg)
        return dims, fam.layout(_load_state_dict(model_dir), dims, *([fam.rope(cfg)] if fam.rope else []))
    dims = fam.dims(cfg, max_positions)
    wdt = fam.dtype(dtype, cfg)
    block = fp8_block(cfg)   # the fine-grained FP8 spelling: kept packed, or expanded into the plain spelling first
    if fam.layout is llama_fp8_device_layout:
        return dims, fam.layout(_load_state_dict(model_dir), dims, fam.rope(cfg), wdt, block)
    sd = _load_state_dict(model_dir)
    if block is not None:
        sd = fp8_dense_state(sd, dims, block, wdt)
    return dims, fam.layout(sd, dims, fam.rope(cfg), wdt)


def build_scorer(model_dir: str, device="cuda", share_prefixes=False, context_cache_tokens=0, max_positions=None, *,
                 linear_weights="dense", expert_weights="dense", dtype=None):
    """The scorer of the checkpoint in model_dir by config.json's model_type: the row of FAMILIES that serves it (the one
    list of the supported families: OPT, GPT-2, GPT-NeoX / Pythia, Llama / Mistral / Qwen2 / Qwen3, OLMo-2, Mixtral, Gemma-2,
    Phi-3 / Phi-4, gpt-oss, each with its scorer class).  Anything else ("olmo", "olmo3", "gemma", "gemma3", "qwen3_moe", "phi",
    "phimoe" and "phi3small" included) is refused.
    max_positions caps the rotary table of every LlamaScorer.  dtype (the family's rule: clm_dtype for every LlamaScorer, fp16
    alone for OPT, GPT-2 and GPT-NeoX): None or "float16", "bfloat16" (without a context cache), or "auto" = the dtype
    config.json says the checkpoint was saved in (bfloat16 -> bfloat16; anything else, and every fp16-only family -> float16).
    A dtype or a context cache that is refused (gpt-oss has no cache, nor has bfloat16, nor a device without GPU memory) is
    refused before any weight is read.
    expert_weights (by keyword, like dtype behind it): "dense" (the default) expands a gpt-oss checkpoint's MXFP4 experts to the compute dtype, four times their
    published size; "mxfp4" keeps them packed in host and device memory and unpacks them in the grouped GEMM (GptOssMxScorer:
    the same scores to the byte).  "mxfp4" for another family, or for a gpt-oss checkpoint in the plain spelling (by the name of
    the _blocks tensor it lacks), is refused before any weight is expanded.
    A Llama / Mistral / Qwen2 / Qwen3 checkpoint in the fine-grained FP8 spelling (config.json's quantization_config with
    quant_method "fp8", fmt "e4m3" or none, weight_block_size [bn, bk], bn a multiple of 32 and bk of 64; every quantised linear
    a float8_e4m3fn weight beside an fp32 weight_scale_inv; activation_scheme is ignored, for this scorer quantises no
    activation) is read by fp8_block / fp8_dequant.  linear_weights (by keyword): "dense" (the default) expands it into the
    compute dtype, dequantise then cast as HF does, into the layout of any other checkpoint; "fp8" keeps the four projections
    of every layer packed in host and device memory, one byte a weight plus the scales, and unpacks them in the tile GEMM
    (Fp8LlamaScorer: the same scores to the byte, weight_bytes() the bytes held).  Every other quant_method or fmt, a block the
    kernels cannot follow, "fp8" for another family or for a checkpoint without the FP8 quantization_config, and "fp8" with
    bfloat16 and a context cache are refused before any weight is read; a NaN code, a scale or a value that is not finite in the
    compute dtype, a shape the block does not divide and a half-packed GEMM are refused by the tensor's name."""
    cfg = load_config(model_dir)
    mt = cfg.get("model_type", "opt")
    fam = FAMILIES.get(mt)
    if fam is None:
        raise ValueError(f"model_type {mt!r} is not supported (opt, gpt2, gpt_neox, {', '.join(LLAMA_MODEL_TYPES)}, gemma2, phi3, "
                         f"gpt_oss, olmo2, mixtral)")
    fp8_block(cfg)   # refuses the quantization_configs that nothing here reads
    fam = _family_for(fam, expert_weights, linear_weights, cfg)
    # every refusal that needs no weight, before the weights are read
    if not fam.scorer._CONTEXT_CACHE:
        gptoss_check_cache(context_cache_tokens)
    wdt = fam.dtype(dtype, cfg)
    if issubclass(fam.scorer, LlamaScorer):
        llama_check_dtype_cache(wdt, context_cache_tokens)
        LlamaScorer.check_cache_device(device, context_cache_tokens)
    dims, arrays = _load_arrays(fam, model_dir, max_positions, wdt)
    return fam.scorer(dims, arrays, device, share_prefixes, context_cache_tokens, wdt)


def build_opt(model_name="facebook/opt-6.7b", cache_dir=None, device="cuda", share_prefixes=False, context_cache_tokens=0,
              max_positions=None, *, linear_weights="dense", expert_weights="dense", dtype=None):
    """(scorer, tokenizer) from a local checkpoint; weights converted once into the device layout (fp16, or bf16 for a
    LlamaScorer's checkpoint with dtype="bfloat16" or, saved in bfloat16, dtype="auto").  The scorer is build_scorer's: its
    docstring lists the families.
    share_prefixes=True makes the scorer compute each distinct candidate prefix (the decoding context included) once;
    context_cache_tokens > 0 also keeps the context's keys / values / log-probs across calls (either scorer; GPU memory).
    expert_weights="mxfp4" keeps a gpt-oss checkpoint's experts packed, linear_weights="fp8" the projections of a Llama-family
    checkpoint in the fine-grained FP8 spelling (build_scorer)."""
    model_dir = resolve_model_dir(model_name, cache_dir)
    scorer = build_scorer(model_dir, device, share_prefixes, context_cache_tokens, max_positions, expert_weights=expert_weights,
                          linear_weights=linear_weights, dtype=dtype)
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(model_dir, local_files_only=True)
    tok.padding_side = "right"
    if tok.pad_token is None:
        tok.pad_token = tok.eos_token
    return scorer, tok


class WordTokenizer:
    """A whitespace word-level tokenizer with the call shape of a HF tokenizer (input_ids / attention_mask, BOS first): id =
    a fixed table entry, else a CRC32 bucket.  For synthetic models (tests, benchmarks) that have no BPE files."""

    def __init__(self, vocab_size: int, bos_id: int = 2, pad_id: int = 1, first_id: int = 4, words: Sequence[str] = ()):
        self.vocab_size, self.bos_id, self.pad_id, self.first_id = vocab_size, bos_id, pad_id, first_id
        self.table = {w: first_id + i for i, w in enumerate(words)}

    def word_id(self, w: str) -> int:
        import zlib
        if w in self.table:
            return self.table[w]
        return self.first_id + zlib.crc32(w.encode()) % (self.vocab_size - self.first_id)

    def __call__(self, texts, return_tensors=None, padding=False):
        if isinstance(texts, str):
            texts = [texts]
        rows = [[self.bos_id] + [self.word_id(w) for w in t.split()] for t in texts]
        if padding or return_tensors is not None:
            n = max(len(r) for r in rows)
            mask = [[1] * len(r) + [0] * (n - len(r)) for r in rows]
            rows = [r + [self.pad_id] * (n - len(r)) for r in rows]
        else:
            mask = [[1] * len(r) for r in rows]
        if return_tensors == "pt":
            import torch
            return {"input_ids": torch.tensor(rows), "attention_mask": torch.tensor(mask)}
        if return_tensors == "np":
            return {"input_ids": np.array(rows), "attention_mask": np.array(mask)}
        return {"input_ids": rows, "attention_mask": mask}
