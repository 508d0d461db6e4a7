#!/usr/bin/env python3
"""What swt_word_plan_dev, swt_word_predict_dev and swt_entity_spans_dev cost next to torch ops that make the same arrays on the
device (needs an MI355X).

Two shapes, both FastBPE ids of bench.py's 8,000-merge table with nine labels: S85k-open, one sentence per row at width 64; and
the question / context rows of tools/gpu_labels.py -- 6,000 sentences as questions, twelve more each as the context, width 384,
stride 128, only_second -- whose words, the context's, show up in overlapping windows.  The logits are normal values.  The torch
legs: for the plan a row maximum and scatter_reduce over the rows of a text, then a cumsum; for the words first columns by the
left neighbour, the run lengths by scatter_add, a key (context, then the earlier cell) reduced per word by scatter_reduce, a
gather of the owners' first columns, softmax and argmax; for the entities a head flag, its cumsum and scatter_reduce per entity.
Before the timing both legs must give the same arrays (scores to 1e-5).  Legs alternate round after round, HIP events around
enough back-to-back calls for 0.2 s.  Prints one JSON line per call and shape; --out FILE appends the lines."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, STRIDE, SPAN, LABELS = 384, 128, 12, 9
HBM_GBPS = 8000.0  # the data sheet's peak; a float4 copy reaches about 6,300


def torch_plan(torch, word, tok, sample, n_texts):
    per_row = torch.where(tok, word, -1).amax(1).long() + 1
    n_words = torch.zeros(n_texts, dtype=torch.int64, device=word.device).scatter_reduce(0, sample, per_row, "amax")
    return torch.nn.functional.pad(n_words.cumsum(0), (1, 0))


def torch_words(torch, logits, word, tok, sample, word_off, n_words):
    """strategy "first": -> label, score, row, col, n_tokens per word (every word has a run)"""
    rows, width = word.shape
    left_w = torch.nn.functional.pad(word[:, :-1], (1, 0), value=-1)
    left_t = torch.nn.functional.pad(tok[:, :-1], (1, 0), value=False)
    first = tok & (~left_t | (left_w != word))
    run = first.flatten().cumsum(0) - 1  # the run of a token column
    n_runs = int(run[-1]) + 1
    ncols = torch.zeros(n_runs, dtype=torch.int64, device=word.device).scatter_add_(0, run[tok.flatten()], torch.ones_like(run[tok.flatten()]))
    before = tok.cumsum(1) - tok.long()
    r, c = first.nonzero(as_tuple=True)
    left = before[r, c]
    context = torch.minimum(left, tok.sum(1)[r] - left - ncols)
    cells = rows * width
    key = context * cells + (cells - 1 - (r * width + c))
    at = word_off[sample[r]] + word[r, c].long()
    best = torch.zeros(n_words, dtype=torch.int64, device=word.device).scatter_reduce(0, at, key, "amax", include_self=False)
    own = key == best[at]
    r, c, at, ncols = r[own], c[own], at[own], ncols[own]
    x = logits[r, c]
    top, label = x.max(1)
    score = 1.0 / torch.exp(x - top[:, None]).sum(1)
    out = [torch.empty(n_words, dtype=t, device=word.device) for t in (torch.int64, torch.float32, torch.int64, torch.int64, torch.int64)]
    for o, v in zip(out, (label, score, r, c, ncols)):
        o[at] = v
    return out


def torch_entities(torch, label, score, char_start, char_end, word_off, etype, begins):
    """-> count, then text, type, first_word, last_word, char_start, char_end, score per entity"""
    n = label.shape[0]
    t = etype[label.long()]
    starts = word_off[:-1][word_off[1:] > word_off[:-1]]
    first = torch.zeros(n, dtype=torch.bool, device=label.device)
    first[starts] = True
    before = torch.nn.functional.pad(t[:-1], (1, 0), value=-1)
    head = (t >= 0) & (first | (before != t) | (begins[label.long()] != 0))
    ent = head.cumsum(0) - 1
    count = int(ent[-1]) + 1
    inside = t >= 0
    w = torch.arange(n, device=label.device)
    at = head.nonzero(as_tuple=True)[0]
    last = torch.zeros(count, dtype=torch.int64, device=label.device).scatter_reduce(0, ent[inside], w[inside], "amax", include_self=False)
    total = torch.zeros(count, dtype=torch.float32, device=label.device).scatter_add_(0, ent[inside], score[inside])
    text = torch.searchsorted(word_off, at, right=True) - 1
    return count, [text, t[at], at - word_off[text], last - word_off[text], char_start[at], char_end[last], total / (last - at + 1).float()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--pairs", type=int, default=6000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    lib, stream = N.lib(), torch.cuda.current_stream().cuda_stream

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / reps

    def measure(legs):
        reps = {k: max(1, int(np.ceil(200.0 / max(timed(fn, 5), 1e-3)))) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            t = {k: timed(fn, reps[k]) for k, fn in legs.items()}
            if r >= args.warmup:
                for k, v in t.items():
                    ms[k].append(v)
        res = {k: {"ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                   "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for k, v in ms.items()}
        return reps, res

    def same(name, ours, theirs):
        for k, (a, b) in enumerate(zip(ours, theirs)):
            ok = torch.allclose(a, b, rtol=1e-5, atol=0) if b.dtype == torch.float32 else torch.equal(a.to(b.dtype), b)
            if not ok:
                raise AssertionError("%s: output %d of the library differs from the torch leg's" % (name, k))

    def ratio(legs, ours, theirs):
        legs[theirs]["ratio_to_" + ours] = round(legs[theirs]["median_ms"] / legs[ours]["median_ms"], 1)

    n = args.pairs
    sents, pair_sents = synth.s85k_open(args.sentences), synth.s85k_open(n * (1 + SPAN))
    contexts = [" ".join(pair_sents[n + SPAN * i:n + SPAN * (i + 1)]) for i in range(n)]
    shapes = (("S85k-open, one sentence per row", 0,
               lambda: tok.encode_batch(sents, max_length=64, padding="max_length", return_offsets=True, device=True)),
              ("question / context windows", 1,
               lambda: tok.encode_batch(pair_sents[:n], text_pairs=contexts, max_length=WIDTH, stride=STRIDE, truncation="only_second",
                                        return_overflowing=True, return_offsets=True, device=True, padding="max_length")))
    etype = torch.tensor([-1] + [k // 2 for k in range(LABELS - 1)], dtype=torch.int32, device="cuda")
    begins = torch.tensor([0] + [1 - k % 2 for k in range(LABELS - 1)], dtype=torch.uint8, device="cuda")
    lines = []
    for shape, side, make in shapes:
        batch = make()
        word, spans = batch["word_ids"].contiguous(), batch["offset_mapping"].contiguous()
        seq = batch["sequence_ids"].contiguous() if "sequence_ids" in batch else None
        rows, width = (int(x) for x in word.shape)
        if "overflow_to_sample_mapping" in batch:
            sample = batch["overflow_to_sample_mapping"].contiguous()
        else:
            sample = torch.arange(rows, dtype=torch.int32, device="cuda")
        n_texts = int(sample[-1]) + 1
        long_sample = sample.long()
        tokc = (seq == side) if seq is not None else (word >= 0)
        gen = torch.Generator(device="cuda").manual_seed(11)
        logits = torch.randn((rows, width, LABELS), device="cuda", generator=gen)
        p = lambda a: None if a is None else a.data_ptr()
        about = {"shape": shape, "rows": rows, "width": width, "texts": n_texts, "n_labels": LABELS, "rounds": args.rounds}

        # ---- the plan
        d_off, d_info = torch.empty(n_texts + 1, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")

        def plan():
            N.check(lib.swt_word_plan_dev(p(word), p(seq), side, p(sample), rows, width, n_texts, p(d_off), p(d_info), stream))

        plan()
        same("word_plan", (d_off,), (torch_plan(torch, word, tokc, long_sample, n_texts),))
        n_words = int(d_off[-1])
        reps, legs = measure({"word_plan_dev": plan,
                              "torch_amax_cumsum": lambda: torch_plan(torch, word, (seq == side) if seq is not None else (word >= 0), long_sample, n_texts)})
        ratio(legs, "word_plan_dev", "torch_amax_cumsum")
        lines.append(json.dumps(dict(about, call="swt_word_plan_dev", words=n_words, info=d_info[:2].tolist(), calls_per_window=reps, legs=legs)))
        print(lines[-1], flush=True)

        # ---- the words
        types = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
        o_words = {name: torch.empty(n_words, dtype=types[t], device="cuda") for name, t in N.WORD_OUT}

        def words(counts=True):
            N.check(lib.swt_word_predict_dev(p(logits), p(word), p(seq), side, p(sample), p(spans), rows, width, LABELS, p(d_off), n_texts, n_words,
                                             N.TAG_FIRST, *[p(o_words[name]) for name, _ in N.WORD_OUT], None, p(d_info) if counts else None, stream))

        words()
        info = d_info.tolist()
        assert info[1] == 0 and info[3] == 0, info  # every word has a run: the torch leg leaves no room for one without
        same("word_predict", [o_words[k] for k in ("label", "score", "row", "col", "n_tokens")],
             torch_words(torch, logits, word, tokc, long_sample, d_off, n_words))
        reps, legs = measure({"word_predict_dev": words, "word_predict_dev_without_info": lambda: words(False),
                              "torch_scatter_softmax": lambda: torch_words(torch, logits, word, (seq == side) if seq is not None else (word >= 0),
                                                                           long_sample, d_off, n_words)})
        ratio(legs, "word_predict_dev", "torch_scatter_softmax")
        nbytes = rows * width * LABELS * 4
        gbps = nbytes / legs["word_predict_dev"]["median_ms"] / 1e6
        lines.append(json.dumps(dict(about, call="swt_word_predict_dev", strategy="first", words=n_words, info=info, logits_bytes=nbytes,
                                     logits_gb_per_s=round(gbps, 1), share_of_hbm_peak=round(gbps / HBM_GBPS, 3), calls_per_window=reps, legs=legs)))
        print(lines[-1], flush=True)

        # ---- the entities
        o_ents = {name: torch.empty(n_words, dtype=types[t], device="cuda") for name, t in N.ENTITY_OUT}

        def entities():
            N.check(lib.swt_entity_spans_dev(*[p(o_words[k]) for k in ("label", "score", "char_start", "char_end")], p(d_off), n_texts, n_words,
                                             p(etype), p(begins), LABELS, *[p(o_ents[name]) for name, _ in N.ENTITY_OUT], p(d_info), stream))

        entities()
        info = d_info[:2].tolist()
        leg = lambda: torch_entities(torch, o_words["label"], o_words["score"], o_words["char_start"], o_words["char_end"], d_off, etype, begins)
        count, theirs = leg()
        assert count == info[0], (count, info)
        same("entity_spans", [o_ents[name][:count] for name, _ in N.ENTITY_OUT], theirs)
        reps, legs = measure({"entity_spans_dev": entities, "torch_cumsum_scatter": leg})
        ratio(legs, "entity_spans_dev", "torch_cumsum_scatter")
        lines.append(json.dumps(dict(about, call="swt_entity_spans_dev", words=n_words, info=info, calls_per_window=reps, legs=legs)))
        print(lines[-1], flush=True)
        del batch, word, spans, seq, logits, o_words, o_ents

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
