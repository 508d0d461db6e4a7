#!/usr/bin/env python3
"""What swt_label_words_dev, swt_answer_positions_dev and swt_answer_best_dev cost next to torch ops that make the same arrays on
the device (needs an MI355X).

Word labels: S85k-open, FastBPE ids of bench.py's 8,000-merge table, one sentence per row at width 64, a label for every word;
the torch leg is a gather over word_ids and a comparison with the left neighbour.  Answers: the question / context shape of
tools/gpu_pair_batches.py -- 6,000 of S85k-open's sentences as questions, twelve more each as the context -- through
encode_batch at width 384, stride 128, only_second; the torch legs are a masked max and min over the columns, and for the best
spans an `unfold`ed band of max_answer_length end logits behind every start, its maximum with the first index that reaches it, and
scatter_reduce over the rows of a text.  Before the timing both legs must give the same arrays.  Legs alternate round after
round, HIP events around enough back-to-back calls for 0.2 s.  Prints one JSON line per call; --out FILE appends the lines."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, STRIDE, SPAN, MAX_LEN = 384, 128, 12, 30
NONE = 0xFFFFFFFF


def torch_labels(torch, word, d_off, d_lab):
    """single rows, every word labelled: the label of a word on its first token, -100 elsewhere"""
    tok = word >= 0
    idx = d_off[:-1, None] + word.clamp(min=0).long()
    left = torch.nn.functional.pad(word[:, :-1], (1, 0), value=-1)
    return torch.where(tok & (left != word), d_lab[idx.clamp(max=d_lab.numel() - 1)], -100)


def torch_positions(torch, spans, tok, sample, ans):
    rows, width = tok.shape
    st, en = spans[..., 0].long(), spans[..., 1].long()
    a, e = ans[sample, 0][:, None], ans[sample, 1][:, None]
    col = torch.arange(width, device=tok.device).expand(rows, width)
    start = torch.where(tok & (st <= a), col, -1).amax(1)
    end = torch.where(tok & (en >= e), col, width).amin(1)
    c0, c1 = torch.where(tok, col, width).amin(1), torch.where(tok, col, -1).amax(1)
    holds = (c1 >= 0) & (a[:, 0] != NONE) & (a[:, 0] < e[:, 0])
    holds &= st.gather(1, c0.clamp(max=width - 1)[:, None])[:, 0] <= a[:, 0]
    holds &= en.gather(1, c1.clamp(min=0)[:, None])[:, 0] >= e[:, 0]
    return torch.where(holds, start, 0).int(), torch.where(holds, end, 0).int(), holds.to(torch.uint8)


def torch_best(torch, sl, el, spans, tok, sample, n_texts):
    """finite logits, every row with a candidate: the band of MAX_LEN ends behind every start, the first index of its maximum"""
    rows, width = sl.shape
    inf = float("inf")
    e = torch.nn.functional.pad(torch.where(tok, el, -inf), (0, MAX_LEN - 1), value=-inf).unfold(1, MAX_LEN, 1)
    flat = (torch.where(tok, sl, -inf)[:, :, None] + e).reshape(rows, -1)
    top = flat.amax(1)
    at = torch.where(flat == top[:, None], torch.arange(flat.shape[1], device=sl.device).expand_as(flat), flat.shape[1]).amin(1)
    i = at // MAX_LEN
    j = i + at % MAX_LEN
    best = torch.full((n_texts,), -inf, device=sl.device).scatter_reduce(0, sample, top, "amax")
    r = torch.arange(rows, device=sl.device)
    row = torch.full((n_texts,), rows, device=sl.device).scatter_reduce(0, sample, torch.where(top == best[sample], r, rows), "amin")
    null = torch.full((n_texts,), inf, device=sl.device).scatter_reduce(0, sample, sl[:, 0] + el[:, 0], "amin")
    return (best, null, row.int(), i[row].int(), j[row].int(), spans[row, i[row], 0], spans[row, j[row], 1])


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
    rng = np.random.default_rng(7)

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
            if not torch.equal(a.to(b.dtype), b):
                raise AssertionError("%s: output %d of the library differs from the torch leg's" % (name, k))

    lines = []
    # ---- word labels
    sents = synth.s85k_open(args.sentences)
    batch = tok.encode_batch(sents, max_length=64, padding="max_length", return_offsets=True, device=True)
    word = batch["word_ids"].contiguous()
    rows, width = (int(x) for x in word.shape)
    n_words = (word.amax(1) + 1).clamp(min=0).cpu().numpy().astype(np.int64)
    lab_off = np.concatenate([[0], np.cumsum(n_words)])
    d_off, d_lab = torch.from_numpy(lab_off).cuda(), torch.from_numpy(rng.integers(0, 9, size=int(lab_off[-1])).astype(np.int32)).cuda()
    o_lab, d_info = torch.empty((rows, width), dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")

    def labels(counts=True):
        N.check(lib.swt_label_words_dev(word.data_ptr(), None, 0, None, rows, width, d_off.data_ptr(), d_lab.data_ptr(), int(d_lab.numel()), rows,
                                        None, 0, -100, 0, o_lab.data_ptr(), None, d_info.data_ptr() if counts else None, stream))

    labels()
    same("label_words", (o_lab,), (torch_labels(torch, word, d_off, d_lab),))
    reps, legs = measure({"label_words_dev": labels, "label_words_dev_without_info": lambda: labels(False),
                          "torch_gather": lambda: torch_labels(torch, word, d_off, d_lab)})
    legs["torch_gather"]["ratio_to_label_words_dev"] = round(legs["torch_gather"]["median_ms"] / legs["label_words_dev"]["median_ms"], 1)
    lines.append(json.dumps({"call": "swt_label_words_dev", "corpus": "S85k-open", "rows": rows, "width": width, "words": int(lab_off[-1]),
                             "info": d_info.tolist(), "calls_per_window": reps, "rounds": args.rounds, "legs": legs}))
    print(lines[-1], flush=True)
    del batch, word, o_lab

    # ---- answers
    n = args.pairs
    sents = synth.s85k_open(n * (1 + SPAN))
    contexts = [" ".join(sents[n + SPAN * i:n + SPAN * (i + 1)]) for i in range(n)]
    batch = tok.encode_batch(sents[:n], text_pairs=contexts, max_length=WIDTH, stride=STRIDE, truncation="only_second", return_overflowing=True,
                             return_offsets=True, device=True, padding="max_length")
    spans, seq = batch["offset_mapping"].contiguous(), batch["sequence_ids"].contiguous()
    sample, length = batch["overflow_to_sample_mapping"].contiguous(), batch["length"].contiguous()
    rows, width = (int(x) for x in seq.shape)
    tokc = seq == 1
    # an answer per text from the context tokens of its first row: six tokens from a third of the way in; every seventh text none
    h_sample = sample.cpu().numpy()
    first = np.unique(h_sample, return_index=True)[1]
    h_tok, h_spans = tokc[first].cpu().numpy(), spans[first].cpu().numpy()
    ans = np.full((n, 2), NONE, dtype=np.int64)
    for t in range(n):
        c = np.flatnonzero(h_tok[t])
        if t % 7 != 6 and c.size:
            i = c[c.size // 3]
            ans[t] = (h_spans[t, i, 0], h_spans[t, min(i + 5, c[-1]), 1])
    d_ans64 = torch.from_numpy(ans).cuda()
    d_ans = torch.from_numpy(ans.astype(np.uint32).view(np.int32)).cuda()
    o_start, o_end = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")
    o_has, o_hit = torch.empty(rows, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
    d_info = torch.zeros(4, dtype=torch.int64, device="cuda")
    long_sample = sample.long()

    def positions():
        N.check(lib.swt_answer_positions_dev(spans.data_ptr(), None, seq.data_ptr(), 1, sample.data_ptr(), rows, width, d_ans.data_ptr(), n,
                                             length.data_ptr(), -100, N.ANSWER_CLS, o_start.data_ptr(), o_end.data_ptr(), o_has.data_ptr(),
                                             o_hit.data_ptr(), d_info.data_ptr(), stream))

    positions()
    same("answer_positions", (o_start, o_end, o_has), torch_positions(torch, spans, tokc, long_sample, d_ans64))
    reps, legs = measure({"answer_positions_dev": positions, "torch_masked_max_min": lambda: torch_positions(torch, spans, seq == 1, long_sample, d_ans64)})
    legs["torch_masked_max_min"]["ratio_to_answer_positions_dev"] = round(
        legs["torch_masked_max_min"]["median_ms"] / legs["answer_positions_dev"]["median_ms"], 1)
    lines.append(json.dumps({"call": "swt_answer_positions_dev", "corpus": "S85k-open", "pairs": n, "sentences_per_context": SPAN, "rows": rows,
                             "width": width, "stride": STRIDE, "info": d_info[:3].tolist(), "calls_per_window": reps, "rounds": args.rounds,
                             "legs": legs}))
    print(lines[-1], flush=True)

    gen = torch.Generator(device="cuda").manual_seed(11)
    sl, el = (torch.randn((rows, width), device="cuda", generator=gen) for _ in range(2))
    types = {np.float32: torch.float32, np.int32: torch.int32, np.uint32: torch.int32}
    o_text = [torch.empty(n, dtype=types[t], device="cuda") for _, t in N.BEST_TEXT]

    def best():
        N.check(lib.swt_answer_best_dev(sl.data_ptr(), el.data_ptr(), spans.data_ptr(), None, seq.data_ptr(), 1, sample.data_ptr(), rows, width, n,
                                        MAX_LEN, length.data_ptr(), N.ANSWER_CLS, *[o.data_ptr() for o in o_text], None, None, None,
                                        d_info.data_ptr(), stream))

    best()
    same("answer_best", o_text, torch_best(torch, sl, el, spans, tokc, long_sample, n))
    reps, legs = measure({"answer_best_dev": best, "torch_unfold_band": lambda: torch_best(torch, sl, el, spans, seq == 1, long_sample, n)})
    legs["torch_unfold_band"]["ratio_to_answer_best_dev"] = round(legs["torch_unfold_band"]["median_ms"] / legs["answer_best_dev"]["median_ms"], 1)
    lines.append(json.dumps({"call": "swt_answer_best_dev", "corpus": "S85k-open", "pairs": n, "rows": rows, "width": width, "stride": STRIDE,
                             "max_answer_length": MAX_LEN, "info": d_info[:2].tolist(), "calls_per_window": reps, "rounds": args.rounds,
                             "legs": legs}))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
