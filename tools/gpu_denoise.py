#!/usr/bin/env python3
"""What swt_denoise_plan_dev and swt_denoise_rows_dev cost next to torch ops that make the same arrays, and next to
swt_mlm_mask_dev on the same rows (needs an MI355X).

S85k-open, FastBPE ids of bench.py's 8,000-merge table with [CLS] and [SEP]: packed "whole" at width 512, and one sentence per
row at width 64.  Noise density 0.15, geometric lengths of mean 3 cut at 10, whole words, 100 sentinels behind the vocabulary.
Legs that alternate round after round, HIP events around enough back-to-back calls for 0.2 s: the plan, the rows in the three
modes (without info, as corrupt_spans calls them behind a plan), swt_mlm_mask_dev without info or `selected` -- in MASK mode the
two read and write the same bytes --, and torch ops on the device for the three modes: cumsum and cummax for the units and the
reach, masked scatters for the two compactions.  The library's first 256 rows are compared with the plain-Python model of the
tests before the timing; torch's generator is not Philox by position, so the torch legs are held to their noise share only.
Prints one JSON line per shape; --out FILE appends the lines."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DENSITY, MEAN, LONGEST, N_SENTINEL, CHECK_ROWS = 0.15, 3.0, 10, 100, 256


def torch_noise(torch, ids, d_cls, start_p, d_cdf):
    """-> (noise, run start, run number per column) with torch ops on the device; whole words"""
    cls = d_cls[ids.to(torch.int64)]
    eligible = cls < 2
    left = torch.nn.functional.pad(cls[:, :-1], (1, 0), value=2)
    head = (cls == 0) | ((cls == 1) & (left == 2))
    unit = torch.cumsum(head, dim=1) - 1
    start = head & (torch.rand(ids.shape, device=ids.device) < start_p)
    length = 1 + torch.searchsorted(d_cdf, torch.rand(ids.shape, device=ids.device), right=True)
    reach = torch.cummax(torch.where(start, unit + length, torch.zeros_like(unit)), dim=1).values
    noise = eligible & (reach > unit)
    first = noise & ~torch.nn.functional.pad(noise[:, :-1], (1, 0), value=False)
    return noise, first, torch.cumsum(first, dim=1) - 1


def by_torch(torch, mode, ids, d_cls, start_p, d_cdf, mask_id, pad_id, d_sent):
    noise, first, k = torch_noise(torch, ids, d_cls, start_p, d_cdf)
    if mode == "mask":
        return torch.where(noise, torch.full_like(ids, mask_id), ids), torch.where(noise, ids, torch.full_like(ids, -100)), noise
    rows, width = ids.shape
    mark = d_sent[k.clamp(0, N_SENTINEL - 2)].to(ids.dtype) if mode == "sentinel" else torch.full_like(ids, mask_id)
    keep = ~noise | first
    pos = torch.cumsum(keep, dim=1) - 1
    r = torch.arange(rows, device=ids.device)[:, None].expand(ids.shape)
    out, mask = torch.full_like(ids, pad_id), torch.zeros(ids.shape, dtype=torch.uint8, device=ids.device)
    value = torch.where(first, mark, ids)
    out[r[keep], pos[keep]] = value[keep]
    mask[r[keep], pos[keep]] = (first | (ids != pad_id))[keep].to(torch.uint8)
    if mode == "infill":
        return out, mask, keep.sum(dim=1), noise
    takes = noise.to(torch.int64) + first
    lpos = torch.cumsum(takes, dim=1) - takes
    lab_len = takes.sum(dim=1) + 1
    labels = torch.full((rows, int(lab_len.max())), -100, dtype=ids.dtype, device=ids.device)
    labels[r[first], lpos[first]] = mark[first]
    labels[r[noise], (lpos + first)[noise]] = ids[noise]
    labels[torch.arange(rows, device=ids.device), lab_len - 1] = d_sent[first.sum(dim=1).clamp(max=N_SENTINEL - 1)].to(ids.dtype)
    return out, mask, keep.sum(dim=1), labels, lab_len, noise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import batching, synth, tokenizers
    from tests import denoise_cases as D

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    voc = tok._batch_vocabulary()
    sents = synth.s85k_open(args.sentences)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    n_class, mask_id, pad_id = int(voc.cls_tab.size), int(voc.mask_id), int(voc.special["pad"])
    sent = np.arange(n_class + 1, n_class + 1 + N_SENTINEL, dtype=np.uint32)
    d_cls, d_rand, d_sent = (torch.from_numpy(a).cuda() for a in (voc.cls_tab, voc.rand_ids.view(np.int32), sent.view(np.int32)))
    _, start_below, len_below = batching._denoise_thresholds("sentinel", DENSITY, MEAN, "geometric", LONGEST)
    start_p, d_cdf = start_below / 2.0 ** 32, torch.tensor([b / 2.0 ** 32 for b in len_below], device="cuda")
    modes = {"mask": N.DENOISE_MASK, "sentinel": N.DENOISE_SENTINEL, "infill": N.DENOISE_INFILL}
    mlm = N.mlm_spec(n_class, mask_id, int(DENSITY * 2 ** 32), int(0.8 * 2 ** 32), int(0.8 * 2 ** 32), seed=2024)
    shapes = (("whole_512", {"max_length": 512, "packing": "whole"}), ("one_per_row_64", {"max_length": 64, "padding": "max_length"}))
    lines = []
    for name, kw in shapes:
        ids = tok.encode_batch(sents, device=True, **kw)["input_ids"].contiguous()
        rows, width = (int(x) for x in ids.shape)
        h_ids = ids[:CHECK_ROWS].cpu().numpy()
        d_info = torch.zeros(7, dtype=torch.int64, device="cuda")
        spec = lambda mode, label_width: N.denoise_spec(modes[mode], n_class, mask_id, pad_id, start_below, len_below, N_SENTINEL, label_width,
                                                        seed=2024, epoch=0, whole_word=True)
        N.check(lib.swt_denoise_plan_dev(ids.data_ptr(), rows, width, d_cls.data_ptr(), C.byref(spec("sentinel", 2 ** 32 - 1)), d_info.data_ptr(), stream))
        info = [int(x) for x in d_info.cpu().numpy()]
        label_width = info[6]
        o_ids, o_lab, o_mask = torch.empty_like(ids), torch.empty((rows, max(width, label_width)), dtype=ids.dtype, device="cuda"), \
            torch.empty(ids.shape, dtype=torch.uint8, device="cuda")
        o_len, o_lab_len = torch.empty(rows, dtype=torch.int32, device="cuda"), torch.empty(rows, dtype=torch.int32, device="cuda")
        specs = {m: spec(m, label_width) for m in modes}

        def plan():
            N.check(lib.swt_denoise_plan_dev(ids.data_ptr(), rows, width, d_cls.data_ptr(), C.byref(specs["sentinel"]), d_info.data_ptr(), stream))

        def ours(mode):
            squeeze, sentinel = mode != "mask", mode == "sentinel"
            N.check(lib.swt_denoise_rows_dev(ids.data_ptr(), rows, width, d_cls.data_ptr(), d_sent.data_ptr(), C.byref(specs[mode]), o_ids.data_ptr(),
                                             o_mask.data_ptr() if squeeze else None, o_len.data_ptr() if squeeze else None,
                                             o_lab.data_ptr() if mode != "infill" else None, o_lab_len.data_ptr() if sentinel else None, None, stream))

        def mlm_mask():
            N.check(lib.swt_mlm_mask_dev(ids.data_ptr(), rows, width, d_cls.data_ptr(), d_rand.data_ptr(), int(d_rand.numel()), C.byref(mlm),
                                         o_ids.data_ptr(), o_lab.data_ptr(), None, None, stream))

        out = {"shape": name, "corpus": "S85k-open", "sentences": len(sents), "rows": rows, "width": width, "noise_density": DENSITY,
               "mean_span_length": MEAN, "max_span_length": LONGEST, "sentinels": N_SENTINEL, "label_width": label_width,
               "info": dict(zip(batching.DENOISE_COUNTS, info)), "noise_share": round(info[1] / info[0], 5), "torch_noise_share": {}}
        for mode, m in modes.items():  # the first rows against the model, element by element
            ours(mode)
            torch.cuda.synchronize()
            want = D.expected(h_ids, voc.cls_tab, dict(D.spec(m, start_below, len_below, seed=2024, n_sentinel=N_SENTINEL, label_width=label_width),
                                                       n_class=n_class, mask_id=mask_id, pad_id=pad_id), sent)
            got = {"input_ids": o_ids, "attention_mask": o_mask, "length": o_len, "label_length": o_lab_len,
                   "labels": o_lab.view(-1)[:rows * want["labels"].shape[1]].view(rows, -1) if want["labels"] is not None else None}
            for what, a in want.items():
                if a is not None and what != "info" and not np.array_equal(got[what][:CHECK_ROWS].cpu().numpy().astype(a.dtype), a):
                    raise AssertionError("%s, %s: %s of swt_denoise_rows_dev differs from the model" % (name, mode, what))
            noise = by_torch(torch, mode, ids, d_cls, start_p, d_cdf, mask_id, pad_id, d_sent)[-1]
            out["torch_noise_share"][mode] = round(int(noise.sum()) / info[0], 5)

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps

        legs = {"denoise_plan_dev": plan, "mlm_mask_dev": mlm_mask}
        legs.update(("denoise_rows_dev_" + m, lambda m=m: ours(m)) for m in modes)
        legs.update(("torch_" + m, lambda m=m: by_torch(torch, m, ids, d_cls, start_p, d_cdf, mask_id, pad_id, d_sent)) for m in modes)
        reps = {k: max(1, int(np.ceil(200.0 / max(timed(fn, 5), 1e-3)))) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            t = {k: timed(fn, reps[k]) for k, fn in legs.items()}
            if r >= args.warmup:
                for k, v in t.items():
                    ms[k].append(v)
        out.update({"calls_per_window": reps, "rounds": args.rounds, "legs": {}})
        for leg, v in ms.items():
            med = statistics.median(v)
            out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
        for m in modes:
            out["legs"]["torch_" + m]["ratio_to_denoise_rows_dev"] = round(
                out["legs"]["torch_" + m]["median_ms"] / out["legs"]["denoise_rows_dev_" + m]["median_ms"], 1)
        out["legs"]["denoise_rows_dev_mask"]["ratio_to_mlm_mask_dev"] = round(
            out["legs"]["denoise_rows_dev_mask"]["median_ms"] / out["legs"]["mlm_mask_dev"]["median_ms"], 3)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
