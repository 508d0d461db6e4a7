#!/usr/bin/env python3
"""What swt_mlm_mask_dev costs next to torch ops that make the same three arrays (needs an MI355X).

S85k-open, FastBPE ids of bench.py's 8,000-merge table with [CLS] and [SEP]: packed "whole" at width 512, and one sentence per
row at width 64.  Legs that alternate round after round, HIP events around enough back-to-back calls for 0.2 s: swt_mlm_mask_dev
with whole words, the same per token, and input_ids / labels / selected from torch ops on the device -- per token torch.rand and
where, whole words by the heads' cummax and a gather.  The library's result is compared with the NumPy model of the tests
element by element before the timing; torch's generator is not Philox by position, so the torch legs are held to the structural
properties and the shares instead.  Prints one JSON line per shape; --out FILE appends the lines."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_COPY_GB_S = 6290.0
PROBABILITY, MASK_SHARE, RANDOM_SHARE = 0.15, 0.8, 0.1


def by_torch(torch, ids, d_cls, d_rand, mask_id, whole_word):
    """-> (input_ids, labels, selected uint8, head column per column) with torch ops on the device"""
    cls = d_cls[ids.to(torch.int64)]
    eligible = cls < 2
    u = torch.rand(ids.shape, device=ids.device)
    hc = None
    if whole_word:
        left = torch.nn.functional.pad(cls[:, :-1], (1, 0), value=2)
        head = (cls == 0) | ((cls == 1) & (left == 2))
        col = torch.arange(ids.shape[1], device=ids.device, dtype=torch.int64).expand(ids.shape)
        hc = torch.cummax(torch.where(head, col, torch.zeros_like(col)), dim=1).values
        u = torch.gather(u, 1, hc)
    selected = eligible & (u < PROBABILITY)
    v = torch.rand(ids.shape, device=ids.device)
    masked = selected & (v < MASK_SHARE)
    random = selected & ~masked & (v < MASK_SHARE + RANDOM_SHARE)
    drawn = d_rand[torch.randint(int(d_rand.numel()), ids.shape, device=ids.device)]
    out = torch.where(masked, torch.full_like(ids, mask_id), torch.where(random, drawn, ids))
    labels = torch.where(selected, ids, torch.full_like(ids, -100))
    return out, labels, selected.to(torch.uint8), hc


def within(share, q, n, what):
    sigma = math.sqrt(q * (1 - q) / n)
    if abs(share - q) > 4 * sigma:
        raise AssertionError("%s: share %.5f is %.1f sigma off %.2f" % (what, share, (share - q) / sigma, q))
    return round(share, 5)


def check_torch_leg(torch, ids, d_cls, n_rand, mask_id, got, whole_word):
    """the structural properties and the shares of a torch leg -> its shares"""
    out, labels, selected, hc = got
    sel = selected.bool()
    cls = d_cls[ids.to(torch.int64)]
    assert not sel[cls == 2].any(), "a special was selected"
    assert torch.equal(labels[sel], ids[sel]) and bool((labels[~sel] == -100).all()) and torch.equal(out[~sel], ids[~sel])
    eligible = cls < 2
    if whole_word:
        assert torch.equal(sel[eligible], torch.gather(sel, 1, hc)[eligible]), "a word was selected in part"
        heads = eligible & (hc == torch.arange(ids.shape[1], device=ids.device).expand(ids.shape))
        n, k = int(heads.sum()), int((heads & sel).sum())
    else:
        n, k = int(eligible.sum()), int(sel.sum())
    n_sel = int(sel.sum())
    n_mask = int((sel & (out == mask_id)).sum())
    n_new = int((sel & (out != mask_id) & (out != ids)).sum())  # a random id that equals the id it replaces shows as kept: 1 in n_rand
    return {"selected": within(k / n, PROBABILITY, n, "selected"), "masked": within(n_mask / n_sel, MASK_SHARE, n_sel, "masked"),
            "random": within(n_new / n_sel, RANDOM_SHARE * (1 - 1.0 / n_rand), n_sel, "random")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sentences", type=int, default=85000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from subword_tokenizers_amd import _native as N
    from subword_tokenizers_amd import synth, tokenizers
    from tests import mlm_cases as M

    N.init(0)
    tok = tokenizers.FastBPE()
    tok.merges_list = list(synth.pretrained_merges()[:8000])
    tok._build_table()
    voc = tok._batch_vocabulary()
    sents = synth.s85k_open(args.sentences)
    stream = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    d_cls, d_rand = torch.from_numpy(voc.cls_tab).cuda(), torch.from_numpy(voc.rand_ids.view(np.int32)).cuda()
    n_class, mask_id = int(voc.cls_tab.size), int(voc.mask_id)
    select_below, mask_below, random_below = M.thresholds(PROBABILITY, MASK_SHARE, RANDOM_SHARE)
    shapes = (("whole_512", {"max_length": 512, "packing": "whole"}), ("one_per_row_64", {"max_length": 64, "padding": "max_length"}))
    lines = []
    for name, kw in shapes:
        ids = tok.encode_batch(sents, device=True, **kw)["input_ids"].contiguous()
        rows, width = (int(x) for x in ids.shape)
        h_ids = ids.cpu().numpy()
        o_ids, o_lab = torch.empty_like(ids), torch.empty_like(ids)
        o_sel, d_info = torch.empty(ids.shape, dtype=torch.uint8, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda")
        specs = {w: N.mlm_spec(n_class, mask_id, select_below, mask_below, random_below, seed=2024, epoch=0, whole_word=w) for w in (True, False)}

        def ours(whole_word, counts=True):
            N.check(lib.swt_mlm_mask_dev(ids.data_ptr(), rows, width, d_cls.data_ptr(), d_rand.data_ptr(), int(d_rand.numel()),
                                         C.byref(specs[whole_word]), o_ids.data_ptr(), o_lab.data_ptr(), o_sel.data_ptr(),
                                         d_info.data_ptr() if counts else None, stream))

        out = {"shape": name, "corpus": "S85k-open", "sentences": len(sents), "rows": rows, "width": width, "probability": PROBABILITY,
               "mask_share": MASK_SHARE, "random_share": RANDOM_SHARE, "class_table_bytes": n_class, "random_ids": int(d_rand.numel()),
               "counts": {}, "torch_shares": {}}
        for whole_word in (True, False):
            key = "whole_word" if whole_word else "per_token"
            ours(whole_word)
            torch.cuda.synchronize()
            want = M.expected_mlm(h_ids, voc.cls_tab, voc.rand_ids, M.spec(n_class, mask_id, PROBABILITY, whole_word, 2024, 0, MASK_SHARE, RANDOM_SHARE))
            for what, a in (("input_ids", o_ids), ("labels", o_lab), ("selected", o_sel), ("info", d_info)):
                if not np.array_equal(a.cpu().numpy(), want[what].view(np.int64) if what == "info" else want[what]):
                    raise AssertionError("%s, %s: %s of swt_mlm_mask_dev differs from the model" % (name, key, what))
            out["counts"][key] = {k: want[k] for k in M.COUNTS}
            out["torch_shares"][key] = check_torch_leg(torch, ids, d_cls, int(d_rand.numel()), mask_id, by_torch(torch, ids, d_cls, d_rand, mask_id, whole_word), whole_word)

        def timed(fn, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record(); e1.synchronize()
            return e0.elapsed_time(e1) / reps

        legs = {"mlm_mask_dev_whole_word": lambda: ours(True), "mlm_mask_dev_per_token": lambda: ours(False),
                "mlm_mask_dev_whole_word_without_info": lambda: ours(True, False),
                "torch_whole_word": lambda: by_torch(torch, ids, d_cls, d_rand, mask_id, True),
                "torch_per_token": lambda: by_torch(torch, ids, d_cls, d_rand, mask_id, False)}
        reps = {k: max(1, int(np.ceil(200.0 / max(timed(fn, 10), 1e-3)))) for k, fn in legs.items()}
        ms = {k: [] for k in legs}
        for r in range(args.warmup + args.rounds):
            t = {k: timed(fn, reps[k]) for k, fn in legs.items()}
            if r >= args.warmup:
                for k, v in t.items():
                    ms[k].append(v)
        cells, size = rows * width, ids.element_size()
        read_b, write_b = cells * size, cells * (2 * size + 1)  # the ids; ids, labels and selected.  The class table stays in L2
        out.update({"calls_per_window": reps, "rounds": args.rounds, "bytes_read": read_b, "bytes_written": write_b, "legs": {}})
        for leg, v in ms.items():
            med = statistics.median(v)
            out["legs"][leg] = {"ms": [round(x, 4) for x in v], "median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4)}
            if leg.startswith("mlm_mask_dev"):
                out["legs"][leg]["gb_s"] = round((read_b + write_b) / 1e6 / med, 1)
                out["legs"][leg]["share_of_hbm_copy"] = round(out["legs"][leg]["gb_s"] / HBM_COPY_GB_S, 4)
        for kind in ("whole_word", "per_token"):
            out["legs"]["torch_" + kind]["ratio_to_mlm_mask_dev"] = round(
                out["legs"]["torch_" + kind]["median_ms"] / out["legs"]["mlm_mask_dev_" + kind]["median_ms"], 1)
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a", encoding="utf-8") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
